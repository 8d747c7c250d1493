#!/usr/bin/env python3
"""Times the pose feeders of vec_env on the GPU: TerrainSim.advance(1) (one rover_motion_step launch) against KinematicSim.step()
(about fifteen torch ops and a height lookup), both as VecEnv's world object would call them, on the same task (EXPERIMENTS.md §22),
and "bogie", TerrainSim(suspension="bogie").advance(1) (one rover_motion_step_bogie launch; EXPERIMENTS.md §29); "wheels" and
"wheels_bogie" are the same two with drive="wheels" (one rover_motion_step_drive launch; EXPERIMENTS.md §35), with ideal actuators
unless --steer-rate / --wheel-accel say otherwise.

    python tools/motion_timing.py [--envs 512 4096 65536] [--reps 30] [--feeders kinematic terrain bogie wheels wheels_bogie] [--json out.json]

Per size one task is built (synthetic scene, 37-ray distribution), stepped a few times with random actions so that the histories, the
joint targets and the poses are those of a rollout, and then each feeder is called in windows of --inner calls between two device
events; the windows of the two feeders alternate, so that a drift of the machine meets both.  A figure is the time of one call inside
such a window — enqueue cost included where the host is the limit, as in a rollout —: median (min .. max) over --reps windows.
"terrain_graph" / "bogie_graph" is the same window of TerrainSim calls captured once in a graph and replayed: the device's share of a
call, with no enqueue cost.  --feeders kinematic alone runs on a tree without TerrainSim, --feeders kinematic terrain on one without the
bogie mode.  Needs a GPU; there is no fallback."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from isaac_rover_amd import _lib, config, synth, vec_env  # noqa: E402
from isaac_rover_amd.tasks.rover import RoverTask  # noqa: E402


def window(fn, inner):
    """-> microseconds per call over one event-bracketed window of ``inner`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[512, 4096, 65536])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=200, help="calls per window")
    ap.add_argument("--feeders", nargs="+", choices=("kinematic", "terrain", "bogie", "wheels", "wheels_bogie"),
                    default=["kinematic", "terrain", "bogie", "wheels", "wheels_bogie"])
    ap.add_argument("--steer-rate", type=float, default=math.inf, help="wheels: rad/s")
    ap.add_argument("--wheel-accel", type=float, default=math.inf, help="wheels: rad/s^2")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("motion_timing: needs a GPU")
    scene = synth.make_scene(n_cells=600, k=200, n_stones=128, device="cuda")
    extent = scene.terrain.map_indices.shape[0] * scene.terrain.cell_size
    result = {"version": _lib.version(), "inner": args.inner, "reps": args.reps, "sizes": {}}
    for e in args.envs:
        env = vec_env.VecEnv(headless=True)
        task = RoverTask("Rover", config.SimConfig(num_envs=e, device="cuda:0"), env, scene=scene, distribution=synth.ray_distribution("37"))
        g = torch.Generator().manual_seed(0)
        spawn = torch.zeros(e, 3)
        spawn[:, 0:2] = 0.15 * extent + 0.7 * extent * torch.rand(e, 2, generator=g)
        env.set_task(task, sim_params={"dt": 0.05}, spawn_positions=spawn)
        env.reset()
        for _ in range(5):
            env.step(2 * torch.rand(e, 2, device=task.device) - 1)
        worlds = {"kinematic": lambda: vec_env.KinematicSim(task, dt=0.05), "terrain": lambda: vec_env.TerrainSim(task, dt=0.05),
                  "bogie": lambda: vec_env.TerrainSim(task, dt=0.05, suspension="bogie"),
                  "wheels": lambda: vec_env.TerrainSim(task, dt=0.05, drive="wheels", steer_rate=args.steer_rate, wheel_accel=args.wheel_accel),
                  "wheels_bogie": lambda: vec_env.TerrainSim(task, dt=0.05, suspension="bogie", drive="wheels", steer_rate=args.steer_rate,
                                                             wheel_accel=args.wheel_accel)}
        calls = {}
        for name in args.feeders:
            w = worlds[name]()
            calls[name] = (lambda w=w: w.step(render=False)) if name == "kinematic" else (lambda w=w: w.advance(1))
        pos, quat = task._rover.get_world_poses()
        jpos, jvel = task._rover.get_joint_positions(), task._rover.get_joint_velocities()
        start = (pos.clone(), quat.clone(), jpos.clone(), jvel.clone())
        graphs = {}
        for name in ("terrain", "bogie", "wheels", "wheels_bogie"):
            if name not in calls:
                continue
            for _ in range(3):
                calls[name]()
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(args.inner):
                    calls[name]()
        samples = {name: [] for name in calls}
        for name, fn in calls.items():                               # warm-up: every op's code object loaded
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, fn in calls.items():
                pos.copy_(start[0]), quat.copy_(start[1]), jpos.copy_(start[2]), jvel.copy_(start[3])      # every window starts from the same state
                torch.cuda.synchronize()
                samples[name].append(window(fn, args.inner))
            for name, graph in graphs.items():
                pos.copy_(start[0]), quat.copy_(start[1]), jpos.copy_(start[2]), jvel.copy_(start[3])
                torch.cuda.synchronize()
                samples.setdefault(name + "_graph", []).append(window(graph.replay, 1) / args.inner)
        rec = {name: (statistics.median(v), min(v), max(v)) for name, v in samples.items()}
        result["sizes"][str(e)] = rec
        print(f"--- {e} envs (us per call: median (min .. max); {args.inner} calls per window, {args.reps} windows, alternating)")
        for name, (med, lo, hi) in rec.items():
            print(f"{name:14s} {med:10.2f} ({lo:.2f} .. {hi:.2f})")
        env.close()
        del task, env
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
