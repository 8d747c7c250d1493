#!/usr/bin/env python3
"""Times rover_obs_occlusion (both routes) on the GPU against a torch-ops restatement of the same definition, a plain copy of the
observation, rover_obs_noise on it and the student's act() (EXPERIMENTS.md §30).

    python tools/occlusion_timing.py [--envs 512 4096 65536] [--warmup 200] [--reps 20] [--torch-max 4096] [--profile-calls N] [--json out.json]

The scene is the Mars yard generated from seed 10, moved by the terrain-following motion model with the rocker-bogie posture, native
1 750-float observation; the rovers take --warmup random steps first so that they are spread and tilted.  Every figure is device-event
time per call: median (min .. max) over --reps windows, the functions alternating inside one process, each window long enough to dwarf
the events' own cost.  The two routes must agree bit for bit at every size; the torch restatement is compared with them up to
--torch-max envs and its agreement reported.  Also reported: the share of hidden columns and, from the restatement, the share of samples
a tile maximum answers.  --profile-calls N skips the timing and makes N calls per route instead (for a kernel trace or a counter run of
its own).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from isaac_rover_amd import _lib, assets, config, vec_env  # noqa: E402
from isaac_rover_amd.learning.noise import HeightmapNoise, HeightmapOcclusion  # noqa: E402

TILE = 8


def torch_occlusion(hm, hscale, vscale, shift, body, pos, quat, clean, first, occ, tiles=None, rcp=True):
    """The definition of include/rover_step.h in torch ops, one op per written operation (a tensor divisor: ATen turns a division by a
    Python scalar into a multiplication).  ``rcp``: the task's cell_index_mode, cuda_rcp by default.  -> (out, hidden, samples, samples a tile maximum answers)."""
    f32 = torch.float32
    dev = clean.device
    k_ = lambda v: torch.tensor(v, dtype=f32, device=dev)
    w, x, y, z = (quat[:, i:i + 1] for i in range(4))
    r = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
         [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
         [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]
    rot = lambda i, v0, v1, v2: (r[i][0] * v0 + r[i][1] * v1) + r[i][2] * v2
    cam = [pos[:, i:i + 1] + rot(i, *occ.camera) for i in range(3)]
    b = [body[None, :, i] for i in range(3)]
    v = clean[:, first:]
    d = 2.0 * v
    t3 = [(pos[:, i:i + 1] + rot(i, *b)) + d * (-r[i][2]) for i in range(3)]
    dx, dy, dz = (t3[i] - cam[i] for i in range(3))
    u = torch.ceil(torch.sqrt(dx * dx + dy * dy) / k_(occ.step))
    n = torch.where(u < occ.max_steps, u, k_(float(occ.max_steps)))
    n = torch.where(v.abs() < occ.miss, n, torch.zeros_like(n))
    hidden = torch.zeros_like(v, dtype=torch.bool)
    samples = answered = 0
    n0, n1 = hm.shape
    hs, hi = k_(hscale), float(n0 - 1)
    inv = k_(1.0) / hs
    node = lambda c, s: torch.round(torch.clamp((c - s) * inv if rcp else (c - s) / hs, 0.0, hi)).long()
    for k in range(1, int(n.max().item())):
        t = k_(float(k)) / n
        live = n > k
        line = (cam[2] + t * dz) + occ.clearance
        ix, iy = node(cam[0] + t * dx, shift[0]), node(cam[1] + t * dy, shift[1]).clamp_(max=n1 - 1)
        h = hm[ix, iy] * vscale
        hidden |= live & (h > line)
        if tiles is not None:
            samples += int(live.sum())
            answered += int((live & ~(tiles[ix // TILE, iy // TILE] > line)).sum())
    out = clean.clone()
    out[:, first:] = torch.where(hidden, torch.full_like(v, occ.drop_value), v)
    return out, hidden, samples, answered


def timed(fns, reps, inner):
    """{name: (median, min, max)} microseconds per call: every round one event-bracketed window of ``inner[name]`` calls per function."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner[k]):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / inner[k])
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[512, 4096, 65536])
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-max", type=int, default=4096, help="the torch restatement runs up to this many envs")
    ap.add_argument("--profile-calls", type=int, default=0)
    ap.add_argument("--scene-seed", type=int, default=10)
    ap.add_argument("--spawn", choices=("task", "inside"), default="task",
                    help="task: where the task puts the rovers (x += 0.05 m while a stone is within 1.4 m: on the Mars yard that ends beyond the "
                         "yard's edge, on the heightfield's border); inside: the requested positions themselves, also after a reset")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("occlusion_timing: needs a GPU")
    from isaac_rover_amd.learning.student import StudentPolicy
    from isaac_rover_amd.tasks.rover import RoverTask
    scene = assets.example_scene("mars", args.scene_seed)
    extent = scene.terrain.map_indices.shape[0] * scene.terrain.cell_size
    result = {"version": _lib.version(), "envs": {}}
    for e in args.envs:
        env = vec_env.VecEnv(headless=True, sim="terrain", suspension="bogie")
        g = torch.Generator().manual_seed(0)
        spawn = torch.zeros(e, 3)
        spawn[:, 0:2] = 0.15 * extent + 0.7 * extent * torch.rand(e, 2, generator=g)
        task = RoverTask("Rover", config.SimConfig(num_envs=e, device="cuda:0"), env, scene=scene, distribution=None)
        env.set_task(task, sim_params={"dt": 0.05}, spawn_positions=spawn)
        dev = task.device
        if args.spawn == "inside":                          # in-place writes: the bound launch state keeps its addresses
            task.initial_pos[:, 0:2] = spawn[:, 0:2].to(dev)
            task.initial_pos[:, 2] = task._engine.sample_height(task.initial_pos[:, 0:2].contiguous()) + 0.5
            task._rover.set_world_poses(task.initial_pos, None)
        obs = env.reset()
        gd = torch.Generator(device=dev).manual_seed(1)
        for _ in range(args.warmup):
            obs, _, _, _ = env.step(2 * torch.rand(e, 2, device=dev, generator=gd) - 1)
        eng = task._engine
        occ = HeightmapOcclusion(eng, task)
        noise = HeightmapNoise(eng, task, sigma_point=0.05, sigma_offset=0.02, dropout=0.05, seed=3)
        clean = obs.clone()
        pos, quat = (t.clone() for t in task._rover.get_world_poses())
        first = clean.shape[1] - occ.columns
        out = [torch.empty_like(clean) for _ in range(2)]
        hidden = torch.zeros(e, occ.columns, dtype=torch.uint8, device=dev)

        def route(r, o=None, h=None):
            eng.set_option("occlusion_route", r)
            return occ.apply(clean, out=o, pos=pos, quat=quat, hidden=h)

        route(0, out[0], hidden)
        route(1, out[1])
        torch.cuda.synchronize()
        assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)), f"{e} envs: the two routes differ"
        rec = {"spawn": args.spawn, "on_the_map": float(((pos[:, :2] > 0) & (pos[:, :2] < extent)).all(1).float().mean()),
               "miss_share": float((clean[:, first:].abs() >= occ.miss).float().mean()), "hidden_share": float(hidden.float().mean()), "hidden_share_worst_env": float(hidden.float().mean(1).max())}
        if args.profile_calls:
            for r in (0, 1):
                for _ in range(args.profile_calls):
                    route(r, out[r])
            torch.cuda.synchronize()
            print(f"{e} envs: {args.profile_calls} calls per route made; hidden {rec['hidden_share']:.2%}")
            env.close()
            continue
        restate = None
        if e <= args.torch_max:
            hmap = task.Camera.heightmap
            cols = list(_lib._host(hmap.coarse_idx, "int64").reshape(-1)) + list(_lib._host(hmap.fine_idx, "int64").reshape(-1))
            body = torch.from_numpy(_lib._host(hmap.distribution, "float64")[cols]).float().to(dev)
            hm = scene.heightmap.to(dev).float()
            tiles = torch.nn.functional.max_pool2d(hm[None, None], TILE, ceil_mode=True)[0, 0] * scene.vertical_scale
            sh = scene.shift
            restate = lambda with_tiles=False: torch_occlusion(hm, scene.horizontal_scale, scene.vertical_scale, (float(sh[0]), float(sh[1])), body, pos,
                                                               quat, clean, first, occ, tiles if with_tiles else None)
            t_out, t_hidden, samples, answered = restate(True)
            rec["torch_agrees_bit_for_bit"] = bool(torch.equal(t_out.view(torch.int32), out[0].view(torch.int32)))
            rec["columns_where_torch_differs"] = int((t_hidden != hidden.bool()).sum())
            rec["samples_per_env"], rec["tile_answered_share"] = samples / e, answered / max(samples, 1)
        student = {p: StudentPolicy(eng, task, device=dev, precision=p) for p in ("f32", "bf16")}
        for s in student.values():
            s.init_hidden(e)
        fns = {"route0": lambda: route(0, out[0]), "route1": lambda: route(1, out[1]), "copy": lambda: out[0].copy_(clean),
               "obs_noise": lambda: noise.apply(clean, out=out[0]), "student_act_f32": lambda: student["f32"].act(clean),
               "student_act_bf16": lambda: student["bf16"].act(clean)}
        per = max(2, min(100, (1 << 19) // e))
        inner = {k: per for k in fns}
        if restate is not None:
            fns["torch_restatement"] = lambda: restate()
            inner["torch_restatement"] = 1
        times = timed(fns, args.reps, inner)
        rec.update({k: dict(median_us=v[0], min_us=v[1], max_us=v[2]) for k, v in times.items()})
        result["envs"][str(e)] = rec
        print(f"--- {e} envs, spawn {args.spawn}: {rec['on_the_map']:.1%} of the rovers on the map, {rec['miss_share']:.1%} of the columns at miss")
        print(f"--- {e} envs, obs {tuple(clean.shape)}: hidden {rec['hidden_share']:.2%} of the columns (worst env {rec['hidden_share_worst_env']:.2%})"
              + (f"; {rec['samples_per_env']:.0f} samples per env, {rec['tile_answered_share']:.2%} answered by a tile maximum; torch restatement "
                 f"{'agrees bit for bit' if rec['torch_agrees_bit_for_bit'] else 'DIFFERS in %d columns' % rec['columns_where_torch_differs']}" if restate else ""))
        for k, (med, lo, hi) in times.items():
            print(f"{k:20s} {med:12.2f} us ({lo:.2f} .. {hi:.2f})   {inner[k]} calls per window")
        env.close()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
