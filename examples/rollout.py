#!/usr/bin/env python3
"""train.py-shaped rollout on the MI355X rover step path (no Isaac Sim, no learner).

Mirrors the loop of the reference's `omniisaacgymenvs/train.py:57-125` (env = load...("Rover"); trainer loop:
actions = agent.act(obs); obs, rew, done, info = env.step(actions)) with `vec_env.KinematicSim` standing in for PhysX and, for
the skrl PPO agent, either a random policy (`--policy random`, the default), the actor itself (`--policy actor`:
`StochasticActorHeightmap.act`, sampled on the GPU in the kernel that ends its forward; `--checkpoint` loads a `state_dict` saved
from the reference's module) or the recurrent student the teacher is distilled into (`--policy student`: `StudentPolicy.act(obs,
reset=done)`, the reference's `student_loader.act` with a carried GRU state; `--checkpoint best.pt` loads its `['state_dict']`).

    python examples/rollout.py --envs 4096 --steps 200 [--assets /path/to/omniisaacgymenvs] [--policy actor|student [--checkpoint actor.pt|best.pt]]

`--rollouts N` (with `--policy actor`) adds what skrl's PPO does around that loop up to the weight update: a `DeterministicHeightmap` critic,
a `RolloutMemory` of N steps (train.py:82, `rollouts: 60` in cfg/trainSKRL/RoverPPOSKRL.yaml:12) that stores states, actions, log_prob,
values, rewards and terminated every step, and every N steps `compute_gae` (one pass on the GPU) with the critic's value of the current
obs as `last_values`.
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from isaac_rover_amd import assets, config, synth, vec_env  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--assets", default="", help="directory holding the reference's tasks/utils/terrain/... files")
    ap.add_argument("--native-rays", action="store_true", help="the reference's 1634-point distribution (1750-float obs)")
    ap.add_argument("--policy", choices=("random", "actor", "student"), default="random",
                    help="random actions, StochasticActorHeightmap.act(obs), or StudentPolicy.act(obs, reset=done)")
    ap.add_argument("--checkpoint", default="", help="--policy actor: a state_dict of the reference's StochasticActorHeightmap (torch.save); "
                    "--policy student: the reference's best.pt (its ['state_dict'] is loaded)")
    ap.add_argument("--rollouts", type=int, default=0, help="--policy actor: store N steps in a RolloutMemory, then compute_gae (0 = off)")
    ap.add_argument("--precision", choices=("f32", "bf16"), default="f32",
                    help="--policy actor: what the actor and the critic act in (bf16: bf16 operands, f32 accumulation and head); "
                    "--policy student: what StudentPolicy.act runs in (bf16: every matrix product, the GRU state stays f32)")
    ap.add_argument("--obs-noise", type=float, default=0.0, help="--policy actor / student: standard deviation of Gaussian noise on the heightmap "
                    "columns the policy sees (rover_obs_noise; the task and its rewards keep the clean observation)")
    ap.add_argument("--obs-offset", type=float, default=0.0, help="... of a per-env, per-episode offset on them")
    ap.add_argument("--obs-dropout", type=float, default=0.0, help="... probability of a heightmap column reading 0")
    ap.add_argument("--occlusion", action="store_true",
                    help="--policy actor / student: heightmap columns whose measured point a camera on the mast cannot see read 0 "
                         "(rover_obs_occlusion: the line-of-sight stage of the sensor model, after the noise; the task keeps the clean observation)")
    ap.add_argument("--camera", type=float, nargs=3, default=(0.0, 0.0, 0.7), metavar=("F", "L", "U"), help="--occlusion: the camera in the body frame, metres")
    ap.add_argument("--sight-step", type=float, default=0.05, help="--occlusion: spacing of the samples along a sight line, metres")
    ap.add_argument("--sight-clearance", type=float, default=0.03, help="--occlusion: how far the ground must rise above the sight line to hide, metres")
    ap.add_argument("--sim", choices=("kinematic", "terrain"), default="kinematic",
                    help="what moves the rovers between two steps: vec_env.KinematicSim, a flat unicycle, or TerrainSim, the terrain-following "
                         "motion model (one rover_motion_step launch per control step: tilt from the ground under the wheels, joint state)")
    ap.add_argument("--suspension", choices=("plane", "bogie"), default="plane",
                    help="with --sim terrain: plane fits a plane through the six wheel contacts; bogie solves the rocker-bogie posture, which keeps "
                         "all six wheels down and writes the three passive joints (uprightness penalty, wheel-ray origins)")
    ap.add_argument("--drive", choices=("command", "wheels"), default="command",
                    help="with --sim terrain: command moves the body by the policy's command itself; wheels (rover_motion_step_drive) lets the "
                         "steering and drive joints follow Ackermann's targets at a limited rate and moves the body the way its six wheels roll")
    ap.add_argument("--wheel-radius", type=float, default=0.2,
                    help="--drive wheels: metres per radian of wheel turn; 0.2 is the length the reference's Ackermann divides by (the command's "
                         "speed), 0.1 the asset's physical radius, which halves every speed as the reference's rover in PhysX does")
    ap.add_argument("--steer-rate", type=float, default=math.inf,
                    help="--drive wheels: the steering joints' speed limit in rad/s; inf = ideal.  The repository holds no actuator limits for "
                         "the asset: a finite value such as 1.5 is this project's choice")
    ap.add_argument("--wheel-accel", type=float, default=math.inf,
                    help="--drive wheels: the drive joints' acceleration limit in rad/s^2; inf = ideal.  A finite value such as 20 is this "
                         "project's choice")
    ap.add_argument("--track-interval", type=int, default=0,
                    help="every N steps print the episode statistics kept on the device (learning/tracking.py:EpisodeTracker, one "
                         "rover_episode_track call per step, one read per N steps): skrl's nine Reward / Episode tags, the interval's exact "
                         "episode figures and the means of the eight reward components; 0 = off")
    ap.add_argument("--track-window", type=int, default=100, help="how many of the last finished episodes the Total reward / Total timesteps tags cover (skrl: 100)")
    ap.add_argument("--scene", choices=("synth", "mars"), default="synth",
                    help="without --assets: synth = the synthetic sine-and-discs scene; mars = a 60 m yard from the reference's Mars terrain "
                         "generator (assets.build_mars_scene: hills and rocks from --scene-seed, both KNN maps and the heightfield on the GPU)")
    ap.add_argument("--scene-seed", type=int, default=10, help="--scene mars: the generator's seed (10 = the reference's own)")
    args = ap.parse_args()
    if args.suspension != "plane" and args.sim != "terrain":
        ap.error("--suspension bogie needs --sim terrain")
    if args.drive != "command" and args.sim != "terrain":
        ap.error("--drive wheels needs --sim terrain")
    if args.track_interval < 0 or not 1 <= args.track_window <= 1024:
        ap.error("--track-interval N needs N >= 0, --track-window W needs W in 1 .. 1024")
    noisy = bool(args.obs_noise or args.obs_offset or args.obs_dropout)
    if noisy and args.policy == "random":
        ap.error("--obs-noise / --obs-offset / --obs-dropout need --policy actor or student")
    if args.occlusion and args.policy == "random":
        ap.error("--occlusion needs --policy actor or student")
    if args.rollouts < 0 or (args.rollouts and args.policy != "actor"):
        ap.error("--rollouts N needs N >= 0 and --policy actor")

    scene = assets.load_reference_assets(args.assets) if args.assets else assets.example_scene(args.scene, args.scene_seed)
    cfg = config.SimConfig(num_envs=args.envs, device="cuda:0")
    env = vec_env.VecEnv(headless=True, sim=args.sim, suspension=args.suspension, drive=args.drive, wheel_radius=args.wheel_radius,
                         steer_rate=args.steer_rate, wheel_accel=args.wheel_accel)
    extent = scene.terrain.map_indices.shape[0] * scene.terrain.cell_size
    g = torch.Generator().manual_seed(0)
    spawn = torch.zeros(args.envs, 3)
    spawn[:, 0:2] = 0.15 * extent + 0.7 * extent * torch.rand(args.envs, 2, generator=g)
    from isaac_rover_amd.tasks.rover import RoverTask
    task = RoverTask("Rover", cfg, env, scene=scene, distribution=None if args.native_rays else synth.ray_distribution("37"))
    env.set_task(task, sim_params={"dt": 0.05}, spawn_positions=spawn)          # utils/task_util.py:45
    obs = env.reset()
    print(f"obs {tuple(obs.shape)}  actions {task.num_actions}  device {task.device}")
    tracker = None
    if args.track_interval:
        from isaac_rover_amd.learning.tracking import EpisodeTracker
        tracker = EpisodeTracker.for_task(task, window=args.track_window)
    agent = None
    if args.policy == "actor":
        from isaac_rover_amd.learning.model import StochasticActorHeightmap
        agent = StochasticActorHeightmap(task._engine, task, precision=args.precision)
        if args.checkpoint:
            sd = torch.load(args.checkpoint, map_location="cpu")
            agent.load_state_dict(sd.get("policy", sd) if isinstance(sd, dict) else sd)
        print(f"policy: StochasticActorHeightmap, {sum(v.numel() for v in agent.state_dict().values()):,} parameters"
              f"{' from ' + args.checkpoint if args.checkpoint else ' (fresh initialisation)'}"
              f"{', acting in bf16' if args.precision == 'bf16' else ''}")
    student = None
    if args.policy == "student":
        from isaac_rover_amd.learning.student import StudentPolicy
        student = StudentPolicy(task._engine, task, device=task.device, precision=args.precision)
        if args.checkpoint:
            sd = torch.load(args.checkpoint, map_location="cpu")
            student.load_state_dict(sd["state_dict"] if isinstance(sd, dict) and "state_dict" in sd else sd)
        student.init_hidden(args.envs)
        print(f"policy: StudentPolicy, {sum(v.numel() for v in student.state_dict().values()):,} parameters"
              f"{' from ' + args.checkpoint if args.checkpoint else ' (fresh initialisation)'}"
              f"{', acting in bf16' if args.precision == 'bf16' else ''}")
    noise = None
    if noisy:
        from isaac_rover_amd.learning.noise import HeightmapNoise
        noise = HeightmapNoise(task._engine, task, sigma_point=args.obs_noise, sigma_offset=args.obs_offset, dropout=args.obs_dropout, seed=3)
        print(f"perception: rover_obs_noise, sigma_point {args.obs_noise} sigma_offset {args.obs_offset} dropout {args.obs_dropout}")
    occlusion = hidden = None
    if args.occlusion:
        from isaac_rover_amd.learning.noise import HeightmapOcclusion
        occlusion = HeightmapOcclusion(task._engine, task, camera=args.camera, step=args.sight_step, clearance=args.sight_clearance)
        hidden = torch.zeros(args.envs, occlusion.columns, dtype=torch.uint8, device=task.device)
        print(f"perception: rover_obs_occlusion, camera {tuple(args.camera)} step {args.sight_step} clearance {args.sight_clearance}")
    critic = memory = done = None
    if args.rollouts:
        from isaac_rover_amd.learning.model import DeterministicHeightmap
        from isaac_rover_amd.learning.rollout import RolloutMemory, compute_gae
        critic = DeterministicHeightmap(task._engine, task, seed=1, precision=args.precision)
        memory = RolloutMemory(args.rollouts, args.envs, device=task.device, report=print)
        for name, size, dtype in (("states", obs.shape[1], torch.float32), ("actions", task.num_actions, torch.float32), ("log_prob", 1, torch.float32),
                                  ("values", 1, torch.float32), ("rewards", 1, torch.float32), ("terminated", 1, torch.bool),
                                  ("returns", 1, torch.float32), ("advantages", 1, torch.float32)):
            memory.create_tensor(name, size, dtype)
    ret = torch.zeros(args.envs, device=task.device)
    episodes = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(args.steps):
        seen = obs if noise is None else noise.apply(obs, reset=done)              # what the policy sees; the task keeps the clean obs
        if occlusion is not None:                                                  # the poses are still the ones obs was made from
            seen = occlusion.apply(obs, noisy=seen, out=None if seen is obs else seen, hidden=hidden)
        if student is not None:
            actions = student.act(seen, reset=None if done is None else done.bool())  # an env that just ended starts from a zero hidden state
        elif agent is None:
            actions = 2 * torch.rand(args.envs, 2, device=task.device) - 1
        else:
            actions, log_prob, outputs = agent.act(seen)                           # what a PPO rollout stores next to obs and rew
        if memory is not None:
            values, _, _ = critic.act(obs)
            states = obs.clone()                                                   # env.step() rewrites the observation buffer
        obs, rew, done, info = env.step(actions)
        if tracker is not None:
            tracker.step(rew, done, info)                                          # two launches, nothing read back
            if (step + 1) % args.track_interval == 0:
                print(f"step {step + 1}: {tracker.read().line()}")
        if memory is not None:
            memory.add_samples(states=states, actions=actions, log_prob=log_prob, values=values, rewards=rew, terminated=done.bool())
            if memory.memory_index == 0:                                           # full: returns and advantages of these N steps
                last_values, _, _ = critic.act(obs)
                returns, adv = compute_gae(task._engine, memory, last_values)
                print(f"rollout of {args.rollouts} steps: mean return {float(returns.mean()):.4f}, advantages mean {float(adv.mean()):+.2e} "
                      f"std {float(adv.std()):.4f}")
                memory.reset()
        ret += rew
        episodes += int(done.sum())                                             # host sync, like a logger would do
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{args.steps} steps x {args.envs} envs in {dt:.2f} s = {args.steps * args.envs / dt:,.0f} env-steps/s "
          f"(incl. {args.policy} policy + {'toy pose feeder' if args.sim == 'kinematic' else 'terrain-following motion model' + (', rocker-bogie posture' if args.suspension == 'bogie' else '') + (', wheel-level drive' if args.drive == 'wheels' else '')}); episodes finished: {episodes}; mean return {float(ret.mean()):.4f}")
    if hidden is not None:
        print(f"occlusion: {100.0 * float(hidden.float().mean()):.2f} % of the heightmap columns hidden at the last step")
    env.close()


if __name__ == "__main__":
    main()
