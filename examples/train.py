#!/usr/bin/env python3
"""train.py-shaped PPO training on the MI355X rover step path (no Isaac Sim, no skrl, no autograd).

`examples/rollout.py`'s loop (`--policy actor --rollouts N`) with the weight update behind it: every `--rollouts` steps
`learning.ppo.PPO.update` runs compute_gae and `learning_epochs` x `mini_batches` minibatches of forward, PPO loss, backward
(`rover_ppo_loss`, `rover_linear_backward`), gradient clipping and one Adam step, with the reference's hyper-parameters
(cfg/trainSKRL/RoverPPOSKRL.yaml).  Prints losses, KL and the mean return per update.

    python examples/train.py --envs 512 --native-rays --steps 120 --rollouts 60 [--time-update]

`--state-preprocessor` / `--value-preprocessor` put skrl's RunningStandardScaler (`learning/preprocess.py`, `rover_scaler_update` /
`rover_scaler_apply`) where skrl's PPO puts it: the nets read the normalised observation, the memory stores the denormalised value, the
update trains both scalers.  `--lr-scheduler kl` steps skrl's KLAdaptiveRL once per epoch.  `--save PATH` writes `{policy, value,
state_preprocessor, value_preprocessor}` after the last step (the scalers' entries under skrl's three keys), `--load PATH` resumes from it.
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
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--assets", default="", help="directory holding the reference's tasks/utils/terrain/... files")
    ap.add_argument("--native-rays", action="store_true", help="the reference's 1634-point distribution (1750-float obs)")
    ap.add_argument("--checkpoint", default="", help="a state_dict of the reference's StochasticActorHeightmap (torch.save)")
    ap.add_argument("--rollouts", type=int, default=60, help="steps per rollout = rows of the memory (cfg/trainSKRL/RoverPPOSKRL.yaml:12)")
    ap.add_argument("--epochs", type=int, default=4, help="learning_epochs")
    ap.add_argument("--mini-batches", type=int, default=60, help="mini_batches")
    ap.add_argument("--kl-threshold", type=float, default=0.008)
    ap.add_argument("--native-step", action="store_true", help="gradient-norm clip + Adam as two HIP launches (learning/optim.py) instead of torch's")
    ap.add_argument("--kl-stop", choices=("host", "device"), default="host",
                    help="where the KL early stop is decided: host = one read per minibatch; device = by the native step's gate (needs --native-step)")
    ap.add_argument("--rollout-precision", choices=("f32", "bf16"), default="f32",
                    help="what the actor and the critic ACT in while the rollout is collected; the update stays f32 (learning/ppo.py)")
    ap.add_argument("--state-preprocessor", action="store_true", help="a RunningStandardScaler on the observation (learning/preprocess.py)")
    ap.add_argument("--value-preprocessor", action="store_true", help="a RunningStandardScaler on values and returns")
    ap.add_argument("--lr-scheduler", choices=("none", "kl"), default="none", help="kl = skrl's KLAdaptiveRL, one step per epoch (not with --kl-stop device)")
    ap.add_argument("--save", default="", help="after the last step, torch.save {policy, value, state_preprocessor, value_preprocessor} here")
    ap.add_argument("--load", default="", help="resume from a file --save wrote (a skrl agent checkpoint's preprocessor entries load as well)")
    ap.add_argument("--time-update", action="store_true", help="print the wall time of each update between two torch.cuda.synchronize()")
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
    if args.rollouts < 1:
        ap.error("--rollouts N needs N >= 1")

    scene = assets.load_reference_assets(args.assets) if args.assets else assets.example_scene(args.scene, args.scene_seed)
    cfg = config.SimConfig(num_envs=args.envs, device="cuda:0")
    env = vec_env.VecEnv(headless=True, sim=args.sim, suspension=args.suspension, drive=args.drive, wheel_radius=args.wheel_radius,
                         steer_rate=args.steer_rate, wheel_accel=args.wheel_accel)
    extent = scene.terrain.map_indices.shape[0] * scene.terrain.cell_size
    g = torch.Generator().manual_seed(0)
    spawn = torch.zeros(args.envs, 3)
    spawn[:, 0:2] = 0.15 * extent + 0.7 * extent * torch.rand(args.envs, 2, generator=g)
    from isaac_rover_amd.learning.model import DeterministicHeightmap, StochasticActorHeightmap
    from isaac_rover_amd.learning.ppo import PPO
    from isaac_rover_amd.learning.rollout import RolloutMemory
    from isaac_rover_amd.tasks.rover import RoverTask
    task = RoverTask("Rover", cfg, env, scene=scene, distribution=None if args.native_rays else synth.ray_distribution("37"))
    env.set_task(task, sim_params={"dt": 0.05}, spawn_positions=spawn)          # utils/task_util.py:45
    obs = env.reset()
    print(f"obs {tuple(obs.shape)}  actions {task.num_actions}  device {task.device}")
    tracker = None
    if args.track_interval:
        from isaac_rover_amd.learning.tracking import EpisodeTracker
        tracker = EpisodeTracker.for_task(task, window=args.track_window)
    agent = StochasticActorHeightmap(task._engine, task, precision=args.rollout_precision)
    if args.checkpoint:
        sd = torch.load(args.checkpoint, map_location="cpu")
        agent.load_state_dict(sd.get("policy", sd) if isinstance(sd, dict) else sd)
    critic = DeterministicHeightmap(task._engine, task, seed=1, precision=args.rollout_precision)
    memory = RolloutMemory(args.rollouts, args.envs, device=task.device, report=print)
    for name, size, dtype in (("states", obs.shape[1], torch.float32), ("actions", task.num_actions, torch.float32), ("log_prob", 1, torch.float32),
                              ("values", 1, torch.float32), ("rewards", 1, torch.float32), ("terminated", 1, torch.bool),
                              ("returns", 1, torch.float32), ("advantages", 1, torch.float32)):
        memory.create_tensor(name, size, dtype)
    extra = {}
    if args.state_preprocessor or args.value_preprocessor or args.lr_scheduler == "kl":
        from isaac_rover_amd.learning.ppo import KLAdaptiveRL
        from isaac_rover_amd.learning.preprocess import RunningStandardScaler
        if args.state_preprocessor:
            extra["state_preprocessor"] = RunningStandardScaler(task._engine, obs.shape[1])
        if args.value_preprocessor:
            extra["value_preprocessor"] = RunningStandardScaler(task._engine, 1)
        if args.lr_scheduler == "kl":
            extra["lr_scheduler"] = KLAdaptiveRL()
        print("preprocessors: " + ", ".join(k for k in ("state_preprocessor", "value_preprocessor") if k in extra)
              + ("  lr scheduler: KLAdaptiveRL" if "lr_scheduler" in extra else ""))
    ppo = PPO(task._engine, agent, critic, memory, {"learning_epochs": args.epochs, "mini_batches": args.mini_batches, "kl_threshold": args.kl_threshold},
              generator=torch.Generator().manual_seed(0), native_step=args.native_step, kl_stop=args.kl_stop, **extra)
    if args.load:
        ck = torch.load(args.load, map_location="cpu")
        agent.load_state_dict(ck["policy"])
        critic.load_state_dict(ck["value"])
        for name in ("state_preprocessor", "value_preprocessor"):
            if name in extra and ck.get(name) is not None:
                extra[name].load_state_dict(ck[name])
        print(f"resumed from {args.load}: " + ", ".join(k for k in ("policy", "value", "state_preprocessor", "value_preprocessor") if ck.get(k) is not None))
    normalized = torch.empty_like(obs) if args.state_preprocessor else None
    updates = 0
    for step in range(args.steps):
        seen = obs if normalized is None else ppo.preprocess_states(obs, out=normalized)      # what the nets read
        actions, log_prob, _ = agent.act(seen)
        values, _, _ = critic.act(seen)
        if args.value_preprocessor:
            values = ppo.denormalize_values(values)
        states = obs.clone()                                                       # env.step() rewrites the observation buffer
        obs, rew, done, info = env.step(actions)
        if tracker is not None:
            tracker.step(rew, done, info)                                          # two launches, nothing read back
            if (step + 1) % args.track_interval == 0:
                print(f"step {step + 1}: {tracker.read().line()}")
        memory.add_samples(states=states, actions=actions, log_prob=log_prob, values=values, rewards=rew, terminated=done.bool())
        if memory.memory_index == 0:                                               # full: one PPO update on these N steps
            last_values, _, _ = critic.act(obs if normalized is None else ppo.preprocess_states(obs, out=normalized))
            last_values = ppo.denormalize_values(last_values) if args.value_preprocessor else last_values.clone()      # the update's forwards reuse the critic's buffers
            if args.time_update:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            out = ppo.update(last_values)
            if args.time_update:
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            updates += 1
            steps = sum(ppo.minibatches_done)
            print(f"update {updates}: policy_loss {float(out['policy_loss']):+.5f}  value_loss {float(out['value_loss']):.5f}  "
                  f"entropy_loss {float(out['entropy_loss']):+.5f}  kl {float(out['kl']):.3e}  mean return "
                  f"{float(memory.get_tensor_by_name('returns').mean()):.4f}  minibatches stepped per epoch {ppo.minibatches_done}"
                  + (f"  update {dt * 1e3:.1f} ms ({dt * 1e3 / max(steps, 1):.2f} ms per stepped minibatch of "
                     f"{args.rollouts * args.envs // args.mini_batches} rows)" if args.time_update else "")
                  + (f"  lr {ppo.learning_rates[-1]:.3e}" if ppo.learning_rates else ""))
            memory.reset()
    if args.save:
        torch.save({"policy": {k: v.detach().cpu() for k, v in agent.state_dict().items()}, "value": {k: v.detach().cpu() for k, v in critic.state_dict().items()},
                    "state_preprocessor": {k: v.cpu() for k, v in extra["state_preprocessor"].state_dict().items()} if "state_preprocessor" in extra else None,
                    "value_preprocessor": {k: v.cpu() for k, v in extra["value_preprocessor"].state_dict().items()} if "value_preprocessor" in extra else None},
                   args.save)
        print(f"saved policy, value and preprocessors to {args.save}")
    env.close()


if __name__ == "__main__":
    main()
