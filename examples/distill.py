#!/usr/bin/env python3
"""Distilling a teacher into the recurrent student on the MI355X rover step path (no Isaac Sim, no autograd).

The teacher (`StochasticActorHeightmap`, fresh or from `--teacher`, acting with its mean) drives `RoverTask` on a synthetic scene.
Windows of `--window` steps of (observation, teacher action, done) are collected; after each window `learning.distill.StudentTrainer.update`
runs one step of back-propagation through time on the student (`rover_gru_cell_train`, `rover_gru_cell_backward`, `rover_linear_dgrad`, ...,
clip + Adam as `rover_optim_step`), with Gaussian noise on the student's heightmap columns and the clean ones as the reconstruction target.
The hidden state is carried from window to window (truncated BPTT); an env that ended starts its next step from a zero state.
Prints the three losses per update and saves the reference's `{"state_dict": ...}` layout, which `rollout.py --policy student --checkpoint`
loads.

    python examples/distill.py --envs 512 --window 32 --updates 20 [--teacher actor.pt] [--out student.pt]

`--device-noise`, `--obs-offset S` or `--obs-dropout P` switch the perception model to `learning.noise.HeightmapNoise`: every step's
observation is written into the window by one `rover_obs_noise` launch (Gaussian noise `--noise` per column, a Gaussian offset per env
and episode, dropout to 0), counter-based and independent of the batch shape; the window-sized `torch.randn` tensor is then never made.
`--occlusion [--camera F L U] [--sight-step S] [--sight-clearance C]` adds the line-of-sight stage behind it (`HeightmapOcclusion`, one
`rover_obs_occlusion` launch on the window row): columns a camera on the mast cannot see read 0; the target stays the clean row.
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from isaac_rover_amd import assets, config, synth, vec_env  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--window", type=int, default=32, help="time steps per update (the length back-propagation through time covers)")
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--native-rays", action="store_true", help="the reference's 1634-point distribution (1750-float obs)")
    ap.add_argument("--teacher", default="", help="a state_dict of the reference's StochasticActorHeightmap (torch.save)")
    ap.add_argument("--noise", type=float, default=0.05, help="standard deviation of the noise on the student's heightmap columns")
    ap.add_argument("--obs-offset", type=float, default=0.0, help="standard deviation of a per-env, per-episode offset on the heightmap columns")
    ap.add_argument("--obs-dropout", type=float, default=0.0, help="probability of a heightmap column reading 0")
    ap.add_argument("--device-noise", action="store_true", help="the noise as one rover_obs_noise launch per step instead of torch.randn "
                    "(implied by --obs-offset / --obs-dropout / --occlusion)")
    ap.add_argument("--occlusion", action="store_true",
                    help="after the noise, heightmap columns whose measured point a camera on the mast cannot see read 0 in the window "
                         "(rover_obs_occlusion); the reconstruction target stays the clean row")
    ap.add_argument("--camera", type=float, nargs=3, default=(0.0, 0.0, 0.7), metavar=("F", "L", "U"), help="--occlusion: the camera in the body frame, metres")
    ap.add_argument("--sight-step", type=float, default=0.05, help="--occlusion: spacing of the samples along a sight line, metres")
    ap.add_argument("--sight-clearance", type=float, default=0.03, help="--occlusion: how far the ground must rise above the sight line to hide, metres")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--grad-norm-clip", type=float, default=1.0)
    ap.add_argument("--recon-scale", type=float, default=0.5)
    ap.add_argument("--torch-step", action="store_true", help="clip_grad_norm_ + torch.optim.Adam instead of the two HIP launches")
    ap.add_argument("--teacher-precision", choices=("f32", "bf16"), default="f32", help="what the teacher acts in (the student trains in f32)")
    ap.add_argument("--out", default="", help="where to save {'state_dict': ...} (the reference's best.pt layout)")
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
                    help="every N env steps print the episode statistics kept on the device (learning/tracking.py:EpisodeTracker, one "
                         "rover_episode_track call per step, one read per N steps): skrl's nine Reward / Episode tags, the interval's exact "
                         "episode figures and the means of the eight reward components; 0 = off")
    ap.add_argument("--track-window", type=int, default=100, help="how many of the last finished episodes the Total reward / Total timesteps tags cover (skrl: 100)")
    ap.add_argument("--scene", choices=("synth", "mars"), default="synth",
                    help="synth = the synthetic sine-and-discs scene; mars = a 60 m yard from the reference's Mars terrain "
                         "generator (assets.build_mars_scene: hills and rocks from --scene-seed, both KNN maps and the heightfield on the GPU)")
    ap.add_argument("--scene-seed", type=int, default=10, help="--scene mars: the generator's seed (10 = the reference's own)")
    args = ap.parse_args()
    if args.suspension != "plane" and args.sim != "terrain":
        ap.error("--suspension bogie needs --sim terrain")
    if args.drive != "command" and args.sim != "terrain":
        ap.error("--drive wheels needs --sim terrain")
    if args.window < 1 or args.updates < 1:
        ap.error("--window and --updates need values >= 1")
    if args.track_interval < 0 or not 1 <= args.track_window <= 1024:
        ap.error("--track-interval N needs N >= 0, --track-window W needs W in 1 .. 1024")

    scene = assets.example_scene(args.scene, args.scene_seed)
    cfg = config.SimConfig(num_envs=args.envs, device="cuda:0")
    env = vec_env.VecEnv(headless=True, sim=args.sim, suspension=args.suspension, drive=args.drive, wheel_radius=args.wheel_radius,
                         steer_rate=args.steer_rate, wheel_accel=args.wheel_accel)
    extent = scene.terrain.map_indices.shape[0] * scene.terrain.cell_size
    g = torch.Generator().manual_seed(0)
    spawn = torch.zeros(args.envs, 3)
    spawn[:, 0:2] = 0.15 * extent + 0.7 * extent * torch.rand(args.envs, 2, generator=g)
    from isaac_rover_amd.learning.distill import StudentTrainer
    from isaac_rover_amd.learning.model import StochasticActorHeightmap
    from isaac_rover_amd.learning.student import StudentPolicy
    from isaac_rover_amd.tasks.rover import RoverTask
    task = RoverTask("Rover", cfg, env, scene=scene, distribution=None if args.native_rays else synth.ray_distribution("37"))
    env.set_task(task, sim_params={"dt": 0.05}, spawn_positions=spawn)
    obs = env.reset()
    teacher = StochasticActorHeightmap(task._engine, task, precision=args.teacher_precision)
    if args.teacher:
        sd = torch.load(args.teacher, map_location="cpu")
        teacher.load_state_dict(sd.get("policy", sd) if isinstance(sd, dict) else sd)
    student = StudentPolicy(task._engine, task, device=task.device, seed=1)
    trainer = StudentTrainer(task._engine, student, lr=args.lr, grad_norm_clip=args.grad_norm_clip, recon_scale=args.recon_scale,
                             native_step=not args.torch_step)
    e, t_len, f, ex = args.envs, args.window, obs.shape[1], student.info["sparse"] + student.info["dense"]
    print(f"obs {tuple(obs.shape)}  teacher {'from ' + args.teacher if args.teacher else '(fresh initialisation)'}  student "
          f"{sum(p.numel() for p in student.parameters()):,} trainable parameters in {len(student.parameters())} tensors")
    x = torch.empty(e, t_len, f, device=task.device)
    clean = torch.empty(e, t_len, ex, device=task.device)
    wanted = torch.empty(e, t_len, task.num_actions, device=task.device)
    reset = torch.zeros(e, t_len, dtype=torch.bool, device=task.device)
    noise = noise_gen = None
    if args.device_noise or args.obs_offset or args.obs_dropout or args.occlusion:
        from isaac_rover_amd.learning.noise import HeightmapNoise
        noise = HeightmapNoise(task._engine, task, sigma_point=args.noise, sigma_offset=args.obs_offset, dropout=args.obs_dropout, seed=2)
        print(f"perception: rover_obs_noise, sigma_point {args.noise} sigma_offset {args.obs_offset} dropout {args.obs_dropout}")
    else:
        noise_gen = torch.Generator(device=task.device).manual_seed(2)
    occlusion = None
    if args.occlusion:
        from isaac_rover_amd.learning.noise import HeightmapOcclusion
        occlusion = HeightmapOcclusion(task._engine, task, camera=args.camera, step=args.sight_step, clearance=args.sight_clearance)
        print(f"perception: rover_obs_occlusion, camera {tuple(args.camera)} step {args.sight_step} clearance {args.sight_clearance}")
    tracker = None
    if args.track_interval:
        from isaac_rover_amd.learning.tracking import EpisodeTracker
        tracker = EpisodeTracker.for_task(task, window=args.track_window)
    h, done = None, torch.zeros(e, dtype=torch.bool, device=task.device)
    for u in range(args.updates):
        for t in range(t_len):
            actions, _, _ = teacher.act(obs, deterministic=True)
            if noise is None:
                x[:, t] = obs
            else:
                noise.apply(obs, out=x[:, t], reset=done)                          # the noisy row straight into the window
                if occlusion is not None:                                          # ... and what the camera cannot see out of it, in place
                    occlusion.apply(obs, noisy=x[:, t], out=x[:, t])
            clean[:, t] = obs[:, f - ex:]
            wanted[:, t] = actions
            reset[:, t] = done                                                     # an env that just ended starts from a zero hidden state
            obs, rew, done, info = env.step(actions)
            if tracker is not None:
                tracker.step(rew, done, info)                                      # two launches, nothing read back
                if (u * t_len + t + 1) % args.track_interval == 0:
                    print(f"step {u * t_len + t + 1}: {tracker.read().line()}")
            done = done.bool().clone()
        if noise is None:
            x[:, :, f - ex:] += args.noise * torch.randn(e, t_len, ex, device=task.device, generator=noise_gen)
        loss, action_loss, recon_loss, h = trainer.update(x, wanted, h0=h, reset=reset, target=clean)
        print(f"update {u + 1}: loss {float(loss):.6f}  action_loss {float(action_loss):.6f}  recon_loss {float(recon_loss):.6f}")
    if args.out:
        torch.save({"state_dict": {k: v.cpu() for k, v in student.state_dict().items()}}, args.out)
        print(f"saved {args.out}")
    env.close()


if __name__ == "__main__":
    main()
