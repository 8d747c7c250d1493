"""Minimal VecEnv so ``train.py``-style loops run without Isaac ("What calls the path").

Mirrors the contract of omni.isaac.gym's ``VecEnvBase`` as the reference uses it (``utils/task_util.py:45``,
``train.py:58-59``): ``set_task(task, backend, sim_params, init_sim)``, ``reset()``, ``step(actions)`` →
``(obs, rew, dones, info)`` with ``task.pre_physics_step`` before and ``task.post_physics_step`` after the
physics sub-steps, observations clipped to ``clip_obs`` and actions to ``clip_actions``.
PhysX is replaced by ``KinematicSim``: a toy unicycle integrator that moves each rover along the commanded
(linear, angular) velocity and keeps it on the heightfield — a pose FEEDER, not a simulator.  ``VecEnv(sim="terrain")`` selects
``TerrainSim`` instead: the terrain-following motion model of ``rover_motion_step``, one HIP launch per control step,
which also tilts the body with the ground under its six wheels, obeys Ackermann's turn-on-the-spot rule and writes the joint state.
``VecEnv(sim="terrain", suspension="bogie")`` runs its rocker-bogie posture mode: all six wheels on the ground, the three
passive suspension joints in the joint state, where the uprightness penalty and the wheel rays read them.
``VecEnv(sim="terrain", drive="wheels")`` runs its wheel-level drive mode, with either suspension: the steering and
drive joints follow Ackermann's targets at a limited rate, and the body moves the way its six wheels roll.
"""
from __future__ import annotations

import math

import torch


class KinematicSim:
    def __init__(self, task, dt: float = 0.05, max_lin: float = 1.0, max_ang: float = 1.0, ride_height: float = 0.3):
        self.task, self.dt, self.max_lin, self.max_ang, self.ride_height = task, dt, max_lin, max_ang, ride_height
        self._playing = True

    def is_playing(self):
        return self._playing

    def step(self, render: bool = False):
        t = self.task
        pos, quat = t._rover.get_world_poses()
        lin = t.linear_velocity.get_state(0) * self.max_lin
        ang = t.angular_velocity.get_state(0) * self.max_ang
        yaw = 2.0 * torch.atan2(quat[:, 3], quat[:, 0])
        yaw = yaw + ang * self.dt
        pos[:, 0] += lin * torch.cos(yaw) * self.dt
        pos[:, 1] += lin * torch.sin(yaw) * self.dt
        pos[:, 2] = t.get_pos_height(t.heightmap, pos[:, 0:2], t.horizontal_scale, t.vertical_scale, t.shift[0:2]) + self.ride_height
        quat[:, 0] = torch.cos(yaw / 2)
        quat[:, 1] = 0.0
        quat[:, 2] = 0.0
        quat[:, 3] = torch.sin(yaw / 2)


class TerrainSim:
    """``KinematicSim``'s interface on the terrain-following motion model (``Engine.motion_step``): the rover poses are advanced in place
    on the task's engine and heightfield, and the joint state follows the joint targets (ideal actuators).  ``advance(n)`` folds ``n``
    sub-steps of length ``dt`` into one launch; ``step`` is ``advance(1)``.  ``suspension="bogie"`` solves the rocker-bogie posture
    (``iters`` chord iterations, joints clamped to +-``max_bogie`` rad) and writes the passive joints into columns 0-2 of the joint
    positions; ``"plane"``, the default, fits a plane and leaves them at the targets' 0.  ``drive="wheels"`` moves the body by the
    wheels instead of by the command: the steering angles and wheel speeds of the joint state follow their targets by at most
    ``steer_rate`` rad/s and ``wheel_accel`` rad/s^2 (``inf``: ideal actuators), and the body takes the rigid motion that fits the six
    wheels, rolling on ``wheel_radius`` m, best (0.2 is the length the reference's Ackermann divides by; 0.1, the asset's physical
    radius, halves every speed); ``last_slip`` then holds the wheel slip of the last sub-step in m/s.  ``"command"`` is the default."""

    def __init__(self, task, dt: float = 0.05, max_lin: float = 1.0, max_ang: float = 1.0, ride_height: float = 0.3,
                 suspension: str = "plane", iters: int = 4, max_bogie: float = 0.6, drive: str = "command", wheel_radius: float = 0.2,
                 steer_rate: float = math.inf, wheel_accel: float = math.inf):
        if suspension not in SUSPENSIONS:
            raise ValueError(f"suspension must be one of {SUSPENSIONS}, not {suspension!r}")
        if drive not in DRIVES:
            raise ValueError(f"drive must be one of {DRIVES}, not {drive!r}")
        self.task, self.dt, self.max_lin, self.max_ang, self.ride_height = task, dt, max_lin, max_ang, ride_height
        self.suspension, self.iters, self.max_bogie = suspension, iters, max_bogie
        self.drive, self.wheel_radius, self.steer_rate, self.wheel_accel = drive, wheel_radius, steer_rate, wheel_accel
        self.last_slip = None
        self._playing = True

    def is_playing(self):
        return self._playing

    def step(self, render: bool = False):
        self.advance(1)

    def advance(self, n: int = 1):
        t = self.task
        r = t._rover
        pos, quat = r.get_world_poses()
        kw = {}
        if self.drive == "wheels":
            if self.last_slip is None or self.last_slip.shape[0] != pos.shape[0]:
                self.last_slip = torch.zeros(pos.shape[0], dtype=torch.float32, device=pos.device)
            kw = dict(drive="wheels", wheel_radius=self.wheel_radius, steer_rate=self.steer_rate, wheel_accel=self.wheel_accel, slip=self.last_slip)
        t._engine.motion_step(pos, quat, t.linear_velocity.get_state(0), t.angular_velocity.get_state(0), dt=self.dt, substeps=n,
                              max_lin=self.max_lin, max_ang=self.max_ang, ride_height=self.ride_height,
                              joints=(r._joint_pos_targets, r._joint_vel_targets, r.get_joint_positions(), r.get_joint_velocities()),
                              suspension=self.suspension, iters=self.iters, max_bogie=self.max_bogie, **kw)


SUSPENSIONS = ("plane", "bogie")
DRIVES = ("command", "wheels")
SIMS = {"kinematic": KinematicSim, "terrain": TerrainSim}


class VecEnv:
    def __init__(self, headless: bool = True, sim_device: int = 0, sim: str = "kinematic", suspension: str = "plane", drive: str = "command",
                 wheel_radius: float = 0.2, steer_rate: float = math.inf, wheel_accel: float = math.inf):
        if sim not in SIMS:
            raise ValueError(f"sim must be one of {tuple(SIMS)}, not {sim!r}")
        if suspension not in SUSPENSIONS:
            raise ValueError(f"suspension must be one of {SUSPENSIONS}, not {suspension!r}")
        if suspension != "plane" and sim != "terrain":
            raise ValueError(f"suspension={suspension!r} needs sim='terrain': KinematicSim writes no joint state")
        if drive not in DRIVES:
            raise ValueError(f"drive must be one of {DRIVES}, not {drive!r}")
        if drive != "command" and sim != "terrain":
            raise ValueError(f"drive={drive!r} needs sim='terrain': KinematicSim drives no joints")
        self._sim, self._suspension = sim, suspension
        self._drive = {} if drive == "command" else dict(drive=drive, wheel_radius=wheel_radius, steer_rate=steer_rate, wheel_accel=wheel_accel)
        self._render = not headless
        self._task = None
        self._world = None

    def set_task(self, task, backend="torch", sim_params=None, init_sim=True, spawn_positions=None) -> None:
        self._task = task
        task._env = self
        kw = dict(self._drive, suspension=self._suspension) if self._sim == "terrain" else {}
        self._world = SIMS[self._sim](task, dt=(sim_params or {}).get("dt", 0.05), **kw)
        task.set_up_scene(spawn_positions=spawn_positions)
        task.post_reset()
        self.num_envs = task.num_envs
        self.observation_space = task.observation_space
        self.action_space = task.action_space

    def reset(self):
        self._task.reset()
        actions = torch.zeros((self.num_envs, self._task.num_actions), device=self._task.rl_device)
        obs, _, _, _ = self.step(actions)
        return obs

    def step(self, actions):
        task = self._task
        actions = torch.clamp(actions, -task.clip_actions, task.clip_actions).to(task.device)
        task.pre_physics_step(actions)
        advance = getattr(self._world, "advance", None)
        if advance is not None:
            advance(task.control_frequency_inv)
        else:
            for _ in range(task.control_frequency_inv):
                self._world.step(render=False)
        obs, rew, resets, extras = task.post_physics_step()
        obs = torch.clamp(obs, -task.clip_obs, task.clip_obs)
        return obs, rew, resets, extras

    def close(self):
        if self._task is not None:
            self._task.close()


def initialize_task(sim_config, env, scene, init_sim=True, **task_kw):
    """utils/task_util.py:30-47: build the task named in the config and bind it to the env."""
    from .tasks.rover import RoverTask
    task = RoverTask(name=sim_config.task_config.get("name", "Rover"), sim_config=sim_config, env=env, scene=scene, **task_kw)
    env.set_task(task=task, sim_params=sim_config.task_config.get("sim"), backend="torch", init_sim=init_sim)
    return task
