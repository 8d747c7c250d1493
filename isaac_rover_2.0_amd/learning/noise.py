"""The sensor model between the task's observation and a policy: noise on the heightmap columns, on the MI355X.

The reference's authors tried Gaussian noise, dropout, a constant offset and zeroed columns on the observation
(``omniisaacgymenvs/tasks/rover.py:326-329``, commented out) and carry ``is_evaluation_with_noise`` / ``max_noise_dev = 0.2``; their
evaluation runs are named ``..._no_noise_...``.  The student exists to act on such a degraded heightmap and to reconstruct the clean one
(``learning/distill.py``: ``target=clean``).  ``HeightmapNoise`` is that model as ONE ``rover_obs_noise`` launch (``include/rover_step.h``
holds the definition, ``csrc/rover_noise.hip`` the kernel): per column Gaussian noise ``sigma_point``, one Gaussian offset per env and
episode ``sigma_offset``, and dropout to ``drop_value``.  ``RoverTask`` and its rewards keep the clean observation; only what is fed to a
policy (or written into a training window) goes through ``apply``.

The noise is counter-based (Philox4x32-10 keyed by ``seed``; the streams of the goal draws and of the action noise are disjoint from it
under one seed): a value depends on (seed, call counter, global env, column) and on the env's episode count, not on the batch shape — a
shard that passes its ``env_offset`` reproduces its slice of the whole —, and no second window-sized tensor of random numbers exists.
The two counters are device tensors at fixed addresses, advanced by torch ops enqueued after the launch: after one warm-up call,
``apply`` can be captured in a graph, and eager calls and replays continue one stream of draws.

``HeightmapOcclusion`` is the scene-dependent stage behind it, ONE ``rover_obs_occlusion`` launch (``csrc/rover_occlusion.hip``): a column
whose measured point a camera on the mast cannot see — the ground rises above the sight line — reads ``drop_value``.  It is stateless.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch

from .student import _info_of

PARAMS = ("sigma_point", "sigma_offset", "dropout", "drop_value", "seed", "env_offset")


class HeightmapNoise:
    def __init__(self, engine, task_or_info, sigma_point=0.0, sigma_offset=0.0, dropout=0.0, drop_value=0.0, seed=0, row_scale=None,
                 env_offset=0, device=None):
        """``task_or_info``: what ``StudentPolicy`` takes (a RoverTask, or a mapping with proprioceptive / sparse / dense / actions): the
        last ``sparse + dense`` columns of a row are the heightmap.  ``row_scale``: optional [E] float32 tensor multiplying both sigmas of
        its env (``noise_sweep``).  ``env_offset``: the global index of env 0 (a shard's).  ``engine`` may be None for a ``device`` that is
        not a GPU: the object then only carries its parameters and counters (``state_dict``), ``apply`` raises."""
        self.engine = engine
        self.info = _info_of(task_or_info)
        for name, v in (("sigma_point", sigma_point), ("sigma_offset", sigma_offset), ("drop_value", drop_value)):
            if not math.isfinite(float(v)) or (name != "drop_value" and float(v) < 0.0):
                raise ValueError(f"HeightmapNoise: {name} = {v} must be finite{'' if name == 'drop_value' else ' and >= 0'}")
        if not 0.0 <= float(dropout) <= 1.0:                                # also refuses a NaN
            raise ValueError(f"HeightmapNoise: dropout = {dropout} outside [0, 1]")
        if int(env_offset) < 0:
            raise ValueError(f"HeightmapNoise: env_offset = {env_offset} is negative")
        self.sigma_point, self.sigma_offset, self.dropout, self.drop_value = float(sigma_point), float(sigma_offset), float(dropout), float(drop_value)
        self.seed, self.env_offset = int(seed) & (2 ** 64 - 1), int(env_offset)
        if row_scale is not None and (not isinstance(row_scale, torch.Tensor) or row_scale.dim() != 1 or row_scale.dtype != torch.float32):
            raise ValueError("HeightmapNoise: row_scale must be a float32 tensor [E]")
        if device is None:
            device = engine.device if engine is not None else (row_scale.device if row_scale is not None else "cpu")
        self.device = torch.device(device)
        if row_scale is not None:
            row_scale = row_scale.to(self.device).contiguous()
        self.row_scale = row_scale
        self.counter = torch.zeros(1, dtype=torch.int64, device=self.device)       # calls of apply() so far: the kernels' t
        self.episode = None                                                         # [E] int64, made by the first apply (or load_state_dict)

    @property
    def columns(self):
        """How many trailing columns of a row ``apply`` perturbs: sparse + dense."""
        return self.info["sparse"] + self.info["dense"]

    @staticmethod
    def noise_sweep(max_dev, num_envs, device="cpu"):
        """The reference's ``max_noise_dev`` idea: one evaluation run covers every noise level.  -> ``row_scale = linspace(0, 1, E)``
        (float32, on ``device``), to be used with ``sigma_* = max_dev``: env i is then perturbed with the deviation max_dev * i / (E - 1)."""
        if not math.isfinite(float(max_dev)) or float(max_dev) < 0.0 or int(num_envs) < 1:
            raise ValueError(f"HeightmapNoise.noise_sweep: max_dev = {max_dev} must be finite and >= 0, num_envs = {num_envs} >= 1")
        return torch.linspace(0.0, 1.0, int(num_envs), dtype=torch.float32, device=device)

    def _episodes(self, e):
        if self.episode is None:
            self.episode = torch.zeros(e, dtype=torch.int64, device=self.device)
        if self.episode.shape[0] != e:
            raise ValueError(f"HeightmapNoise: {e} envs, the episode counter holds {self.episode.shape[0]}")
        if self.row_scale is not None and self.row_scale.shape[0] != e:
            raise ValueError(f"HeightmapNoise: {e} envs, row_scale holds {self.row_scale.shape[0]}")
        return self.episode

    def apply(self, obs, out=None, reset=None):
        """obs [E, F] -> out [E, F] (a new tensor when None; ``out`` may be ``obs`` itself, or a row view such as ``x[:, t]`` of a
        [B, T, F] window): the heightmap columns perturbed, the others copied.  ``reset``: optional [E] bool / integer device tensor (the
        step's done): AFTER this call's launch the marked envs' episode counts go up by one, so their next observation is the first
        with a new offset.  The call counter goes up by one.  Both updates are torch ops on the current stream."""
        if self.engine is None:
            raise RuntimeError("HeightmapNoise.apply needs an Engine (this object was made without one)")
        e, f = obs.shape
        ex = self.columns
        if f < ex:
            raise ValueError(f"HeightmapNoise: obs has {f} columns, the heightmap alone has sparse + dense = {ex}")
        out = self.engine.obs_noise(obs, out, first=f - ex, sigma_point=self.sigma_point, sigma_offset=self.sigma_offset, dropout=self.dropout,
                                    drop_value=self.drop_value, row_scale=self.row_scale, episode=self._episodes(e), seed=self.seed,
                                    step_dev=self.counter, row_offset=self.env_offset)
        self.counter += 1
        if reset is not None:
            self.episode += reset != 0
        return out

    # ---- resuming a run continues the same streams -------------------------------------------------------------
    def state_dict(self):
        sd = OrderedDict((k, getattr(self, k)) for k in PARAMS)
        sd["counter"] = self.counter.detach().clone()
        sd["episode"] = None if self.episode is None else self.episode.detach().clone()
        sd["row_scale"] = None if self.row_scale is None else self.row_scale.detach().clone()
        return sd

    def load_state_dict(self, sd):
        """Parameters and both counters from ``sd``; the counters keep their addresses where the shapes allow (a captured graph stays
        valid).  A missing key is a KeyError naming it."""
        for k in PARAMS + ("counter", "episode", "row_scale"):
            if k not in sd:
                raise KeyError(f"HeightmapNoise.load_state_dict: missing key '{k}'")
        for k in PARAMS:
            setattr(self, k, type(getattr(self, k))(sd[k]))
        self.counter.copy_(torch.as_tensor(sd["counter"]).reshape(1))
        for name in ("episode", "row_scale"):
            v, cur = sd[name], getattr(self, name)
            if v is None:
                setattr(self, name, None)
            elif cur is not None and cur.shape == v.shape:
                cur.copy_(v)
            else:
                setattr(self, name, torch.as_tensor(v).to(self.device).clone())


OCCLUSION_PARAMS = ("camera", "step", "clearance", "max_steps", "miss", "drop_value")


class HeightmapOcclusion:
    def __init__(self, engine, task_or_info, camera=(0.0, 0.0, 0.7), step=0.05, clearance=0.03, max_steps=256, miss=5.0, drop_value=0.0):
        """The line-of-sight stage: a heightmap column whose measured point a camera at ``camera`` (body frame: forward, left, up, in
        metres) cannot see reads ``drop_value``.  ``step``: spacing of the samples along a sight line; ``clearance``: by how much the
        ground must rise above the line to hide; ``max_steps``: the most intervals per line; ``miss``: |clean| at or beyond it is the
        clipped sentinel and stays as it is.  ``task_or_info`` as for ``HeightmapNoise``.  With an engine the constructor calls
        ``configure()``: the engine must hold its distribution and heightfield (a RoverTask's does).  ``engine`` None: a parameter
        carrier whose ``apply`` raises.  The object is stateless: no counters, ``state_dict`` holds the parameters only."""
        self.engine = engine
        self.task = None if hasattr(task_or_info, "keys") else task_or_info
        self.info = _info_of(task_or_info)
        cam = tuple(float(v) for v in camera)
        if len(cam) != 3:
            raise ValueError(f"HeightmapOcclusion: camera = {camera} must have three components (forward, left, up)")
        for name, v in (("camera", cam[0]), ("camera", cam[1]), ("camera", cam[2]), ("step", step), ("clearance", clearance), ("miss", miss),
                        ("drop_value", drop_value)):
            if not math.isfinite(float(v)):
                raise ValueError(f"HeightmapOcclusion: {name} = {v} must be finite")
        if not float(step) > 0.0:
            raise ValueError(f"HeightmapOcclusion: step = {step} must be > 0")
        if not float(miss) > 0.0:
            raise ValueError(f"HeightmapOcclusion: miss = {miss} must be > 0")
        if int(max_steps) != max_steps or not 2 <= int(max_steps) <= 4096:
            raise ValueError(f"HeightmapOcclusion: max_steps = {max_steps} outside 2 .. 4096")
        self.camera, self.step, self.clearance, self.max_steps = cam, float(step), float(clearance), int(max_steps)
        self.miss, self.drop_value = float(miss), float(drop_value)
        if engine is not None:
            self.configure()

    columns = HeightmapNoise.columns

    def configure(self):
        """rover_set_occlusion with this object's parameters: to be called again after the engine's distribution or heightfield was set
        again (``apply`` then raises with a message that says so)."""
        if self.engine is None:
            raise RuntimeError("HeightmapOcclusion.configure needs an Engine (this object was made without one)")
        self.engine.configure_occlusion(self.camera, self.step, self.clearance, self.max_steps, self.miss)

    def apply(self, obs, noisy=None, out=None, pos=None, quat=None, hidden=None):
        """obs [E, F], the task's CLEAN observation -> out [E, F]: ``noisy`` (None: ``obs``; usually ``HeightmapNoise.apply(obs)``) with
        the hidden heightmap columns at ``drop_value``.  ``out`` None: a new tensor; it may be ``noisy`` itself, or a row view such as
        ``x[:, t]`` of a [B, T, F] window, but never ``obs``.  ``pos`` [E, 3] / ``quat`` [E, 4]: the poses the observation was made
        from; they default to the task's ``_rover.get_world_poses()``, which are those until the next sim step.  ``hidden``: optional
        uint8 [E, sparse + dense] receiving the mask."""
        if self.engine is None:
            raise RuntimeError("HeightmapOcclusion.apply needs an Engine (this object was made without one)")
        e, f = obs.shape
        ex = self.columns
        if f < ex:
            raise ValueError(f"HeightmapOcclusion: obs has {f} columns, the heightmap alone has sparse + dense = {ex}")
        if pos is None or quat is None:
            if self.task is None:
                raise ValueError("HeightmapOcclusion.apply: pos and quat must be given (this object was made from an info mapping, not a task)")
            tp, tq = self.task._rover.get_world_poses()
            pos, quat = tp if pos is None else pos, tq if quat is None else quat
        return self.engine.obs_occlusion(obs, noisy, out, first=f - ex, pos=pos, quat=quat, drop_value=self.drop_value, hidden=hidden)

    def state_dict(self):
        return OrderedDict((k, getattr(self, k)) for k in OCCLUSION_PARAMS)

    def load_state_dict(self, sd):
        """The parameters from ``sd`` (a missing key is a KeyError naming it); with an engine, ``configure()`` again."""
        for k in OCCLUSION_PARAMS:
            if k not in sd:
                raise KeyError(f"HeightmapOcclusion.load_state_dict: missing key '{k}'")
        for k in OCCLUSION_PARAMS:
            setattr(self, k, tuple(float(v) for v in sd[k]) if k == "camera" else type(getattr(self, k))(sd[k]))
        if self.engine is not None:
            self.configure()
