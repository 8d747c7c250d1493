"""Episode statistics kept on the MI355X: what tells whether training works.

The reference judges a run by the nine scalars skrl's agent writes every ``write_interval`` steps (``omniisaacgymenvs/train.py:107``; its
sweep maximises ``Reward / Total reward (mean)``, ``train.py:133``): the instantaneous reward, and the total reward and the length of the
episodes in a deque of the last 100 finished ones, each as max / min / mean.  skrl keeps them with a ``nonzero()`` and a host read of its
size every step, six ``.item()`` reads and ``tolist()`` round trips for the finished envs.  ``EpisodeTracker`` keeps the same figures —
and the exact totals of the interval and the means of the reward components the step writes into ``extras`` — with ONE
``rover_episode_track`` call per env step (``include/rover_step.h`` holds the definition, ``csrc/rover_track.hip`` the two kernels):
enqueue only, deterministic, capturable in a graph, read back once per reporting interval.

All state lives in tensors this object owns: the per-env cumulative reward and step count, the ring of the last ``window`` finished
episodes, the interval record and the kernels' scratch.  ``step`` takes the task's own buffers (``rew_buf``, the int64 ``reset_buf``, the
``extras`` dict) without a conversion op.  The window is per tracker: a shard of a multi-GPU run has its own; ``combine`` merges
everything else.
"""
from __future__ import annotations

import math

import torch

from .. import _lib

SKRL_TAGS = tuple(f"{head} ({stat})" for head in ("Reward / Instantaneous reward", "Reward / Total reward", "Episode / Total timesteps")
                  for stat in ("max", "min", "mean"))

_SCALARS = tuple(name for name, _ in _lib.TrackRecord._fields_ if name != "comp_sum")
_ADD = ("inst_sum", "inst_count", "ep_count", "ep_ret_sum", "ep_ret_sumsq", "ep_len_sum")
_MIN = ("inst_min", "ep_ret_min", "ep_len_min")
_MAX = ("inst_max", "ep_ret_max", "ep_len_max")


class TrackReadout(dict):
    """What ``EpisodeTracker.read`` returns: the tags as a dict (``str(r)`` is the one-line print), with the record's own fields in
    ``raw`` (plus ``num_envs``, ``inst_count`` = calls x envs, ``components`` and, if asked for, ``ring_ret`` / ``ring_len``)."""
    raw: dict

    def line(self):
        return "  ".join(f"{k} {v:.6g}" if isinstance(v, float) else f"{k} {v}" for k, v in self.items())


def tags_of(raw, window=True):
    """The read-out dict of a raw record.  A tag with nothing to report is absent."""
    out = TrackReadout()
    out.raw = raw
    if raw["inst_count"] > 0:
        out["Reward / Instantaneous reward (max)"] = raw["inst_max"]
        out["Reward / Instantaneous reward (min)"] = raw["inst_min"]
        out["Reward / Instantaneous reward (mean)"] = raw["inst_sum"] / raw["inst_count"]
    if window and raw.get("win_calls", 0) > 0:
        out["Reward / Total reward (max)"] = raw["win_ret_max"]
        out["Reward / Total reward (min)"] = raw["win_ret_min"]
        out["Reward / Total reward (mean)"] = raw["win_ret_mean_sum"] / raw["win_calls"]
        out["Episode / Total timesteps (max)"] = raw["win_len_max"]
        out["Episode / Total timesteps (min)"] = raw["win_len_min"]
        out["Episode / Total timesteps (mean)"] = raw["win_len_mean_sum"] / raw["win_calls"]
    out["Episodes / finished"] = raw["ep_count"]
    if raw["ep_count"] > 0:
        n = raw["ep_count"]
        mean = raw["ep_ret_sum"] / n
        out["Episodes / return (mean)"] = mean
        out["Episodes / return (std)"] = math.sqrt(max(raw["ep_ret_sumsq"] / n - mean * mean, 0.0))      # of the population
        out["Episodes / return (min)"] = raw["ep_ret_min"]
        out["Episodes / return (max)"] = raw["ep_ret_max"]
        out["Episodes / length (mean)"] = raw["ep_len_sum"] / n
        out["Episodes / length (min)"] = raw["ep_len_min"]
        out["Episodes / length (max)"] = raw["ep_len_max"]
    if raw["inst_count"] > 0:
        for name, s in zip(raw["components"], raw["comp_sum"]):
            out[f"Info / {name} (mean)"] = s / raw["inst_count"]
    return out


class EpisodeTracker:
    def __init__(self, engine, num_envs, window=100, components=(), device=None):
        """``components``: the keys of ``extras`` to follow, at most 16 (``_lib.EXTRAS`` names the eight a ``RoverTask`` writes; see
        ``for_task``).  ``window``: skrl's deque length, 1 .. 1024."""
        self.engine = engine
        self.num_envs, self.window, self.components = int(num_envs), int(window), tuple(components)
        if self.num_envs < 0 or not 1 <= self.window <= _lib.TRACK_MAX_WINDOW or len(self.components) > _lib.TRACK_MAX_COMPONENTS:
            raise ValueError(f"EpisodeTracker: num_envs = {num_envs} must be >= 0, window = {window} in 1 .. {_lib.TRACK_MAX_WINDOW}, and at most "
                             f"{_lib.TRACK_MAX_COMPONENTS} components (got {len(self.components)})")
        self.device = torch.device(device if device is not None else engine.device)
        e, w, dev = self.num_envs, self.window, self.device
        self.sizes = _lib.track_sizes(e, w, len(self.components))
        self.cum_reward = torch.zeros(e, dtype=torch.float32, device=dev)
        self.cum_steps = torch.zeros(e, dtype=torch.int32, device=dev)
        self.ring_ret = torch.zeros(w, dtype=torch.float32, device=dev)
        self.ring_len = torch.zeros(w, dtype=torch.int32, device=dev)
        self.ring_count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.scratch = torch.zeros(self.sizes["scratch_bytes"], dtype=torch.uint8, device=dev)
        fresh = torch.frombuffer(bytearray(bytes(_lib.track_fresh_record())), dtype=torch.uint8)
        self._fresh = fresh.to(dev)                                         # the constant reset() copies from, device to device
        self.record = self._fresh.clone()
        self._descs = {}                                                    # one checked descriptor per set of input buffers

    @classmethod
    def for_task(cls, task, window=100, components=None):
        """A tracker for a ``RoverTask``: its engine and env count, and by default all eight reward components of ``_lib.EXTRAS``."""
        return cls(task._engine, task.num_envs, window=window, components=_lib.EXTRAS if components is None else components, device=task.device)

    def step(self, rewards, done, extras=None):
        """One env step: ``rewards`` [E] float32, ``done`` [E] bool / uint8 / int64, ``extras`` the task's dict holding every key of
        ``components`` (float32 or int64 [E]).  One ``Engine.episode_track``; nothing is read back.  The descriptor is built and checked
        once per set of buffers (a task hands over the same ones every step)."""
        comps = tuple(extras[name] for name in self.components) if self.components else ()
        key = (rewards.data_ptr(), done.data_ptr(), rewards.shape, done.shape, done.dtype) + tuple((t.data_ptr(), t.dtype, t.shape) for t in comps)
        if len(self._descs) > 64:
            self._descs.clear()
        self._descs[key] = self.engine.episode_track(rewards, done, cum_reward=self.cum_reward, cum_steps=self.cum_steps, ring_ret=self.ring_ret,
                                                     ring_len=self.ring_len, ring_count=self.ring_count, record=self.record, scratch=self.scratch,
                                                     components=comps, desc=self._descs.get(key))

    def reset(self):
        """A fresh interval record; the per-env state and the ring go on."""
        self.record.copy_(self._fresh)

    def read(self, reset=True, ring=False):
        """The interval so far as a ``TrackReadout``: one device-to-host copy of the 240-byte record (and, with ``ring``, of the ring, as
        ``raw["ring_ret"]`` / ``raw["ring_len"]`` / ``raw["ring_count"]``, valid slots only), then ``reset()`` if asked."""
        rec = _lib.TrackRecord.from_buffer_copy(self.record.cpu().numpy().tobytes())
        raw = {name: getattr(rec, name) for name in _SCALARS}
        raw["comp_sum"] = [rec.comp_sum[k] for k in range(len(self.components))]
        raw["components"] = self.components
        raw["num_envs"] = self.num_envs
        raw["inst_count"] = rec.calls * self.num_envs
        if ring:
            count = int(self.ring_count.item())
            valid = min(count, self.window)
            raw["ring_count"] = count
            raw["ring_ret"] = self.ring_ret[:valid].cpu().numpy()
            raw["ring_len"] = self.ring_len[:valid].cpu().numpy()
        if reset:
            self.reset()
        return tags_of(raw)

    @staticmethod
    def combine(a, b):
        """Two shards' read-outs of the same interval as one: envs, counts and sums add, minima and maxima combine, the means and the
        standard deviation follow.  The window is per shard and is left out: the result has no ``Reward / Total reward`` and no
        ``Episode / Total timesteps`` tags."""
        ra, rb = a.raw, b.raw
        if ra["calls"] != rb["calls"] or tuple(ra["components"]) != tuple(rb["components"]):
            raise ValueError("EpisodeTracker.combine: the two read-outs cover different calls or components")
        raw = {"calls": ra["calls"], "components": tuple(ra["components"]), "num_envs": ra["num_envs"] + rb["num_envs"]}
        for k in _ADD:
            raw[k] = ra[k] + rb[k]
        for k in _MIN:
            raw[k] = min(ra[k], rb[k])
        for k in _MAX:
            raw[k] = max(ra[k], rb[k])
        raw["comp_sum"] = [x + y for x, y in zip(ra["comp_sum"], rb["comp_sum"])]
        return tags_of(raw, window=False)
