"""Rollout memory and one-pass GAE: the rollout side of PPO for the policy nets of ``learning/model.py``.

The reference trains through skrl: ``RandomMemory(memory_size=60, num_envs=...)`` (``omniisaacgymenvs/train.py:82``) and ``rollouts: 60,
mini_batches: 60, discount_factor: 0.99, lambda: 0.95`` (``cfg/trainSKRL/RoverPPOSKRL.yaml:12-16``); skrl's ``PPO._update`` starts with
``compute_gae``.  ``RolloutMemory`` is the subset of skrl's ``Memory`` that PPO uses, ``compute_gae`` runs the whole recursion, the moments
and the normalisation as ``Engine.gae`` (``rover_gae``: one or two launches) on the stored tensors in place.  The semantics are restated from
a reading of skrl 0.10 / 1.x (skrl is no dependency of this package) and written out in ``include/rover_step.h``; the weight update
that consumes ``returns`` and ``advantages`` is ``learning/ppo.py``.

Time-limit bootstrapping (skrl's ``rewards += discount_factor * values * truncated`` in ``record_transition``) is one elementwise line
before ``add_samples`` and no part of the kernel.
"""
from __future__ import annotations

import torch

from .. import _lib


class RolloutMemory:
    """Tensors of ``memory_size`` time steps x ``num_envs`` envs, stored ``[memory_size, num_envs, size]`` like skrl's ``Memory``."""

    def __init__(self, memory_size, num_envs=1, device="cuda:0", report=None):
        """``report``: a callable (e.g. ``print``) told, per tensor, how many bytes the memory holds — at 65 536 envs x 60 steps x 1 750
        floats the states alone are 27.5 GB, which fits an MI355X's HBM but should not come as a surprise."""
        if int(memory_size) < 1 or int(num_envs) < 0:
            raise ValueError("RolloutMemory: memory_size >= 1 and num_envs >= 0")
        self.memory_size, self.num_envs, self.device = int(memory_size), int(num_envs), torch.device(device)
        self.tensors = {}
        self.memory_index = 0
        self.filled = False
        self._report = report

    @staticmethod
    def bytes_for(memory_size, num_envs, sizes):
        """Bytes a memory holds for tensors ``{name: (size, dtype)}`` — before anything is allocated."""
        return sum(int(memory_size) * int(num_envs) * int(size) * torch.empty((), dtype=dtype).element_size() for size, dtype in sizes.values())

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.tensors.values())

    def __len__(self):
        """Stored time steps x envs (skrl: ``memory_size * num_envs`` once filled, else ``memory_index * num_envs``)."""
        return (self.memory_size if self.filled else self.memory_index) * self.num_envs

    def create_tensor(self, name, size, dtype=torch.float32):
        """A zeroed ``[memory_size, num_envs, size]`` tensor; a second call with the same size and dtype keeps the first tensor."""
        size = int(size)
        if size < 1:
            raise ValueError(f"create_tensor({name!r}): size must be >= 1")
        old = self.tensors.get(name)
        if old is not None:
            if old.shape[2] != size or old.dtype != dtype:
                raise ValueError(f"create_tensor({name!r}): exists as size {old.shape[2]} {old.dtype}, asked for size {size} {dtype}")
            return old
        t = self.tensors[name] = torch.zeros(self.memory_size, self.num_envs, size, dtype=dtype, device=self.device)
        if self._report is not None:
            self._report(f"RolloutMemory: {name} [{self.memory_size}, {self.num_envs}, {size}] {str(dtype).replace('torch.', '')}: "
                         f"{t.numel() * t.element_size():,} bytes ({self.nbytes:,} in all)")
        return t

    def get_tensor_by_name(self, name, keepdim=True):
        """The stored tensor itself (no copy): ``[memory_size, num_envs, size]``, or flattened ``[memory_size * num_envs, size]``."""
        t = self.tensors[name]
        return t if keepdim else t.view(-1, t.shape[2])

    def set_tensor_by_name(self, name, tensor):
        """Copies ``tensor`` (the stored shape, or ``[memory_size, num_envs]`` for a size-1 tensor) into the stored one."""
        t = self.tensors[name]
        if tensor.dtype != t.dtype:
            raise ValueError(f"set_tensor_by_name({name!r}): dtype {tensor.dtype}, stored {t.dtype}")
        if tuple(tensor.shape) == tuple(t.shape[:2]) and t.shape[2] == 1:
            tensor = tensor.unsqueeze(-1)
        if tuple(tensor.shape) != tuple(t.shape):
            raise ValueError(f"set_tensor_by_name({name!r}): shape {tuple(tensor.shape)}, stored {tuple(t.shape)}")
        t.copy_(tensor)

    def add_samples(self, **tensors):
        """Writes one time step — per name a ``[num_envs, size]`` tensor (``[num_envs]`` for a size-1 tensor) of the stored dtype — into
        row ``memory_index``, then advances the index; it wraps to 0 after ``memory_size`` rows and sets ``filled``."""
        if not tensors:
            raise ValueError("add_samples: no tensor given")
        rows = []
        for name, v in tensors.items():
            if name not in self.tensors:
                raise KeyError(f"add_samples: no tensor named {name!r} (create_tensor first)")
            t = self.tensors[name]
            if v.dtype != t.dtype:
                raise ValueError(f"add_samples({name!r}): dtype {v.dtype}, stored {t.dtype}")
            if v.dim() == 1 and t.shape[2] == 1:
                v = v.unsqueeze(-1)
            if tuple(v.shape) != tuple(t.shape[1:]):
                raise ValueError(f"add_samples({name!r}): shape {tuple(v.shape)}, expected {tuple(t.shape[1:])}")
            rows.append((t, v))
        for t, v in rows:
            t[self.memory_index].copy_(v)
        self.memory_index += 1
        if self.memory_index >= self.memory_size:
            self.memory_index = 0
            self.filled = True

    def sample_all(self, names, mini_batches=1, shuffle=False, generator=None):
        """-> ``mini_batches`` lists of tensors (one per name) over the flattened ``N = memory_size * num_envs`` rows, ``N // mini_batches``
        rows each; the remainder is dropped.  Unshuffled batches are views of the stored tensors (contiguous slices, no copy);
        ``shuffle=True`` gathers rows by ``torch.randperm(N, generator=generator)`` (a CPU generator: the same seed gives the same
        batches)."""
        mini_batches = int(mini_batches)
        n = self.memory_size * self.num_envs
        if mini_batches < 1:
            raise ValueError("sample_all: mini_batches must be >= 1")
        size = n // mini_batches
        flat = [self.get_tensor_by_name(name, keepdim=False) for name in names]
        if not shuffle:
            return [[t[i * size:(i + 1) * size] for t in flat] for i in range(mini_batches)]
        perm = torch.randperm(n, generator=generator).to(self.device)
        return [[t[perm[i * size:(i + 1) * size]] for t in flat] for i in range(mini_batches)]

    def reset(self):
        """Forgets what is stored (the tensors stay allocated, and keep their contents until overwritten)."""
        self.memory_index = 0
        self.filled = False


def compute_gae(engine, memory, last_values, discount_factor=0.99, lambda_coefficient=0.95, normalize=True, stats=None, stats_out=None):
    """skrl's ``compute_gae`` over a full memory: reads ``rewards``, ``terminated`` and ``values``, writes ``returns`` and ``advantages``
    into the memory (created if absent) with ``engine.gae`` on the stored tensors in place.  ``last_values`` [num_envs] or [num_envs, 1]:
    the critic's value of the current observation.  ``stats`` (3 float64 on the device): normalise with these moments instead of this
    memory's own — the global ones of a sharded rollout, combined from every shard's ``stats_out`` with ``combine_moments``;
    ``stats_out`` (3 float64 on the device, an addition to skrl's signature for that protocol) receives (count, mean, M2) of this memory's
    raw advantages.  The memory must have just been filled (``filled`` and ``memory_index == 0``): the recursion runs over all rows in
    storage order, so a partly filled or wrapped-around memory would mix rollouts — ValueError.
    Enqueues only; capturable in a graph once the two output tensors exist.  -> (returns, advantages), the stored tensors."""
    if not memory.filled or memory.memory_index != 0:
        raise ValueError(f"compute_gae: the memory holds {len(memory)} of {memory.memory_size * memory.num_envs} samples (row {memory.memory_index} is next): "
                         "it runs over all memory_size rows in storage order, so it wants a memory that has just been filled")
    returns = memory.create_tensor("returns", 1, torch.float32)
    advantages = memory.create_tensor("advantages", 1, torch.float32)
    get = memory.get_tensor_by_name
    engine.gae(get("rewards"), get("values"), get("terminated"), last_values, returns, advantages, gamma=discount_factor, lam=lambda_coefficient,
               normalize=normalize, stats_out=stats_out, stats_in=stats)
    return returns, advantages


combine_moments = _lib.combine_moments
