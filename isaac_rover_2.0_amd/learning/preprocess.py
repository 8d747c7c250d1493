"""skrl's ``RunningStandardScaler`` on the MI355X: the preprocessor every skrl PPO recipe for Isaac tasks passes for states and values.

The reference's ``train.py`` imports it (``omniisaacgymenvs/train.py``); skrl is no dependency of this package, so the semantics are
restated in ``include/rover_step.h`` (``rover_scaler_update``, ``rover_scaler_apply``).  The state is skrl's, float64 on the device:
``running_mean`` [size] = 0, ``running_variance`` [size] = 1 and ``current_count`` = 1 (one pseudo-sample).  A train call folds the batch's
column means and UNBIASED variances into it (two launches, f64 accumulation, no atomics: the same bits on every run); the forward is
``clamp((x - mean) / (sqrt(var) + epsilon), -clip, clip)`` and the inverse ``sqrt(var) * clamp(x, -clip, clip) + mean``, in f32 with the
statistics rounded to f32 first (one launch).  A call with ``train=True`` updates first and normalises with the new statistics.

One deviation: a train call on fewer than 2 rows is refused (skrl's variance of one row is a NaN that poisons the state for good).

Nothing here reads the device: a call enqueues one to three launches and can be captured in a graph once the scratch has its size
(it is sized for the largest batch seen and grows only outside a capture).
"""
from __future__ import annotations

import torch

KEYS = ("running_mean", "running_variance", "current_count")


class RunningStandardScaler:
    def __init__(self, engine, size, epsilon=1e-8, clip_threshold=5.0, device=None):
        """``engine``: the ``Engine`` whose library runs the kernels (None: the state and its (de)serialisation only — a call then
        raises); ``size``: the number of columns, 1 .. 4096; ``device``: where the state lives (default: the engine's)."""
        size = int(size)
        if not 1 <= size <= 4096:
            raise ValueError(f"RunningStandardScaler: size = {size} outside 1 .. 4096")
        epsilon, clip_threshold = float(epsilon), float(clip_threshold)
        if not (0.0 <= epsilon < float("inf")) or not (0.0 <= clip_threshold < float("inf")):
            raise ValueError(f"RunningStandardScaler: epsilon = {epsilon} and clip_threshold = {clip_threshold} must be finite and >= 0")
        if device is None:
            if engine is None:
                raise ValueError("RunningStandardScaler: a device must be given where there is no engine")
            device = engine.device
        self.engine, self.size, self.epsilon, self.clip_threshold = engine, size, epsilon, clip_threshold
        self.device = torch.device(device)
        self.running_mean = torch.zeros(size, dtype=torch.float64, device=self.device)
        self.running_variance = torch.ones(size, dtype=torch.float64, device=self.device)
        self.current_count = torch.ones(1, dtype=torch.float64, device=self.device)
        self._scratch = None

    def _rows(self, x, name):
        """``x`` as [M, size] without a copy: [M, size], [T, E, size], and [M] / [T, E] where size is 1."""
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise ValueError(f"RunningStandardScaler: {name} must be a float32 tensor")
        if x.dim() >= 2 and x.shape[-1] == self.size and x.dim() <= 3:
            lead = x.shape[:-1]
        elif self.size == 1 and 1 <= x.dim() <= 2:
            lead = x.shape
        else:
            raise ValueError(f"RunningStandardScaler: {name} is {tuple(x.shape)}, expected [M, {self.size}] or [T, E, {self.size}]"
                             + (", [M] or [T, E]" if self.size == 1 else ""))
        if len(lead) == 1 and x.dim() == 2 and x.stride(1) == 1:
            return x                                                     # a row-strided matrix goes through as it is
        if not x.is_contiguous():
            raise ValueError(f"RunningStandardScaler: {name} must be contiguous (or a matrix with unit column stride)")
        return x.view(-1, self.size)

    def _scratch_for(self, m):
        need = self.engine.scaler_plan(m, self.size)["scratch_bytes"]
        if self._scratch is None or self._scratch.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"RunningStandardScaler: the scratch would have to grow to {need} bytes inside a graph capture: make one "
                                   "train call of this size before capturing")
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._scratch

    def __call__(self, x, train=False, inverse=False, out=None, skip_if=None):
        """``x`` normalised (or, with ``inverse``, denormalised) -> a tensor of x's shape: a new one, or ``out`` (``out=x``: in place).
        ``train``: fold x into the statistics first; ``skip_if`` (one int32 on the device): nonzero when the kernels run leaves the
        statistics unchanged (the normalisation still happens)."""
        if self.engine is None:
            raise RuntimeError("RunningStandardScaler: built without an engine")
        rows = self._rows(x, "x")
        if train:
            if rows.shape[0] < 2:
                raise ValueError(f"RunningStandardScaler: a train call needs at least 2 rows (got {rows.shape[0]}): the unbiased variance of "
                                 "one row is undefined")
            self.engine.scaler_update(rows, self.running_mean, self.running_variance, self.current_count, self._scratch_for(rows.shape[0]), skip_if)
        elif skip_if is not None:
            raise ValueError("RunningStandardScaler: skip_if belongs to a train call")
        if out is None:
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        elif tuple(out.shape) != tuple(x.shape):
            raise ValueError(f"RunningStandardScaler: out is {tuple(out.shape)}, x {tuple(x.shape)}")
        self.engine.scaler_apply(rows, self.running_mean, self.running_variance, self._rows(out, "out"), epsilon=self.epsilon,
                                 clip=self.clip_threshold, inverse=inverse)
        return out

    def state_dict(self):
        """skrl's three keys, float64 copies: ``running_mean`` [size], ``running_variance`` [size], ``current_count`` (a scalar)."""
        return {"running_mean": self.running_mean.clone(), "running_variance": self.running_variance.clone(),
                "current_count": self.current_count[0].clone()}

    def load_state_dict(self, sd):
        """Takes ``state_dict()``'s output or the ``state_preprocessor`` / ``value_preprocessor`` entry of a skrl agent checkpoint; copies
        in place (a captured graph keeps reading the same memory)."""
        missing = [k for k in KEYS if k not in sd]
        if missing:
            raise ValueError(f"RunningStandardScaler.load_state_dict: missing {missing}")
        mean, var, count = (torch.as_tensor(sd[k]).to(dtype=torch.float64) for k in KEYS)
        if tuple(mean.shape) != (self.size,) or tuple(var.shape) != (self.size,) or count.numel() != 1:
            raise ValueError(f"RunningStandardScaler.load_state_dict: running_mean {tuple(mean.shape)} / running_variance {tuple(var.shape)} / "
                             f"current_count {tuple(count.shape)}, expected ({self.size},), ({self.size},) and one number")
        self.running_mean.copy_(mean)
        self.running_variance.copy_(var)
        self.current_count.copy_(count.reshape(1))
