"""Adam with gradient-norm clipping on the MI355X: ``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.Adam.step()`` (no weight decay, no
amsgrad) over all parameter tensors in two launches (``Engine.optim_step``, csrc/rover_optim.hip; the arithmetic and its order are
written out in include/rover_step.h).

The state lives in this object: ``exp_avg`` / ``exp_avg_sq`` flat over all tensors in parameter order, ``steps`` (one int64: Adam's step
count, shared by all tensors) and ``stopped`` (one int32: the latch of the device-side early stop).  A gated step (``gate``, a float64
device scalar such as the KL in ``stats[3:]`` of ``Engine.ppo_loss``) is decided by the kernels: once ``gate > gate_threshold`` the latch
is set and every following step changes nothing until the caller zeroes it.  Nothing here synchronises.

The engine binds the parameters' and gradients' ADDRESSES when the optimiser is built: the parameter tensors and their ``.grad`` must
stay the same objects (``HeightmapNet.load_state_dict`` copies in place, ``HeightmapNet.backward`` overwrites ``.grad`` in place).
``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.Adam``'s layout, so either optimiser continues the other's run.
"""
from __future__ import annotations

import torch


class Adam:
    def __init__(self, engine, params, lr, betas=(0.9, 0.999), eps=1e-8):
        """``params``: float32 tensors with ``.grad`` (created as zeros where missing).  ``engine`` None: the state and its
        (de)serialisation only — ``step()`` then raises."""
        self.engine, self.params = engine, list(params)
        if not self.params:
            raise ValueError("Adam: no parameters")
        if not (lr >= 0.0 and eps >= 0.0 and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Adam: lr = {lr}, betas = {betas}, eps = {eps}")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        for p in self.params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        dev = self.params[0].device
        self.numel = [p.numel() for p in self.params]
        total = sum(self.numel)
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self.steps = torch.zeros(1, dtype=torch.int64, device=dev)
        self.stopped = torch.zeros(1, dtype=torch.int32, device=dev)
        self._handle = None
        if engine is not None:
            self._handle = engine.optim_create(self.params, [p.grad for p in self.params], self.exp_avg, self.exp_avg_sq, self.steps, self.stopped)

    def close(self):
        if self._handle is not None and getattr(self.engine, "_h", None):
            self.engine.optim_destroy(self._handle)
        self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, grad_norm_clip, gate=None, gate_threshold=0.0, norm_out=None):
        """Clip by the total gradient norm (``grad_norm_clip`` <= 0: no clipping) and step, unless the latch is set or ``gate >
        gate_threshold`` (then the latch is set and nothing else changes).  ``norm_out``: one float64 on the device, receives the norm
        before clipping.  Enqueues two launches."""
        if self._handle is None:
            raise RuntimeError("Adam.step: built without an engine")
        self.engine.optim_step(self._handle, self.lr, self.betas[0], self.betas[1], self.eps, grad_norm_clip, gate, gate_threshold, norm_out)

    def _views(self, flat):
        out, lo = [], 0
        for p, n in zip(self.params, self.numel):
            out.append(flat[lo:lo + n].view(p.shape))
            lo += n
        return out

    def state_dict(self):
        """``torch.optim.Adam.state_dict()``'s layout: per parameter index ``step`` (a float32 scalar tensor on the CPU, torch's default
        form), ``exp_avg`` and ``exp_avg_sq`` (copies, shaped as the parameter), and one param group.  Reads the step count (synchronises)."""
        step = float(self.steps.item())
        state = {i: {"step": torch.tensor(step, dtype=torch.float32), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
                 for i, (m, v) in enumerate(zip(self._views(self.exp_avg), self._views(self.exp_avg_sq)))}
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": 0, "amsgrad": False, "maximize": False, "foreach": None,
                 "capturable": False, "differentiable": False, "fused": None, "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        """Takes ``state_dict()``'s output or a ``torch.optim.Adam``'s over the same parameters (one param group, no weight decay, no
        amsgrad, not maximize); lr, betas and eps are taken over.  A torch optimiser that has not stepped yet has an empty state: zeros
        and step 0.  Parameters without an entry must then be all of them (Adam here keeps ONE step count)."""
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError(f"Adam.load_state_dict: expected one param group of {len(self.params)} parameters")
        g = groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("Adam.load_state_dict: weight_decay, amsgrad and maximize are not supported")
        state = sd["state"]
        ids = list(g["params"])
        if state and any(i not in state for i in ids):
            raise ValueError("Adam.load_state_dict: some parameters have a state and some have none")
        steps = {float(state[i]["step"]) for i in ids} if state else {0.0}
        if len(steps) != 1 or next(iter(steps)) != int(next(iter(steps))) or next(iter(steps)) < 0:
            raise ValueError(f"Adam.load_state_dict: the parameters' step counts {sorted(steps)} are not one whole number")
        for name in ("exp_avg", "exp_avg_sq"):
            for i, p in zip(ids, self.params):
                if state and tuple(state[i][name].shape) != tuple(p.shape):
                    raise ValueError(f"Adam.load_state_dict: {name} of parameter {i} is {tuple(state[i][name].shape)}, expected {tuple(p.shape)}")
        for name, flat in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            for i, dst in zip(ids, self._views(flat)):
                if state:
                    dst.copy_(state[i][name].to(device=dst.device, dtype=torch.float32))
                else:
                    dst.zero_()
        self.steps.fill_(int(next(iter(steps))))
        self.lr, self.betas, self.eps = float(g["lr"]), (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])
