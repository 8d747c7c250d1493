"""The PPO weight update for the policy nets of ``learning/model.py`` on the MI355X: skrl's ``PPO._update`` without autograd.

The reference trains through skrl (``omniisaacgymenvs/train.py:82-124``) with ``PPO_DEFAULT_CONFIG`` overridden by
``cfg/trainSKRL/RoverPPOSKRL.yaml``; ``DEFAULT_CONFIG`` below holds those values under skrl's key names.  ``train.py`` imports
``RunningStandardScaler`` and ``KLAdaptiveRL`` but never passes them: there are no preprocessors and no scheduler here either.  The
semantics are restated from a reading of skrl 1.x (skrl is no dependency of this package); the loss and its gradients are written out
in ``include/rover_step.h`` (``rover_ppo_loss``).

Per minibatch: the actor's forward on the stored states with the stored actions as ``taken_actions`` (the noise counter does not move),
the critic's forward, ``Engine.ppo_loss`` (losses, KL and the gradients at both outputs in one launch plus a merge), both nets'
``backward`` (``rover_linear_backward`` per layer), then gradient-norm clipping and one Adam step over both nets' parameters.

The optimiser step has two forms.  By default (``native_step=False``) it is ``torch.nn.utils.clip_grad_norm_`` and ``torch.optim.Adam``
on plain tensors with ``.grad`` set: torch plumbing, some dozens of launches.  ``native_step=True`` runs ``learning/optim.py``'s ``Adam``
instead: ``rover_optim_step``, two launches over all 33 tensors, deterministic, the clipped gradient not written back (``.grad`` keeps
the unclipped one).  Both keep Adam's state in torch's ``state_dict`` layout.

The KL early stop has two forms as well.  ``kl_stop="host"`` (the default) reads the minibatch's KL on the host before its step, as
skrl does: one stream drain per minibatch.  ``kl_stop="device"`` (needs ``native_step``) hands the KL to the native step as its gate:
every minibatch of every epoch is enqueued, the kernels skip the steps after the one whose KL exceeded the threshold (a latch, zeroed
at the start of each epoch), and ``update()`` reads the per-epoch step counts once at its end.  The parameters come out bit-equal to
the host form's; the skipped minibatches still cost their forward, loss and backward.

Out of scope: the backward of the fused chain kernels (the update runs every layer as its own launch), gradient all-reduce across ranks,
preprocessors, learning-rate schedulers, bf16 / fp16 training.

Training precision is f32 whatever the nets' ``precision``: the update's forwards pass ``precision="f32"`` explicitly.  A rollout may
ACT in bf16 (``HeightmapNet(precision="bf16")``): the stored ``log_prob`` is then the bf16 behaviour policy's own, the ratio
``pi_new / pi_behaviour`` is exact, and only the KL estimate of the first minibatch picks up the small f32 - bf16 offset.
"""
from __future__ import annotations

from itertools import chain

import torch

from .optim import Adam
from .rollout import compute_gae

# cfg/trainSKRL/RoverPPOSKRL.yaml over skrl's PPO_DEFAULT_CONFIG
DEFAULT_CONFIG = {
    "learning_epochs": 4, "mini_batches": 60, "discount_factor": 0.99, "lambda": 0.95, "learning_rate": 1e-4, "grad_norm_clip": 1.0,
    "ratio_clip": 0.2, "value_clip": 0.2, "clip_predicted_values": True, "entropy_loss_scale": 0.0, "value_loss_scale": 1.0,
    "kl_threshold": 0.008,
}
NAMES = ("states", "actions", "log_prob", "values", "returns", "advantages")
STATS = ("policy_loss", "value_loss", "entropy_loss", "kl")


class PPO:
    def __init__(self, engine, policy, value, memory, cfg=None, generator=None, native_step=False, kl_stop="host"):
        """``policy`` / ``value``: the actor and critic ``HeightmapNet``; ``memory``: a ``RolloutMemory`` holding ``NAMES`` plus rewards and
        terminated; ``cfg``: skrl's keys over ``DEFAULT_CONFIG`` (an unknown key is an error); ``generator``: the CPU generator that
        shuffles the minibatches (the same seed gives the same batches); ``native_step``: the optimiser step as two HIP launches
        (``learning/optim.py``) instead of torch's; ``kl_stop``: "host" or "device" (module docstring; "device" needs ``native_step``)."""
        if kl_stop not in ("host", "device"):
            raise ValueError(f"PPO: kl_stop must be 'host' or 'device' (got {kl_stop!r})")
        if kl_stop == "device" and not native_step:
            raise ValueError("PPO: kl_stop='device' needs native_step=True (the gate is part of the native optimiser step)")
        unknown = sorted(set(cfg or {}) - set(DEFAULT_CONFIG))
        if unknown:
            raise ValueError(f"PPO: unknown cfg keys {unknown} (known: {sorted(DEFAULT_CONFIG)})")
        self.cfg = {**DEFAULT_CONFIG, **(cfg or {})}
        rows = memory.memory_size * memory.num_envs
        if int(self.cfg["mini_batches"]) < 1 or rows // int(self.cfg["mini_batches"]) < 1:
            raise ValueError(f"PPO: mini_batches = {self.cfg['mini_batches']} leaves no row per minibatch of the memory's {rows}")
        if int(self.cfg["learning_epochs"]) < 1:
            raise ValueError("PPO: learning_epochs must be >= 1")
        if policy.log_std_parameter is None or value.log_std_parameter is not None:
            raise ValueError("PPO: policy must be the stochastic actor, value the deterministic critic")
        if policy.reduction != "sum":
            raise ValueError("PPO: the log-prob reduction must be 'sum' (the reference's)")
        self.engine, self.policy, self.value, self.memory, self.generator = engine, policy, value, memory, generator
        self.params = list(chain(policy.parameters(), value.parameters()))
        for p in self.params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        self.native_step, self.kl_stop = bool(native_step), kl_stop
        if self.native_step:
            self.optimizer = Adam(engine, self.params, lr=float(self.cfg["learning_rate"]))
        else:
            self.optimizer = torch.optim.Adam(self.params, lr=float(self.cfg["learning_rate"]))
        dev = policy.device
        self._stats = torch.zeros(4, dtype=torch.float64, device=dev)
        self._sum = torch.zeros(4, dtype=torch.float64, device=dev)
        self._d = {}
        self.minibatches_done = []                 # optimiser steps per epoch of the last update()

    def _grads(self, rows, a):
        d = self._d.get(rows)
        if d is None:
            dev = self.policy.device
            d = self._d[rows] = (torch.empty(rows, a, device=dev), torch.empty(rows, 1, device=dev))
        return d

    def minibatch(self, states, actions, log_prob, values, returns, advantages):
        """Forward of both nets, the loss and every gradient of one minibatch (no optimiser step) -> the device stats tensor.  Enqueues
        only; after one warm-up call of the same size it can be captured in a graph."""
        c, pol = self.cfg, self.policy
        _, _, out = pol.act(states, taken_actions=actions, fused=False, precision="f32")
        v, _, _ = self.value.act(states, fused=False, precision="f32")
        d_mean, d_value = self._grads(states.shape[0], actions.shape[1])
        self.engine.ppo_loss(out["mean_actions"], pol.log_std_parameter, actions, log_prob, advantages, v, values, returns, d_mean, d_value,
                             pol.log_std_parameter.grad, self._stats, ratio_clip=c["ratio_clip"], value_clip=c["value_clip"],
                             clip_predicted_values=c["clip_predicted_values"], entropy_loss_scale=c["entropy_loss_scale"],
                             value_loss_scale=c["value_loss_scale"], clip_log_std=pol.clip_log_std, min_log_std=pol.min_log_std,
                             max_log_std=pol.max_log_std)
        return self._stats

    def backward(self, rows, a):
        d_mean, d_value = self._grads(rows, a)
        self.policy.backward(d_mean)
        self.value.backward(d_value)

    def step(self, gate=None, gate_threshold=0.0):
        """The optimiser step on the gradients in ``.grad``.  ``gate`` (native step only): a float64 device scalar; the step is skipped
        and the optimiser's ``stopped`` latch set once ``gate > gate_threshold``."""
        if self.native_step:
            self.optimizer.step(float(self.cfg["grad_norm_clip"]), gate=gate, gate_threshold=gate_threshold)
            return
        if gate is not None:
            raise ValueError("PPO.step: a gate needs native_step=True")
        if self.cfg["grad_norm_clip"] > 0:
            torch.nn.utils.clip_grad_norm_(self.params, float(self.cfg["grad_norm_clip"]))
        self.optimizer.step()

    def update(self, last_values):
        """skrl's ``PPO._update``: compute_gae, then ``learning_epochs`` passes over ``mini_batches`` shuffled minibatches.  KL early stop
        as skrl does it: with ``kl_threshold`` > 0 and ``kl_stop="host"`` the minibatch's KL is read on the host (one 8-byte read) and,
        when it exceeds the threshold, the rest of that epoch is skipped before the minibatch's step; with ``kl_stop="device"`` the
        native step decides the same on the device and the call synchronises once, at its end, to read ``minibatches_done``; with
        ``kl_threshold`` 0 nothing synchronises.
        -> {policy_loss, value_loss, entropy_loss, kl}: the last epoch's means over its stepped minibatches, float64 device scalars."""
        c = self.cfg
        compute_gae(self.engine, self.memory, last_values, discount_factor=c["discount_factor"], lambda_coefficient=c["lambda"])
        self.minibatches_done = []
        if self.kl_stop == "device" and c["kl_threshold"] > 0:
            return self._update_device_stop()
        for _ in range(int(c["learning_epochs"])):
            self._sum.zero_()
            done = 0
            for batch in self.memory.sample_all(NAMES, int(c["mini_batches"]), shuffle=True, generator=self.generator):
                stats = self.minibatch(*batch)
                if c["kl_threshold"] > 0 and float(stats[3]) > c["kl_threshold"]:
                    break
                self.backward(batch[0].shape[0], batch[1].shape[1])
                self.step()
                self._sum += stats
                done += 1
            self.minibatches_done.append(done)
        mean = self._sum / max(self.minibatches_done[-1], 1)
        return {k: mean[i] for i, k in enumerate(STATS)}

    def _update_device_stop(self):
        """The epochs with the KL stop on the device: every minibatch is enqueued, the native step is gated by the minibatch's KL, and
        ``_sum`` takes the stats of the minibatches that stepped (the latch is read on the device).  The per-epoch step counts are the
        differences of the optimiser's step counter, copied on the device after each epoch and read once at the end."""
        c, opt = self.cfg, self.optimizer
        marks = [opt.steps.clone()]
        for _ in range(int(c["learning_epochs"])):
            self._sum.zero_()
            opt.stopped.zero_()
            for batch in self.memory.sample_all(NAMES, int(c["mini_batches"]), shuffle=True, generator=self.generator):
                stats = self.minibatch(*batch)
                self.backward(batch[0].shape[0], batch[1].shape[1])
                self.step(gate=stats[3:], gate_threshold=float(c["kl_threshold"]))
                self._sum += torch.where(opt.stopped == 0, stats, torch.zeros_like(stats))
            marks.append(opt.steps.clone())
        counts = torch.cat(marks).cpu()                    # the update's one synchronisation
        self.minibatches_done = [int(b - a) for a, b in zip(counts[:-1], counts[1:])]
        mean = self._sum / max(self.minibatches_done[-1], 1)
        return {k: mean[i] for i, k in enumerate(STATS)}
