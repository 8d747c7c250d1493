"""The PPO weight update for the policy nets of ``learning/model.py`` on the MI355X: skrl's ``PPO._update`` without autograd.

The reference trains through skrl (``omniisaacgymenvs/train.py:82-124``) with ``PPO_DEFAULT_CONFIG`` overridden by
``cfg/trainSKRL/RoverPPOSKRL.yaml``; ``DEFAULT_CONFIG`` below holds those values under skrl's key names.  ``train.py`` imports
``RunningStandardScaler`` and ``KLAdaptiveRL`` but never passes them: by default there are no preprocessors and no scheduler here
either, and both are opt-in (below).  The semantics are restated from a reading of skrl 1.x (skrl is no dependency of this package); the loss and its gradients are written out
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

Preprocessors (``state_preprocessor`` / ``value_preprocessor``: ``learning/preprocess.py``'s ``RunningStandardScaler``) go
where skrl's ``act``, ``record_transition`` and ``_update`` put them.  Rollout (the loop lives in the caller): both nets read
``preprocess_states(obs)`` (no training), the critic's output is stored as ``denormalize_values(v)``, and ``last_values`` is denormalised
the same way before ``update()``.  Update, after GAE on the raw values: the stored ``values`` become ``value_pre(values, train=True)``,
then the stored ``returns`` ``value_pre(returns, train=True)`` — two train calls in this order, both in place in the memory; the
advantages stay as GAE left them.  Per minibatch ``states = state_pre(states, train=(epoch == 0))`` in place on the gathered batch,
before both forwards.  With ``kl_stop="device"`` that train call takes the optimiser's ``stopped`` latch as its ``skip_if``: the
minibatches after the stopping one leave the statistics alone, as the host form never reaches them, and parameters AND scaler state
come out bit-equal between the two forms.  (The stopping minibatch itself has trained the scaler in both forms: skrl preprocesses
before it evaluates the KL.)

``lr_scheduler``: a ``KLAdaptiveRL`` (skrl's), stepped once per epoch with the mean KL of every minibatch evaluated in that epoch, the one
that stopped it included; one 8-byte host read per epoch.  Refused with ``kl_stop="device"``, which enqueues every epoch before it reads
anything.

Out of scope: the backward of the fused chain kernels (the update runs every layer as its own launch), gradient all-reduce across ranks,
bf16 / fp16 training, schedulers other than the KL-adaptive one, combining scaler statistics across ranks.

Training precision is f32 whatever the nets' ``precision``: the update's forwards pass ``precision="f32"`` explicitly.  A rollout may
ACT in bf16 (``HeightmapNet(precision="bf16")``): the stored ``log_prob`` is then the bf16 behaviour policy's own, the ratio
``pi_new / pi_behaviour`` is exact, and only the KL estimate of the first minibatch picks up the small f32 - bf16 offset.
"""
from __future__ import annotations

from itertools import chain

import torch

from .optim import Adam
from .preprocess import RunningStandardScaler
from .rollout import compute_gae

# cfg/trainSKRL/RoverPPOSKRL.yaml over skrl's PPO_DEFAULT_CONFIG
DEFAULT_CONFIG = {
    "learning_epochs": 4, "mini_batches": 60, "discount_factor": 0.99, "lambda": 0.95, "learning_rate": 1e-4, "grad_norm_clip": 1.0,
    "ratio_clip": 0.2, "value_clip": 0.2, "clip_predicted_values": True, "entropy_loss_scale": 0.0, "value_loss_scale": 1.0,
    "kl_threshold": 0.008,
}
NAMES = ("states", "actions", "log_prob", "values", "returns", "advantages")
STATS = ("policy_loss", "value_loss", "entropy_loss", "kl")


class KLAdaptiveRL:
    """skrl's ``KLAdaptiveRL``: ``step(kl)`` divides the learning rate by ``lr_factor`` when ``kl > kl_threshold * kl_factor`` (not below
    ``min_lr``), multiplies it when ``kl < kl_threshold / kl_factor`` (not above ``max_lr``), and leaves it alone otherwise — exact ties
    included.  ``kl_threshold`` is the scheduler's own, not PPO's early-stop threshold.  ``optimizer``: ``learning/optim.py``'s ``Adam``
    (its ``lr``) or a ``torch.optim`` optimiser (its param groups); ``PPO`` binds its own when the scheduler is built without one."""

    def __init__(self, optimizer=None, kl_threshold=0.008, min_lr=1e-6, max_lr=1e-2, kl_factor=2, lr_factor=1.5):
        if not (kl_threshold > 0 and 0 < min_lr <= max_lr and kl_factor > 0 and lr_factor > 0):
            raise ValueError(f"KLAdaptiveRL: kl_threshold = {kl_threshold}, min_lr = {min_lr}, max_lr = {max_lr}, kl_factor = {kl_factor}, "
                             f"lr_factor = {lr_factor}")
        self.optimizer, self.kl_threshold, self.min_lr, self.max_lr = optimizer, float(kl_threshold), float(min_lr), float(max_lr)
        self.kl_factor, self.lr_factor = float(kl_factor), float(lr_factor)

    @staticmethod
    def rule(lr, kl, kl_threshold=0.008, min_lr=1e-6, max_lr=1e-2, kl_factor=2.0, lr_factor=1.5):
        if kl > kl_threshold * kl_factor:
            return max(lr / lr_factor, min_lr)
        if kl < kl_threshold / kl_factor:
            return min(lr * lr_factor, max_lr)
        return lr

    def get_lr(self):
        opt = self.optimizer
        return float(opt.param_groups[0]["lr"]) if hasattr(opt, "param_groups") else float(opt.lr)

    def step(self, kl):
        """One scheduler step on the host number ``kl`` -> the learning rate now in force."""
        if self.optimizer is None:
            raise RuntimeError("KLAdaptiveRL.step: no optimizer bound")
        opt = self.optimizer
        if hasattr(opt, "param_groups"):
            for g in opt.param_groups:
                g["lr"] = self.rule(float(g["lr"]), float(kl), self.kl_threshold, self.min_lr, self.max_lr, self.kl_factor, self.lr_factor)
        else:
            opt.lr = self.rule(float(opt.lr), float(kl), self.kl_threshold, self.min_lr, self.max_lr, self.kl_factor, self.lr_factor)
        return self.get_lr()


class PPO:
    def __init__(self, engine, policy, value, memory, cfg=None, generator=None, native_step=False, kl_stop="host", state_preprocessor=None,
                 value_preprocessor=None, lr_scheduler=None):
        """``policy`` / ``value``: the actor and critic ``HeightmapNet``; ``memory``: a ``RolloutMemory`` holding ``NAMES`` plus rewards and
        terminated; ``cfg``: skrl's keys over ``DEFAULT_CONFIG`` (an unknown key is an error); ``generator``: the CPU generator that
        shuffles the minibatches (the same seed gives the same batches); ``native_step``: the optimiser step as two HIP launches
        (``learning/optim.py``) instead of torch's; ``kl_stop``: "host" or "device" (module docstring; "device" needs ``native_step``);
        ``state_preprocessor`` / ``value_preprocessor``: ``RunningStandardScaler`` instances of the states' width / of size 1, or None;
        ``lr_scheduler``: a ``KLAdaptiveRL`` or None (not with ``kl_stop="device"``)."""
        if kl_stop not in ("host", "device"):
            raise ValueError(f"PPO: kl_stop must be 'host' or 'device' (got {kl_stop!r})")
        if kl_stop == "device" and not native_step:
            raise ValueError("PPO: kl_stop='device' needs native_step=True (the gate is part of the native optimiser step)")
        if lr_scheduler is not None and not isinstance(lr_scheduler, KLAdaptiveRL):
            raise ValueError("PPO: lr_scheduler must be a KLAdaptiveRL instance")
        if lr_scheduler is not None and kl_stop == "device":
            raise ValueError("PPO: lr_scheduler cannot be used with kl_stop='device' (that mode enqueues all epochs before reading any KL)")
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
        for pre, name in ((state_preprocessor, "state_preprocessor"), (value_preprocessor, "value_preprocessor")):
            if pre is None:
                continue
            if not isinstance(pre, RunningStandardScaler):
                raise ValueError(f"PPO: {name} must be a RunningStandardScaler instance")
            size = 1 if pre is value_preprocessor else policy.num_proprioception + policy.num_sparse + policy.num_dense
            if pre.size != size:
                raise ValueError(f"PPO: {name} has size {pre.size}, expected {size}")
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
        self.state_preprocessor, self.value_preprocessor, self.lr_scheduler = state_preprocessor, value_preprocessor, lr_scheduler
        if lr_scheduler is not None:
            lr_scheduler.optimizer = self.optimizer
            self._kl_sum = torch.zeros(1, dtype=torch.float64, device=dev)
        self.learning_rates = []                   # with a scheduler: the learning rate after each epoch of the last update()

    def preprocess_states(self, obs, out=None):
        """What the nets read during a rollout: ``state_preprocessor(obs)`` without training (``obs`` itself where there is none)."""
        return obs if self.state_preprocessor is None else self.state_preprocessor(obs, out=out)

    def denormalize_values(self, v, out=None):
        """What the memory stores for the critic's output ``v``, and what ``update()`` takes as ``last_values``:
        ``value_preprocessor(v, inverse=True)`` (``v`` itself where there is none)."""
        return v if self.value_preprocessor is None else self.value_preprocessor(v, inverse=True, out=out)

    def _normalize_states(self, batch, epoch, skip_if=None):
        """``states = state_pre(states, train=(epoch == 0))`` in place on the minibatch — a gathered copy, never the memory's rows."""
        if self.state_preprocessor is None:
            return
        states = batch[0]
        stored = self.memory.get_tensor_by_name("states")
        lo, hi = stored.data_ptr(), stored.data_ptr() + stored.numel() * stored.element_size()
        assert not lo <= states.data_ptr() < hi, "PPO: the minibatch's states alias the memory (sample_all must gather copies)"
        self.state_preprocessor(states, train=(epoch == 0), out=states, skip_if=skip_if if epoch == 0 else None)

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
        if self.value_preprocessor is not None:                    # two train calls in this order, in place in the memory
            for name in ("values", "returns"):
                t = self.memory.get_tensor_by_name(name)
                self.value_preprocessor(t, train=True, out=t)
        self.minibatches_done, self.learning_rates = [], []
        if self.kl_stop == "device" and c["kl_threshold"] > 0:
            return self._update_device_stop()
        for epoch in range(int(c["learning_epochs"])):
            self._sum.zero_()
            done = seen = 0
            if self.lr_scheduler is not None:
                self._kl_sum.zero_()
            for batch in self.memory.sample_all(NAMES, int(c["mini_batches"]), shuffle=True, generator=self.generator):
                self._normalize_states(batch, epoch)
                stats = self.minibatch(*batch)
                if self.lr_scheduler is not None:                  # skrl appends the KL before the stop test
                    self._kl_sum += stats[3:]
                    seen += 1
                if c["kl_threshold"] > 0 and float(stats[3]) > c["kl_threshold"]:
                    break
                self.backward(batch[0].shape[0], batch[1].shape[1])
                self.step()
                self._sum += stats
                done += 1
            self.minibatches_done.append(done)
            if self.lr_scheduler is not None:
                self.learning_rates.append(self.lr_scheduler.step(float(self._kl_sum) / seen))      # the epoch's one 8-byte read
        mean = self._sum / max(self.minibatches_done[-1], 1)
        return {k: mean[i] for i, k in enumerate(STATS)}

    def _update_device_stop(self):
        """The epochs with the KL stop on the device: every minibatch is enqueued, the native step is gated by the minibatch's KL, and
        ``_sum`` takes the stats of the minibatches that stepped (the latch is read on the device).  The per-epoch step counts are the
        differences of the optimiser's step counter, copied on the device after each epoch and read once at the end."""
        c, opt = self.cfg, self.optimizer
        marks = [opt.steps.clone()]
        for epoch in range(int(c["learning_epochs"])):
            self._sum.zero_()
            opt.stopped.zero_()
            for batch in self.memory.sample_all(NAMES, int(c["mini_batches"]), shuffle=True, generator=self.generator):
                self._normalize_states(batch, epoch, skip_if=opt.stopped)
                stats = self.minibatch(*batch)
                self.backward(batch[0].shape[0], batch[1].shape[1])
                self.step(gate=stats[3:], gate_threshold=float(c["kl_threshold"]))
                self._sum += torch.where(opt.stopped == 0, stats, torch.zeros_like(stats))
            marks.append(opt.steps.clone())
        counts = torch.cat(marks).cpu()                    # the update's one synchronisation
        self.minibatches_done = [int(b - a) for a, b in zip(counts[:-1], counts[1:])]
        mean = self._sum / max(self.minibatches_done[-1], 1)
        return {k: mean[i] for i, k in enumerate(STATS)}
