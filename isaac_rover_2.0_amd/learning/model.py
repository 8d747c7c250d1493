"""Policy / value networks that consume the rover observation layout — forward pass on the MI355X.

Mirrors ``omniisaacgymenvs/learning/model.py``: ``Layer`` (:84-121, Linear + activation), ``Encoder`` (:122-150),
``StochasticActorHeightmap.compute`` (:185-195) and ``DeterministicHeightmap.compute`` (:231-241): obs is sliced as
``[proprioceptive | sparse | dense]``, each heightmap slice goes through its encoder (default 80 → 60,
``cfg/trainSKRL/RoverPPOSKRL.yaml:7-9``), the results are concatenated with the proprioceptive values and fed to the
MLP (256 → 160 → 128, yaml :3-5) with a Tanh head of 2 (actor) or a linear head of 1 (critic).

``act()`` adds what a rollout asks of the actor (skrl's ``GaussianMixin``, built by the reference with ``clip_actions=False,
clip_log_std=True, min_log_std=-20, max_log_std=2, reduction="sum"``, model.py:153-156): a sampled action, its log-probability and the
log-probability of actions taken earlier — inside the kernel that ends the forward (``rover_mlp_chain_act``), with counter-based
noise keyed by (seed, call counter, GLOBAL row), so a shard draws its slice of the whole batch's noise.  The critic's ``act()`` is
``DeterministicMixin``'s (:198-201).

Nets that fit the library's chain kernels run each encoder and the MLP + head as ONE fused kernel each (``rover_mlp_chain_forward``,
f32 MFMA, activations kept in registers between the layers); otherwise every ``Layer`` is one ``rover_linear_forward`` launch.  Which
it is, the library says (``HeightmapNet._plan``); this file holds no width or row limit.  The slices are read in place from ``obs_buf``
and the encoder outputs are written straight into the concat buffer, so there is no ``torch.cat``.  These classes hold plain
tensors, initialised like ``nn.Linear``, and can load a ``state_dict`` saved from the reference's modules (same parameter names).

Training: autograd cannot see the kernels, so ``backward(d_out)`` walks an UNFUSED forward back layer by layer with
``rover_linear_backward`` and leaves every parameter's gradient in its ``.grad``; ``parameters()`` hands the tensors to a torch
optimiser.  The PPO loss at the outputs and the update loop (skrl's ``PPO._update``) live in ``learning/ppo.py``.  The backward of
the fused chain kernels is not built.

``precision="bf16"`` (opt-in, inference only): the same three chains with bf16 operands and f32 accumulation
(``rover_mlp_chain_forward_bf16`` / ``rover_mlp_chain_act_bf16``: every input, weight and hidden activation rounded to bf16, f32 bias,
activation and Gaussian head; the arithmetic is stated in ``include/rover_step.h``, the reasoning in DESIGN.md §4.13).  What a rollout
stores is the acting policy's own action, log-probability and value, so PPO's ratio stays exact; training, and ``act(taken_actions=...)``
inside the update, stay f32.
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

# how a forward runs: both encoders through chain_pair_forward; else each encoder, and the MLP + head, as a chain kernel or layer by layer
ForwardPlan = namedtuple("ForwardPlan", "pair enc0 enc1 mlp")


class Layer:
    def __init__(self, in_channels, out_channels, activation_function="elu", device="cuda:0", generator=None):
        bound = 1.0 / math.sqrt(in_channels) if in_channels > 0 else 0.0      # nn.Linear.reset_parameters (fan_in 0: zeros)
        self.weight = (torch.rand(out_channels, in_channels, generator=generator) * 2 - 1).mul_(bound).to(device)
        self.bias = (torch.rand(out_channels, generator=generator) * 2 - 1).mul_(bound).to(device)
        self.activation = activation_function


class HeightmapNet:
    """Shared body of the reference's two model classes; ``head_activation`` 'tanh' = actor, None = critic."""

    def __init__(self, engine, num_observations, num_sparse, num_dense, num_outputs, head_activation, mlp_features=(256, 160, 128),
                 encoder_features=(80, 60), activation_function="leakyrelu", device="cuda:0", seed=0, clip_actions=False, clip_log_std=True,
                 min_log_std=-20.0, max_log_std=2.0, reduction="sum", row_offset=0, action_low=-1.0, action_high=1.0, precision="f32"):
        """``precision``: "f32" (default) or "bf16" — what compute() / act() run when their own ``precision`` argument is None.  bf16 is
        for large rollout batches.  Measured on an MI355X with the native 1 750-float obs (EXPERIMENTS.md §19): act() in f32 is faster at
        512 and 4 096 rows (63 against 83 us, 80 against 103 us: the f32 split-k / mlp_small routes), the two are level at 8 192 rows
        (107 us each), and bf16 is faster from 16 384 rows on (111 against 177 us; 187 against 337 us at 65 536).
        ``seed`` initialises the weights and keys the action noise; ``row_offset``: the global row of this net's row 0 (a shard's
        env_offset); ``clip_*`` / ``min_log_std`` / ``max_log_std`` / ``reduction``: skrl's mixin arguments (model.py:153-156,198-201);
        ``action_low`` / ``action_high``: the action space's bounds, used only with ``clip_actions``."""
        g = torch.Generator().manual_seed(seed)
        if reduction not in ("sum", "mean", "prod", "max", "min", None):
            raise ValueError(f"reduction must be one of 'sum', 'mean', 'prod', 'max', 'min' or None, not {reduction!r}")
        if precision not in ("f32", "bf16"):
            raise ValueError(f"precision must be 'f32' or 'bf16', not {precision!r}")
        self.precision = precision
        self.seed, self.row_offset, self.reduction = int(seed), int(row_offset), reduction
        self.clip_actions, self.clip_log_std = bool(clip_actions), bool(clip_log_std)
        self.min_log_std, self.max_log_std = float(min_log_std), float(max_log_std)
        self.action_low, self.action_high = float(action_low), float(action_high)
        self.engine, self.device = engine, device
        self.num_sparse, self.num_dense = num_sparse, num_dense
        self.num_proprioception = num_observations - num_sparse - num_dense                # model.py:174
        mk = lambda i, o, act: Layer(i, o, act, device, g)
        self.encoder0, self.encoder1 = [], []
        i = num_sparse
        for f in encoder_features:
            self.encoder0.append(mk(i, f, activation_function)); i = f
        i = num_dense
        for f in encoder_features:
            self.encoder1.append(mk(i, f, activation_function)); i = f
        self.network = []
        i = self.num_proprioception + 2 * encoder_features[-1]                             # model.py:178
        for f in mlp_features:
            self.network.append(mk(i, f, activation_function)); i = f
        self.network.append(mk(i, num_outputs, head_activation))                          # :181-182 / :226
        # :183 — only the stochastic actor owns a log-std parameter (DeterministicHeightmap has none, :197-241)
        self.log_std_parameter = torch.zeros(num_outputs, device=device) if head_activation == "tanh" else None
        self._bufs, self._plans = {}, {}
        self._fwd = {}                         # rows -> (states, ForwardPlan) of the last forward of that batch size (backward())
        # act()'s call counter, in device memory so that a captured graph draws fresh noise on every replay: read by the head's kernel,
        # advanced by act() on the same stream right after it (eager and captured alike)
        self._act_counter = torch.zeros(1, dtype=torch.int64, device=device)
        self._last_rows = 0

    def _buf(self, key, rows, cols):
        b = self._bufs.get(key)
        if b is None or b.shape != (rows, cols):
            b = self._bufs[key] = torch.empty(rows, cols, device=self.device)
        return b

    def _precision(self, precision, fused):
        precision = self.precision if precision is None else precision
        if precision not in ("f32", "bf16"):
            raise ValueError(f"precision must be 'f32' or 'bf16', not {precision!r}")
        if precision == "bf16" and fused is not None and not fused:
            raise ValueError("precision='bf16' runs the fused chain kernels only: fused=False has no bf16 layer kernels")
        return precision

    @staticmethod
    def _kw(precision):
        """The engine calls' precision argument: named only where it is not their default."""
        return {} if precision == "f32" else {"precision": precision}

    def _plan(self, rows, fused, precision="f32"):
        """The ForwardPlan of a batch of ``rows`` rows, asked of the library's route queries once and kept like the buffers: a chain is one
        kernel where rover_mlp_chain_route names one; the encoders take chain_pair_forward at the batch sizes where the library runs two
        encoders of these widths side by side ("pair(...)", rover_step.h).  That is asked with inputs long enough to split along k: at
        those batch sizes shorter slices take the same call, which then runs them one after the other and copies the columns itself.
        ``precision="bf16"``: all three chains as bf16 chain kernels (rover_mlp_chain_route_bf16 must name one for each), never a pair."""
        plan = self._plans.get((rows, fused, precision))
        if plan is None and precision == "bf16":
            # all three chains in bf16 or none: no silent mix of precisions (an empty heightmap slice is a chain too: K0 = 0)
            for name, layers in (("encoder0", self.encoder0), ("encoder1", self.encoder1), ("network", self.network)):
                if self.engine.chain_route(rows, *self.engine.chain_shape(layers), precision="bf16") is None:
                    raise ValueError(f"precision='bf16': {name} {self.engine.chain_shape(layers)} fits no bf16 chain kernel "
                                     "(rover_mlp_chain_route_bf16 refuses it; the built tile shapes are listed in rover_step.h)")
            plan = self._plans[(rows, fused, precision)] = ForwardPlan(False, True, True, True)
        if plan is None:
            eng = self.engine
            chain = lambda layers: bool(fused and eng.chain_route(rows, *eng.chain_shape(layers)) is not None)
            long_enc = [(1 << 20,) + eng.chain_shape(enc)[1:] for enc in (self.encoder0, self.encoder1)]       # (k0, widths, activations)
            pair = bool(fused and self.num_sparse > 0 and self.num_dense > 0 and (eng.chain_pair_route(rows, *long_enc) or "").startswith("pair("))
            plan = self._plans[(rows, fused, precision)] = ForwardPlan(pair, chain(self.encoder0), chain(self.encoder1), chain(self.network))
        return plan

    def compute(self, states, fused=None, precision=None):
        """model.py:185-195 / :231-241.  ``states`` [E, num_observations] float32 (may be the task's obs_buf itself).
        ``fused`` (default): each encoder and the MLP + head run as ONE kernel each (``rover_mlp_chain_forward``: activations stay in
        registers) when the library has a chain kernel for their widths; ``fused=False``: one ``rover_linear_forward`` launch per layer.
        ``precision`` (default: the net's): "bf16" runs all three chains with bf16 operands and f32 accumulation — ValueError if one of
        them fits no bf16 chain kernel, or with ``fused=False``."""
        precision = self._precision(precision, fused)
        cat, mlp_fused = self._encode(states, fused, precision)
        if mlp_fused:
            e = states.shape[0]
            return self.engine.chain_forward(cat, self.network, self._buf(("mlp", len(self.network) - 1), e, self.network[-1].weight.shape[0]),
                                             **self._kw(precision))
        return self._mlp_layers(cat)

    def _mlp_layers(self, cat):
        x = cat
        for li, layer in enumerate(self.network):
            x = self.engine.linear_forward(x, layer.weight, layer.bias, layer.activation, self._buf(("mlp", li), cat.shape[0], layer.weight.shape[0]))
        return x

    def _encode(self, states, fused, precision="f32"):
        """Both encoders and the proprioception columns into the concat buffer -> (cat, whether the MLP + head runs as one chain kernel).
        The proprioception columns are copied as f32 in either precision (the bf16 MLP chain rounds them as it reads them)."""
        e = states.shape[0]
        plan = self._plan(e, fused is None or bool(fused), precision)
        self._fwd[e] = (states, plan)
        p, ns, nd = self.num_proprioception, self.num_sparse, self.num_dense
        ef = self.encoder0[-1].weight.shape[0]
        cat = self._buf("cat", e, p + 2 * ef)
        if plan.pair:
            # small batches: both encoders and the proprioception copy side by side, then the MLP + head: 3 launches instead of 6
            self.engine.chain_pair_forward(states[:, p:p + ns], self.encoder0, cat[:, p:p + ef],
                                           states[:, p + ns:p + ns + nd], self.encoder1, cat[:, p + ef:p + 2 * ef],
                                           copy_src=states, copy_dst=cat, copy_cols=p)
            return cat, plan.mlp
        cat[:, 0:p] = states[:, 0:p]
        for enc, as_chain, lo, n, col in ((self.encoder0, plan.enc0, p, ns, p), (self.encoder1, plan.enc1, p + ns, nd, p + ef)):
            x = states[:, lo:lo + n]
            if as_chain:
                self.engine.chain_forward(x, enc, cat[:, col:col + ef], **self._kw(precision))
                continue
            for li, layer in enumerate(enc):
                last = li == len(enc) - 1
                out = cat[:, col:col + ef] if last else self._buf(("enc", col, li), e, layer.weight.shape[0])
                x = self.engine.linear_forward(x, layer.weight, layer.bias, layer.activation, out)
        return cat, plan.mlp

    # ---- skrl's mixins: GaussianMixin.act (actor), DeterministicMixin.act (critic) --------------------------------
    def act(self, states, taken_actions=None, deterministic=False, step=None, role="", fused=None, precision=None):
        """Actor: -> (actions [E, A], log_prob [E, 1] ([E, A] with reduction None), {"mean_actions": mean [E, A]}) with
        mean = compute(states), actions = mean + exp(log_std') eps (``deterministic``: mean), clamped to the action bounds only with
        ``clip_actions``, and log_prob that of ``taken_actions`` if given, else of the returned actions.  Also skrl's calling shape:
        ``act({"states": s, "taken_actions": a}, role="policy")``.  ``actions`` and ``log_prob`` are new tensors; ``mean_actions`` is
        compute()'s buffer (overwritten by the next compute() / act() of the same batch size).
        The noise of row r is keyed by (seed, call counter, row_offset + r): it does not depend on the batch size or the kernel.  The
        counter lives on the device and advances by one per act() — not when ``taken_actions`` is given (an evaluation of old actions)
        and not when ``step`` (an explicit counter value) is passed.  Capturing act() in a graph: warm it up once first; every replay
        then reads and advances the same counter an eager call does.
        ``precision`` (default: the net's) as in compute(): with "bf16" the mean comes from the bf16 chains and the head is the f32
        head on it — log_prob is exactly that of the policy that acted.
        Critic (no log-std parameter): -> (value, None, {})."""
        if isinstance(states, dict):
            inputs = states
            states, taken_actions = inputs["states"], inputs.get("taken_actions", taken_actions)
        if self.log_std_parameter is None:
            value = self.compute(states, fused, precision)
            if self.clip_actions:
                value = torch.clamp(value, self.action_low, self.action_high)
            return value, None, {}
        e, a = states.shape[0], self.network[-1].weight.shape[0]
        self._last_rows = e
        actions = torch.empty(e, a, device=self.device)
        log_prob = torch.empty(e, a if self.reduction is None else 1, device=self.device)
        mean = self._buf(("mlp", len(self.network) - 1), e, a)
        head = dict(taken_actions=taken_actions, reduction=self.reduction, deterministic=deterministic, seed=self.seed, row_offset=self.row_offset,
                    clip_log_std=self.clip_log_std, min_log_std=self.min_log_std, max_log_std=self.max_log_std, clip_actions=self.clip_actions,
                    low=self.action_low, high=self.action_high)
        if step is None:
            head["step_dev"] = self._act_counter
        else:
            head["step"] = int(step)
        precision = self._precision(precision, fused)
        cat, mlp_fused = self._encode(states, fused, precision)
        if mlp_fused:
            self.engine.chain_act(cat, self.network, mean, self.log_std_parameter, actions, log_prob, **self._kw(precision), **head)
        else:
            self.engine.gaussian_head(self._mlp_layers(cat), self.log_std_parameter, actions, log_prob, **head)
        if step is None and taken_actions is None:
            self._act_counter += 1
        return actions, log_prob, {"mean_actions": mean}

    def _clipped_log_std(self):
        ls = self.log_std_parameter
        return torch.clamp(ls, self.min_log_std, self.max_log_std) if self.clip_log_std else ls

    def get_log_std(self, role=""):
        """log_std' (clamped if ``clip_log_std``) as [rows of the last act(), A]."""
        return self._clipped_log_std().expand(max(self._last_rows, 1), -1)

    def get_entropy(self, role=""):
        """Normal's entropy per component, 0.5 + 0.5 log(2 pi) + log_std', as [rows of the last act(), A]."""
        return 0.5 + 0.5 * math.log(2.0 * math.pi) + self.get_log_std(role)

    # ---- training: parameters and the layer-by-layer backward ---------------------------------------------------
    def parameters(self):
        """The parameter tensors in ``state_dict()`` order (what ``torch.optim.Adam`` and ``clip_grad_norm_`` take)."""
        return list(self.state_dict().values())

    @staticmethod
    def _grad_of(p):
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        return p.grad

    def backward(self, d_out):
        """``d_out`` [E, num_outputs]: the loss gradient at compute()'s output of the last forward of E rows, which must have run with
        ``fused=False`` (it leaves every layer's output in the net's buffers).  Walks the MLP and both encoders back with
        ``Engine.linear_backward`` and overwrites ``weight.grad`` / ``bias.grad`` of every layer (kept tensors, created on first use).
        The encoders' dy are the column slices of d cat, read in place; the first encoder layers compute no dx.  The actor's
        ``log_std_parameter.grad`` is ``Engine.ppo_loss``'s d_log_std, not written here.  Enqueues only."""
        e = d_out.shape[0]
        if e not in self._fwd:
            raise RuntimeError(f"backward: no forward of {e} rows has run")
        states, plan = self._fwd[e]
        if plan.pair or plan.enc0 or plan.enc1 or plan.mlp:
            raise RuntimeError(f"backward: the last forward of {e} rows ran fused chain kernels, which keep no layer outputs: run it with fused=False")
        eng, g = self.engine, self._grad_of
        p, ns, nd = self.num_proprioception, self.num_sparse, self.num_dense
        ef = self.encoder0[-1].weight.shape[0]
        cat = self._bufs["cat"]
        dy = d_out
        for li in range(len(self.network) - 1, -1, -1):
            layer = self.network[li]
            x = cat if li == 0 else self._bufs[("mlp", li - 1)]
            dx = self._buf(("d_mlp", li), e, x.shape[1])
            eng.linear_backward(x, self._bufs[("mlp", li)], dy, layer.weight, layer.activation, dx=dx, dweight=g(layer.weight), dbias=g(layer.bias))
            dy = dx
        d_cat = dy
        for enc, lo, n, col in ((self.encoder0, p, ns, p), (self.encoder1, p + ns, nd, p + ef)):
            dy = d_cat[:, col:col + ef]
            for li in range(len(enc) - 1, -1, -1):
                layer = enc[li]
                y = cat[:, col:col + ef] if li == len(enc) - 1 else self._bufs[("enc", col, li)]
                x = states[:, lo:lo + n] if li == 0 else self._bufs[("enc", col, li - 1)]
                dx = None if li == 0 else self._buf(("d_enc", col, li), e, x.shape[1])
                eng.linear_backward(x, y, dy, layer.weight, layer.activation, dx=dx, dweight=g(layer.weight), dbias=g(layer.bias))
                dy = dx

    # ---- interop with the reference's nn.Module parameter names --------------------------------------------
    def state_dict(self):
        sd = {} if self.log_std_parameter is None else {"log_std_parameter": self.log_std_parameter}
        for name, enc in (("encoder0", self.encoder0), ("encoder1", self.encoder1)):
            for i, l in enumerate(enc):
                sd[f"{name}.encoder.{i}.layer.0.weight"] = l.weight
                sd[f"{name}.encoder.{i}.layer.0.bias"] = l.bias
        for i, l in enumerate(self.network[:-1]):
            sd[f"network.{i}.layer.0.weight"] = l.weight
            sd[f"network.{i}.layer.0.bias"] = l.bias
        k = len(self.network) - 1
        sd[f"network.{k}.weight"] = self.network[-1].weight
        sd[f"network.{k}.bias"] = self.network[-1].bias
        return sd

    def load_state_dict(self, sd):
        for k, v in self.state_dict().items():
            if k in sd:
                v.copy_(sd[k].to(self.device))


def StochasticActorHeightmap(engine, task, **kw):
    hm = task.Camera.heightmap
    kw.setdefault("row_offset", int(engine.cfg.env_offset))       # a shard's actor draws its slice of the global batch's noise
    return HeightmapNet(engine, task.num_observations, hm.get_num_sparse_vector(), hm.get_num_dense_vector(), task.num_actions,
                        "tanh", device=task.device, **kw)


def DeterministicHeightmap(engine, task, **kw):
    hm = task.Camera.heightmap
    return HeightmapNet(engine, task.num_observations, hm.get_num_sparse_vector(), hm.get_num_dense_vector(), 1, None,
                        device=task.device, **kw)
