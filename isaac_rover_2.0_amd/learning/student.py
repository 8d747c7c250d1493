"""The recurrent student policy of the reference's learning-by-cheating scheme — forward pass on the MI355X.

Mirrors ``omniisaacgymenvs/tasks/utils/learning_by_cheating/student_model.py`` (``Student``: two ``Encoder``s, ``Belief_Encoder`` = a
2-layer ``nn.GRU`` + the gated ``gb`` / ``ga`` branches, ``Belief_Decoder``, ``MLP`` with a Tanh head) and ``student_loader.py``
(``act``: one time step per env step with a carried hidden state; ``cfg_fn``: the widths in ``DEFAULT_CFG``).

The GRU is the one new hot path: each layer of a time step is ONE ``rover_gru_cell`` launch (f32 MFMA, gates in the epilogue), the
gates ``x_b + l_e * sigmoid(x_a)`` and ``decoded + e * sigmoid(gate)`` one ``rover_gated_sum`` each.  Everything else is ``Layer`` chains
the library already runs; whether a chain is one kernel or one launch per layer is asked of the library (``Engine.chain_route``,
``Engine.linear_route``), as ``HeightmapNet._plan`` does — this file holds no width or row limit.

Things the reference does that are kept as they are:
  * obs is sliced as ``[proprioceptive | ... | sparse | dense]``: the heightmap slices are taken from the END of the row (:208-210);
  * ``ga``'s last ``Layer`` applies its LeakyReLU BEFORE the ``nn.Sigmoid`` (:63-68);
  * ``Belief_Decoder`` always uses LeakyReLU (its cfg's ``activation_function`` is not read, :95-96);
  * ``Student.forward`` hands the decoder the GRU's output SEQUENCE ``out [B, T, H]``, of which the decoder takes ``out[-1]`` — the LAST
    BATCH ROW's sequence (:121-123,227) — so ``estimated[b, t] = decoded(out[B-1, t]) + e[b, t] * sigmoid(gate(out[B-1, t]))``.

The hidden state lives in ``self.h [n_layers, E, H]`` at a fixed address.  A cell may not write over the state it reads (a tile of h'
needs whole rows of h), so ``act()`` writes the new state into a scratch tensor and copies it back on the device: the
same launches every call, capturable once after a warm-up.

``precision="bf16"`` (opt-in, inference only): every matrix product of ``act()`` / ``forward()`` on bf16 operands
with f32 accumulation — the encoders and the MLP on the bf16 chain kernels, the cells on ``rover_gru_cell_bf16``, the ``gb`` / ``ga``
branches, the decoder and its gate layer by layer on ``rover_linear_forward_bf16`` (each layer's f32 output is rounded by whoever reads
it: a chain's arithmetic).  ``rover_gated_sum``, the proprioceptive copy and ``self.h`` stay f32: the cell's blend ``z * h`` takes the
unrounded state, since a state rounded to 8 bits every step would drop every update below 2^-9 |h|.  A student never mixes precisions
(a chain or layer that fits no bf16 kernel is a ValueError naming it); training is f32 whatever the policy's precision.  Measured on
the MI355X at native width (obs 1 750, H = 300; EXPERIMENTS.md §20; µs per captured ``act()``, median, f32 against bf16): 406 / 321 at
512 envs, 660 / 321 at 4 096, 823 / 459 at 16 384, 2 501 / 1 066 at 65 536 — bf16 is faster at every size measured, there is no
crossover in that range (at 512 envs its ``Layer`` and encoder launches are slower than the f32 ones and the cells pay for them), and
its actions are within 2e-4 of the f32 ones.  The default stays f32: a policy's arithmetic is the user's choice.

Training: ``forward_train()`` is ``forward()`` run so that a backward can follow — time-major inside, every layer
unfused so that its output exists, the GRU cells through ``rover_gru_cell_train`` (which also stores the gates), everything that is
not recurrent ONCE over all T·B rows — and ``backward()`` is back-propagation through time written out on ``rover_gru_cell_backward``,
``rover_linear_dgrad``, ``rover_gated_sum_backward`` and ``rover_linear_backward``; it leaves every parameter's gradient in its
``.grad``.  The distillation loss and the update loop live in ``learning/distill.py``.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch

from .model import Layer

# student_loader.cfg_fn (:29-62), the keys the model reads
DEFAULT_CFG = {
    "encoder": {"activation_function": "leakyrelu", "encoder_features": [80, 60]},
    "belief_encoder": {"hidden_dim": 300, "n_layers": 2, "activation_function": "leakyrelu", "gb_features": [128, 128, 120],
                       "ga_features": [128, 128, 120]},
    "belief_decoder": {"activation_function": "leakyrelu", "gate_features": [128, 256, 512], "decoder_features": [128, 256, 512]},
    "mlp": {"activation_function": "leakyrelu", "network_features": [256, 160, 128]},
}
INFO_KEYS = ("proprioceptive", "sparse", "dense", "actions")


def _info_of(info_or_task):
    """``info``: the reference's dataset header (a mapping with INFO_KEYS), or a task (RoverTask: widths from its heightmap)."""
    if hasattr(info_or_task, "keys"):
        for k in INFO_KEYS:
            if k not in info_or_task:
                raise KeyError(f"StudentPolicy: info has no '{k}' (needs {', '.join(INFO_KEYS)})")
        info = {k: int(info_or_task[k]) for k in INFO_KEYS}
    else:
        t, hm = info_or_task, info_or_task.Camera.heightmap
        ns, nd = hm.get_num_sparse_vector(), hm.get_num_dense_vector()
        info = {"proprioceptive": t.num_observations - ns - nd, "sparse": ns, "dense": nd, "actions": t.num_actions}
    for k, v in info.items():
        if v < 0 or (k == "actions" and v < 1):
            raise ValueError(f"StudentPolicy: info['{k}'] = {v}")
    return info


def _cfg_of(cfg):
    for sec, keys in (("encoder", ("encoder_features",)), ("belief_encoder", ("hidden_dim", "n_layers", "gb_features", "ga_features")),
                      ("belief_decoder", ("gate_features", "decoder_features")), ("mlp", ("network_features",))):
        if sec not in cfg:
            raise KeyError(f"StudentPolicy: cfg has no section '{sec}'")
        for k in keys:
            if k not in cfg[sec]:
                raise KeyError(f"StudentPolicy: cfg['{sec}'] has no '{k}'")
    be = cfg["belief_encoder"]
    ef, gb, ga = list(cfg["encoder"]["encoder_features"]), list(be["gb_features"]), list(be["ga_features"])
    if not ef or not gb or not ga or int(be["n_layers"]) < 1 or int(be["hidden_dim"]) < 1:
        raise ValueError("StudentPolicy: cfg needs encoder_features, gb_features, ga_features, n_layers >= 1 and hidden_dim >= 1")
    # belief = x_b + l_e * x_a (student_model.py:83-85): the three widths are one
    if not (gb[-1] == ga[-1] == 2 * ef[-1]):
        raise ValueError(f"StudentPolicy: gb_features[-1] = {gb[-1]} and ga_features[-1] = {ga[-1]} must equal 2 * encoder_features[-1] = {2 * ef[-1]}")
    return cfg


def param_shapes(info, cfg=DEFAULT_CFG):
    """name -> shape of every parameter of the reference's ``Student(info, cfg)``, in its ``state_dict()`` order.  Pure."""
    info, cfg = _info_of(info), _cfg_of(cfg)
    p, ex = info["proprioceptive"], info["sparse"] + info["dense"]
    be, sd = cfg["belief_encoder"], OrderedDict()

    def layers(prefix, k, widths):
        for i, n in enumerate(widths):
            sd[f"{prefix}.{i}.layer.0.weight"], sd[f"{prefix}.{i}.layer.0.bias"] = (n, k), (n,)
            k = n
        return k

    ef = list(cfg["encoder"]["encoder_features"])
    layers("encoder1.encoder", info["sparse"], ef)
    layers("encoder2.encoder", info["dense"], ef)
    hd, k = int(be["hidden_dim"]), p + 2 * ef[-1]
    for l in range(int(be["n_layers"])):
        sd[f"belief_encoder.gru.weight_ih_l{l}"], sd[f"belief_encoder.gru.weight_hh_l{l}"] = (3 * hd, k), (3 * hd, hd)
        sd[f"belief_encoder.gru.bias_ih_l{l}"], sd[f"belief_encoder.gru.bias_hh_l{l}"] = (3 * hd,), (3 * hd,)
        k = hd
    layers("belief_encoder.gb", hd, list(be["gb_features"]))
    layers("belief_encoder.ga", hd, list(be["ga_features"]))
    layers("belief_decoder.gate_encoder", hd, list(cfg["belief_decoder"]["gate_features"]) + [ex])      # Belief_Decoder appends (:102-103)
    layers("belief_decoder.decoder", hd, list(cfg["belief_decoder"]["decoder_features"]) + [ex])
    sd["MLP.log_std_parameter"] = (info["actions"],)
    nf = list(cfg["mlp"]["network_features"])
    k = layers("MLP.network", p + list(be["gb_features"])[-1], nf)
    sd[f"MLP.network.{len(nf)}.weight"], sd[f"MLP.network.{len(nf)}.bias"] = (info["actions"], k), (info["actions"],)
    return sd


class StudentPolicy:
    """``Student`` + ``student_loader``: plain tensors under the reference's parameter names, ``act()`` per env step, ``forward()`` per sequence."""

    def __init__(self, engine, info_or_task, cfg=DEFAULT_CFG, device="cuda:0", seed=0, precision="f32"):
        """``precision``: "f32" (default) or "bf16" — what act() / forward() run when their own ``precision`` argument is None (module
        docstring).  The parameters, ``self.h`` and training are f32 either way."""
        self.precision = self._precision_of(precision)
        self.info, self.cfg = _info_of(info_or_task), _cfg_of(cfg)
        self.engine, self.device = engine, device
        g = torch.Generator().manual_seed(seed)
        shapes = param_shapes(self.info, cfg)
        be = cfg["belief_encoder"]
        self.hidden_dim, self.n_layers = int(be["hidden_dim"]), int(be["n_layers"])
        self._params = OrderedDict()

        def chain(prefix, act, head=None):
            """the Layers named ``prefix.i.layer.0.*`` (and the bare ``prefix.i.*`` head, activation ``head``)"""
            out, i = [], 0
            while f"{prefix}.{i}.layer.0.weight" in shapes or f"{prefix}.{i}.weight" in shapes:
                plain = f"{prefix}.{i}.weight" in shapes
                stem = f"{prefix}.{i}" if plain else f"{prefix}.{i}.layer.0"
                n, k = shapes[stem + ".weight"]
                layer = Layer(k, n, head if plain else act, device, g)
                self._params[stem + ".weight"], self._params[stem + ".bias"] = layer.weight, layer.bias
                out.append(layer)
                i += 1
            return out

        self.encoder1 = chain("encoder1.encoder", cfg["encoder"].get("activation_function", "leakyrelu"))
        self.encoder2 = chain("encoder2.encoder", cfg["encoder"].get("activation_function", "leakyrelu"))
        bound = 1.0 / math.sqrt(self.hidden_dim)                     # nn.GRU.reset_parameters
        self.gru = []
        for l in range(self.n_layers):
            ws = []
            for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                name = f"belief_encoder.gru.{nm}_l{l}"
                t = (torch.rand(*shapes[name], generator=g) * 2 - 1).mul_(bound).to(device)
                self._params[name] = t
                ws.append(t)
            self.gru.append(tuple(ws))
        self.gb = chain("belief_encoder.gb", be.get("activation_function", "leakyrelu"))
        self.ga = chain("belief_encoder.ga", be.get("activation_function", "leakyrelu"))
        self.gate_encoder = chain("belief_decoder.gate_encoder", "leakyrelu")
        self.decoder = chain("belief_decoder.decoder", "leakyrelu")
        self.log_std_parameter = self._params["MLP.log_std_parameter"] = torch.zeros(self.info["actions"], device=device)
        self.network = chain("MLP.network", cfg["mlp"].get("activation_function", "leakyrelu"), head="tanh")
        self._params = OrderedDict((k, self._params[k]) for k in shapes)          # the reference's order
        self.h = None
        self._bufs, self._plans, self._chunks = {}, {}, {}
        self._saved = None                     # what the last forward_train() kept for backward()

    # ---- interop with the reference's nn.Module parameter names --------------------------------------------
    def state_dict(self):
        return OrderedDict(self._params)

    def load_state_dict(self, sd):
        """Every parameter from ``sd`` (a checkpoint's ``['state_dict']``); a missing key is a KeyError, a wrong shape a ValueError, each naming the key."""
        for k, v in self._params.items():
            if k not in sd:
                raise KeyError(f"StudentPolicy.load_state_dict: missing key '{k}'")
            if tuple(sd[k].shape) != tuple(v.shape):
                raise ValueError(f"StudentPolicy.load_state_dict: '{k}' has shape {tuple(sd[k].shape)}, expected {tuple(v.shape)}")
        for k, v in self._params.items():
            v.copy_(torch.as_tensor(sd[k]).to(device=self.device, dtype=torch.float32))

    def init_hidden(self, num_envs):
        """Zeroes ``self.h [n_layers, E, H]`` (Belief_Encoder.init_hidden, :89-92); the same tensor is kept while E stays the same."""
        if self.h is None or self.h.shape[1] != num_envs:
            self.h = torch.zeros(self.n_layers, num_envs, self.hidden_dim, device=self.device)
            self._h_new = torch.empty_like(self.h)
        else:
            self.h.zero_()
        return self.h

    # ---- the forward ------------------------------------------------------------------------------------------
    @staticmethod
    def _precision_of(precision):
        if precision not in ("f32", "bf16"):
            raise ValueError(f"StudentPolicy: precision must be 'f32' or 'bf16', not {precision!r}")
        return precision

    @staticmethod
    def _kw(precision):
        """The engine calls' precision argument: named only where it is not their default."""
        return {} if precision == "f32" else {"precision": precision}

    def _buf(self, key, rows, cols):
        b = self._bufs.get(key)
        if b is None or b.shape != (rows, cols):
            b = self._bufs[key] = torch.empty(rows, cols, device=self.device)
        return b

    def _linear(self, x, layer, out, precision="f32", name="layer"):
        """One Layer; a layer wider than one linear_forward takes (the decoder's) runs as column blocks of the width the library accepts
        (asked per precision).  bf16: a layer of which not even one column fits is a ValueError naming it — never an f32 layer instead."""
        m, k, n = x.shape[0], x.shape[1], layer.weight.shape[0]
        kw = self._kw(precision)
        ck = (m, k, n) if precision == "f32" else (m, k, n, precision)
        c = self._chunks.get(ck)
        if c is None:
            c = n
            while c > 1 and self.engine.linear_route(m, k, c, **kw) is None:
                c = (c + 1) // 2
            if precision != "f32" and self.engine.linear_route(m, k, c, **kw) is None:
                raise ValueError(f"StudentPolicy: precision='{precision}': {name} [{m}, {k}] -> {n} fits no {precision} layer kernel")
            self._chunks[ck] = c
        for lo in range(0, n, c):
            hi = min(n, lo + c)
            self.engine.linear_forward(x, layer.weight[lo:hi], layer.bias[lo:hi], layer.activation, out[:, lo:hi], **kw)
        return out

    def _run(self, key, x, layers, out, precision="f32"):
        """``layers`` over x into ``out``: one chain kernel where the library names one for these widths (and this precision), else layer
        by layer.  Either way every product of a bf16 run is a bf16 kernel's: a layer's f32 output is rounded by whoever reads it."""
        m, eng, kw = x.shape[0], self.engine, self._kw(precision)
        pk = (key, m) if precision == "f32" else (key, m, precision)
        fused = self._plans.get(pk)
        if fused is None:
            fused = self._plans[pk] = eng.chain_route(m, *eng.chain_shape(layers), **kw) is not None
        if fused:
            return eng.chain_forward(x, layers, out, **kw)
        for i, layer in enumerate(layers):
            last = i == len(layers) - 1
            x = self._linear(x, layer, out if last else self._buf((key, i), m, layer.weight.shape[0]), precision, f"{key}[{i}]")
        return out

    def _step(self, obs, h_in, h_out, reset, actions, estimated, precision="f32"):
        """One time step: obs [E, F] (rows at any stride), h_in / h_out lists of [E, H] per layer -> actions [E, A] (and estimated).
        ``precision="bf16"``: every matrix product in bf16 (chains, cells, layers); the copies, the gated sums and h stay f32."""
        eng, e, f = self.engine, obs.shape[0], obs.shape[1]
        if precision != "f32" and (("cell", e, precision) not in self._plans):          # a student never mixes precisions
            if eng.gru_cell_route(e, 0, self.hidden_dim, precision=precision) is None:
                raise ValueError(f"StudentPolicy: precision='{precision}': the GRU cell [{e}, {self.hidden_dim}] fits no {precision} cell kernel")
            self._plans[("cell", e, precision)] = True
        run = lambda key, x, layers, out: self._run(key, x, layers, out, precision)
        p, ns, nd = self.info["proprioceptive"], self.info["sparse"], self.info["dense"]
        if f < p + ns + nd:
            raise ValueError(f"StudentPolicy: obs has {f} columns, needs proprioceptive + sparse + dense = {p + ns + nd}")
        ef = self.encoder1[-1].weight.shape[0]
        cat = self._buf("cat", e, p + 2 * ef)                        # [p | e_l1 | e_l2]: the GRU's input (:75,222)
        mlp_in = self._buf("mlp_in", e, p + 2 * ef)                  # [p | belief] (:159)
        cat[:, :p] = obs[:, :p]
        mlp_in[:, :p] = obs[:, :p]
        run("enc1", obs[:, f - ns - nd:f - nd], self.encoder1, cat[:, p:p + ef])
        run("enc2", obs[:, f - nd:], self.encoder2, cat[:, p + ef:p + 2 * ef])
        x = cat
        for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(self.gru):
            x = eng.gru_cell(x, h_in[l], w_ih, w_hh, b_ih, b_hh, h_out[l], reset_mask=reset, **self._kw(precision))
        top = x
        x_b = run("gb", top, self.gb, self._buf("x_b", e, 2 * ef))
        x_a = run("ga", top, self.ga, self._buf("x_a", e, 2 * ef))
        eng.gated_sum(x_b, cat[:, p:], x_a, mlp_in[:, p:])           # belief = x_b + l_e * sigmoid(x_a) (:79-85)
        run("mlp", mlp_in, self.network, actions)
        if estimated is not None:
            last, ex = top[e - 1:e], ns + nd                         # the decoder reads the LAST batch row's output (module docstring)
            gate = run("gate", last, self.gate_encoder, self._buf("gate", 1, ex))
            dec = run("dec", last, self.decoder, self._buf("decoded", 1, ex))
            eng.gated_sum(dec.expand(e, ex), obs[:, f - ex:], gate.expand(e, ex), estimated)
        return actions

    def act(self, obs, reset=None, reconstruct=False, precision=None):
        """student_loader.act (:21-24): obs [E, F] -> actions [E, A], the Tanh mean (no sampling); advances ``self.h`` in place (same
        address after every call).  ``reset``: optional [E] bool / uint8 device tensor (e.g. the step's done): marked rows start from a
        zero hidden state — an addition, the reference never resets.  ``reconstruct=True``: -> (actions, estimated [E, sparse + dense]).
        Both are buffers of this object, overwritten by the next call of the same E.  Capturable in a graph after one warm-up call.
        ``precision`` (default: the policy's): "bf16" runs every matrix product of the step in bf16; ``self.h`` stays f32."""
        precision = self.precision if precision is None else self._precision_of(precision)
        e = obs.shape[0]
        if self.h is None or self.h.shape[1] != e:
            self.init_hidden(e)
        actions = self._buf("actions", e, self.info["actions"])
        est = self._buf("estimated", e, self.info["sparse"] + self.info["dense"]) if reconstruct else None
        self._step(obs, list(self.h), list(self._h_new), reset, actions, est, precision)
        self.h.copy_(self._h_new)
        return (actions, est) if reconstruct else actions

    def forward(self, x, h, precision=None):
        """Student.forward (:199-248): x [B, T, F] (batch first), h [n_layers, B, H] -> (actions [B, T, A], estimated [B, T, S + D],
        h [n_layers, B, H]) as a loop of T cell steps; time step t is the row view x[:, t] (row stride T F): no transpose copy.
        ``precision`` as in act()."""
        precision = self.precision if precision is None else self._precision_of(precision)
        b, t_len = x.shape[0], x.shape[1]
        actions = torch.empty(b, t_len, self.info["actions"], device=self.device)
        est = torch.empty(b, t_len, self.info["sparse"] + self.info["dense"], device=self.device)
        cur, nxt = h.to(torch.float32).clone(), torch.empty(self.n_layers, b, self.hidden_dim, device=self.device)
        for t in range(t_len):
            self._step(x[:, t], list(cur), list(nxt), None, actions[:, t], est[:, t], precision)
            cur, nxt = nxt, cur
        return actions, est, cur

    # ---- training: the forward that keeps what the backward needs, and back-propagation through time ---------------------
    def parameters(self):
        """The trainable tensors in ``state_dict()`` order: every parameter but ``MLP.log_std_parameter``, which takes no part in
        ``forward()`` (the student's action is the Tanh mean) and so never has a gradient."""
        return [v for k, v in self._params.items() if k != "MLP.log_std_parameter"]

    @staticmethod
    def _grad_of(p):
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        return p.grad

    def _run_train(self, key, x, layers, out):
        """``layers`` over x into ``out``, layer by layer; the input and every layer's output are kept for the backward."""
        m, ys = x.shape[0], [x]
        for i, layer in enumerate(layers):
            last = i == len(layers) - 1
            ys.append(self._linear(ys[-1], layer, out if last else self._buf(("t", key, i), m, layer.weight.shape[0])))
        self._saved[key] = ys
        return out

    def forward_train(self, x, h0, reset=None):
        """``forward()`` with a backward to follow: x [B, T, F], h0 [n_layers, B, H], ``reset`` optional [B, T] bool / uint8 (a marked
        row starts step t from a zero hidden state) -> (actions [B, T, A], estimated [B, T, S + D], h [n_layers, B, H]).  The first two
        are views of buffers of this object, overwritten by the next call."""
        if x is None or x.dim() != 3:
            raise ValueError("StudentPolicy.forward_train: x must be [B, T, F]")
        b, t_len, f = x.shape
        p, ns, nd, hd = self.info["proprioceptive"], self.info["sparse"], self.info["dense"], self.hidden_dim
        if f < p + ns + nd:
            raise ValueError(f"StudentPolicy.forward_train: x has {f} columns, needs proprioceptive + sparse + dense = {p + ns + nd}")
        if h0 is None or tuple(h0.shape) != (self.n_layers, b, hd):
            raise ValueError(f"StudentPolicy.forward_train: h0 must be [{self.n_layers}, {b}, {hd}]")
        if reset is not None and tuple(reset.shape) != (b, t_len):
            raise ValueError(f"StudentPolicy.forward_train: reset must be [{b}, {t_len}]")
        eng, rows, ex = self.engine, t_len * b, ns + nd
        ef = self.encoder1[-1].weight.shape[0]
        xt = self._buf(("t", "x"), rows, f)                          # time-major: row t B + b
        xt.view(t_len, b, f).copy_(x.transpose(0, 1))
        h0 = h0.to(torch.float32).contiguous()
        rs = None if reset is None else reset.to(torch.uint8).t().contiguous()
        self._saved = {"shape": (b, t_len, f), "x": xt, "h0": h0, "reset": rs}
        cat, mlp_in = self._buf(("t", "cat"), rows, p + 2 * ef), self._buf(("t", "mlp_in"), rows, p + 2 * ef)
        cat[:, :p] = xt[:, :p]
        mlp_in[:, :p] = xt[:, :p]
        self._run_train("enc1", xt[:, f - ex:f - nd], self.encoder1, cat[:, p:p + ef])
        self._run_train("enc2", xt[:, f - nd:], self.encoder2, cat[:, p + ef:p + 2 * ef])
        seq, outs, gates = cat.view(t_len, b, p + 2 * ef), [], []
        for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(self.gru):      # layer l runs all T steps before layer l + 1
            out = self._buf(("t", "out", l), rows, hd).view(t_len, b, hd)
            gt = self._buf(("t", "gates", l), rows, 4 * hd).view(t_len, b, 4 * hd)
            for t in range(t_len):
                eng.gru_cell_train(seq[t], h0[l] if t == 0 else out[t - 1], w_ih, w_hh, b_ih, b_hh, out[t], gt[t], reset_mask=None if rs is None else rs[t])
            outs.append(out)
            gates.append(gt)
            seq = out
        self._saved["out"], self._saved["gates"] = outs, gates
        top = seq.view(rows, hd)
        x_b = self._run_train("gb", top, self.gb, self._buf(("t", "x_b"), rows, 2 * ef))
        x_a = self._run_train("ga", top, self.ga, self._buf(("t", "x_a"), rows, 2 * ef))
        eng.gated_sum(x_b, cat[:, p:], x_a, mlp_in[:, p:])
        actions = self._run_train("mlp", mlp_in, self.network, self._buf(("t", "actions"), rows, self.info["actions"]))
        last = seq[:, b - 1]                                         # [T, H]: the last batch row's sequence (module docstring)
        gate = self._run_train("gate", last, self.gate_encoder, self._buf(("t", "gate"), t_len, ex))
        dec = self._run_train("dec", last, self.decoder, self._buf(("t", "decoded"), t_len, ex))
        est = self._buf(("t", "estimated"), rows, ex).view(t_len, b, ex)
        x3 = xt.view(t_len, b, f)
        for t in range(t_len):                                       # one shared row of dec / gate per time step (row stride 0)
            eng.gated_sum(dec[t:t + 1].expand(b, ex), x3[t][:, f - ex:], gate[t:t + 1].expand(b, ex), est[t])
        h = torch.stack([o[t_len - 1] for o in outs])
        return actions.view(t_len, b, -1).transpose(0, 1), est.transpose(0, 1), h

    def _wgrad(self, x, y, dy, weight, bias, activation):
        """dweight / dbias of one layer over all rows, in row blocks of the width linear_backward takes (a row block of [N][K] is contiguous)."""
        m, (n, k) = dy.shape[0], weight.shape
        c = self._chunks.get(("w", m, k, n))
        if c is None:
            c = n
            while c > 1 and self.engine.linear_backward_route(m, k, c, False) is None:
                c = (c + 1) // 2
            self._chunks[("w", m, k, n)] = c
        gw, gb = self._grad_of(weight), self._grad_of(bias)
        for lo in range(0, n, c):
            hi = min(n, lo + c)
            self.engine.linear_backward(x, None if y is None else y[:, lo:hi], dy[:, lo:hi], weight[lo:hi], activation, dweight=gw[lo:hi], dbias=gb[lo:hi])

    def _layer_backward(self, x, y, dy, layer, dx):
        """One Layer back: its weight.grad / bias.grad, and dx (None: not wanted).  One linear_backward where the library takes the widths,
        else row blocks for the weights and linear_dgrad for dx."""
        m, (n, k) = dy.shape[0], layer.weight.shape
        one = self._chunks.get(("b", m, k, n, dx is not None))
        if one is None:
            one = self._chunks[("b", m, k, n, dx is not None)] = self.engine.linear_backward_route(m, k, n, dx is not None) is not None
        if one:
            self.engine.linear_backward(x, y, dy, layer.weight, layer.activation, dx=dx, dweight=self._grad_of(layer.weight), dbias=self._grad_of(layer.bias))
            return dx
        self._wgrad(x, y, dy, layer.weight, layer.bias, layer.activation)
        if dx is not None:
            self.engine.linear_dgrad(y, dy, layer.weight, layer.activation, dx)
        return dx

    def _chain_backward(self, key, layers, dy, want_dx):
        """The chain ``key`` of the last forward_train back from dy at its output -> the gradient at its input (None unless ``want_dx``)."""
        ys = self._saved[key]
        for i in range(len(layers) - 1, -1, -1):
            x = ys[i]
            dx = self._buf(("t", "d", key, i), x.shape[0], x.shape[1]) if (i > 0 or want_dx) else None
            dy = self._layer_backward(x, ys[i + 1], dy, layers[i], dx)
        return dy

    def backward(self, d_actions, d_estimated=None):
        """Back-propagation through time from the loss gradients at the last ``forward_train()``'s outputs: d_actions [B, T, A],
        d_estimated [B, T, S + D] or None (no reconstruction term) -> dh0 [n_layers, B, H], the gradient at h0.  Overwrites ``.grad`` of
        every tensor of ``parameters()``.  Enqueues only."""
        sv = self._saved
        if not sv:
            raise RuntimeError("StudentPolicy.backward: no forward_train has run")
        b, t_len, f = sv["shape"]
        p, ns, nd, hd, na = self.info["proprioceptive"], self.info["sparse"], self.info["dense"], self.hidden_dim, self.info["actions"]
        ex, rows, eng = ns + nd, t_len * b, self.engine
        if d_actions is None or tuple(d_actions.shape) != (b, t_len, na):
            raise ValueError(f"StudentPolicy.backward: d_actions must be [{b}, {t_len}, {na}]")
        if d_estimated is not None and tuple(d_estimated.shape) != (b, t_len, ex):
            raise ValueError(f"StudentPolicy.backward: d_estimated must be [{b}, {t_len}, {ex}]")
        ef = self.encoder1[-1].weight.shape[0]
        xt, h0, rs, outs, gates = sv["x"], sv["h0"], sv["reset"], sv["out"], sv["gates"]
        cat = self._bufs[("t", "cat")]
        da = self._buf(("t", "d_actions"), rows, na)
        da.view(t_len, b, na).copy_(d_actions.transpose(0, 1))
        # 1. the MLP chain, 2. the belief gate: belief = x_b + l_e * sigmoid(x_a), so d x_b is d belief itself
        d_mlp_in = self._chain_backward("mlp", self.network, da, True)
        d_belief = d_mlp_in[:, p:]
        d_le, d_xa = self._buf(("t", "d_le"), rows, 2 * ef), self._buf(("t", "d_xa"), rows, 2 * ef)
        eng.gated_sum_backward(d_belief, cat[:, p:], sv["ga"][-1], d_mul=d_le, d_pre=d_xa)
        # 3. gb / ga back to the GRU's output
        d_top = self._buf(("t", "d_top"), rows, hd)
        torch.add(self._chain_backward("gb", self.gb, d_belief, True), self._chain_backward("ga", self.ga, d_xa, True), out=d_top)
        # 4. the decoder: estimated[t, b] = dec[t] + e[t, b] * sigmoid(gate[t]) with dec / gate of the LAST batch row's output
        if d_estimated is not None:
            de = self._buf(("t", "d_est"), rows, ex).view(t_len, b, ex)
            de.copy_(d_estimated.transpose(0, 1))
            d_pre = self._buf(("t", "d_gate_rows"), rows, ex).view(t_len, b, ex)
            gate, x3 = sv["gate"][-1], xt.view(t_len, b, f)
            for t in range(t_len):
                eng.gated_sum_backward(de[t], x3[t][:, f - ex:], gate[t:t + 1].expand(b, ex), d_pre=d_pre[t])
            d_dec, d_gate = de.sum(1), d_pre.sum(1)                    # one shared row per step: the batch rows' gradients add up
        else:                                                        # no reconstruction term: the decoder's gradients are zero
            d_dec = d_gate = torch.zeros(t_len, ex, device=self.device)
        d_last = self._chain_backward("dec", self.decoder, d_dec, True) + self._chain_backward("gate", self.gate_encoder, d_gate, True)
        d_top.view(t_len, b, hd)[:, b - 1] += d_last
        # 5. the GRU, each layer from the top: the cells step back through time, everything else runs once over all T B rows
        dh0 = torch.empty(self.n_layers, b, hd, device=self.device)
        dh_above = d_top.view(t_len, b, hd)
        for l in range(self.n_layers - 1, -1, -1):
            w_ih, w_hh, b_ih, b_hh = self.gru[l]
            k = w_ih.shape[1]
            dgi, dgh = self._buf(("t", "dgi", l), rows, 3 * hd), self._buf(("t", "dgh", l), rows, 3 * hd)
            dgi3, dgh3 = dgi.view(t_len, b, 3 * hd), dgh.view(t_len, b, 3 * hd)
            pong = (self._buf(("t", "dh", 0), b, hd), self._buf(("t", "dh", 1), b, hd))
            dh_next = None
            for t in range(t_len - 1, -1, -1):
                dh_in = dh0[l] if t == 0 else pong[t & 1]
                eng.gru_cell_backward(dh_above[t], dh_next, gates[l][t], h0[l] if t == 0 else outs[l][t - 1], w_hh, dgi3[t], dgh3[t], dh_in,
                                      reset_mask=None if rs is None else rs[t])
                dh_next = dh_in
            x_in = cat if l == 0 else outs[l - 1].view(rows, hd)
            dx = self._buf(("t", "d_gru_in", l), rows, k)
            if k > 0:
                eng.linear_dgrad(None, dgi, w_ih, None, dx)         # the next layer's dh_above for every t at once
            h_in = self._buf(("t", "h_in", l), rows, hd).view(t_len, b, hd)
            h_in[0] = h0[l]
            h_in[1:] = outs[l][:-1]
            if rs is not None:
                h_in.masked_fill_(rs.bool().unsqueeze(-1), 0.0)      # what the cells read: reset rows as zeros
            self._wgrad(x_in, None, dgi, w_ih, b_ih, None)
            self._wgrad(h_in.view(rows, hd), None, dgh, w_hh, b_hh, None)
            dh_above = dx.view(t_len, b, k)
        # 6. the encoders: l_e feeds the GRU's input and the belief gate
        d_le += dh_above.view(rows, -1)[:, p:]
        self._chain_backward("enc1", self.encoder1, d_le[:, :ef], False)
        self._chain_backward("enc2", self.encoder2, d_le[:, ef:], False)
        return dh0
