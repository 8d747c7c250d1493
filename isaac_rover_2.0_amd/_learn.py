"""The entry points of rover_capi_learn.cpp: linear layers, MLP chains, the Gaussian head, the GRU cell, the gated sum, GAE, the PPO loss and
the optimiser, with their route queries."""
import ctypes as C

import numpy as np
import torch

from ._abi import (_FAKE, GAE_NORMALIZE, GAE_NORMALIZE_GIVEN, GAE_RAW, REDUCTIONS, ChainDesc, EngineBase, GaeDesc, GaussHead, OptimChunk, OptimDesc,
                   OptimStepDesc, PpoLossDesc, RoverError, _host, _ptr, _route, _rows, host_call, route_query)


def philox4x32(counter, key):
    """rover_philox4x32: the four Philox4x32-10 words for ``counter`` (4 uint32) and ``key`` (2 uint32), computed on the host by the
    round function the kernels run.  No ctx, no device."""
    c = (C.c_uint32 * 4)(*[int(v) & 0xffffffff for v in counter])
    k = (C.c_uint32 * 2)(*[int(v) & 0xffffffff for v in key])
    out = (C.c_uint32 * 4)()
    host_call("rover_philox4x32", c, k, out)
    return tuple(int(v) for v in out)


def combine_moments(a, b):
    """The moments (count, mean, M2) of the union of two disjoint samples from their moments ``a`` and ``b`` (Chan's pairwise update: what
    shards do with the ``stats_out`` of their Engine.gae calls before they hand the result back as ``stats_in``).  Two float64 torch
    tensors of 3 elements: the same IEEE operations in the same order on their device (the same bits as the host helper), nothing
    synchronises; an empty side (count 0) leaves the other unchanged, as on the host.  Anything else (sequences, numpy arrays):
    rover_combine_moments on the host -> a float64 numpy array of 3."""
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):
        if a.dtype != torch.float64 or b.dtype != torch.float64 or a.numel() != 3 or b.numel() != 3:
            raise RoverError("combine_moments: expected two float64 tensors of 3 elements (count, mean, M2)")
        a, b = a.reshape(3), b.reshape(3)
        n = a[0] + b[0]
        d, f = b[1] - a[1], b[0] / n
        merged = torch.stack((n, a[1] + d * f, a[2] + b[2] + d * d * (a[0] * f)))
        return torch.where(a[0] == 0, b, torch.where(b[0] == 0, a, merged))
    ha, hb, out = _host(a, np.float64).reshape(-1), _host(b, np.float64).reshape(-1), np.empty(3, dtype=np.float64)
    if ha.shape != (3,) or hb.shape != (3,):
        raise RoverError("combine_moments: expected two triples (count, mean, M2)")
    host_call("rover_combine_moments", ha.ctypes.data, hb.ctypes.data, out.ctypes.data)
    return out


def gauss_head_desc(A, log_std=_FAKE, actions=_FAKE, log_prob=_FAKE, clip_log_std=True, min_log_std=-20.0, max_log_std=2.0, clip_actions=False,
                    low=-1.0, high=1.0, reduction="sum", deterministic=False, seed=0, step=0, step_dev=None, row_offset=0, taken_actions=None,
                    taken_stride=None, actions_stride=None, log_prob_stride=None, mean=None, mean_stride=None):
    """A rover_gauss_head from plain values (pointers as integers; the defaults are skrl's as the reference sets them, model.py:153-156).
    ``reduction``: a name of REDUCTIONS or a code."""
    red = reduction if isinstance(reduction, int) and not isinstance(reduction, bool) else REDUCTIONS[reduction]
    A = int(A)
    return GaussHead(log_std, A, int(bool(clip_log_std)), float(min_log_std), float(max_log_std), int(bool(clip_actions)), float(low), float(high),
                     int(red), int(bool(deterministic)), int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), step_dev, int(row_offset),
                     taken_actions, A if taken_stride is None else int(taken_stride), actions, A if actions_stride is None else int(actions_stride),
                     log_prob, (A if red == 5 else 1) if log_prob_stride is None else int(log_prob_stride), mean,
                     A if mean_stride is None else int(mean_stride))


def gae_desc(t, e, rewards=1 << 40, values=2 << 40, dones=3 << 40, last_values=4 << 40, returns=5 << 40, advantages=6 << 40, stats_out=None,
             stats_in=None, normalize=GAE_RAW, gamma=0.99, lam=0.95, **strides):
    """A rover_gae_desc from plain values (pointers as integers, disjoint by default; ``<name>_stride`` defaults to ``e``)."""
    st = lambda name: int(strides.pop(name + "_stride", e))
    d = GaeDesc(int(t), int(e), float(gamma), float(lam), rewards, st("rewards"), values, st("values"), dones, st("dones"), last_values, returns,
                st("returns"), advantages, st("advantages"), int(normalize), stats_out, stats_in)
    if strides:
        raise TypeError(f"gae_desc: unknown arguments {sorted(strides)}")
    return d


def ppo_loss_desc(m, a, mean_stride=None, actions_stride=None, d_mean_stride=None, **ptrs):
    """A rover_ppo_loss_desc from plain values: skrl's scalars, the strides default to ``a``, every pointer an integer (disjoint fake
    addresses by default; ``name=None`` or another address through ``ptrs``)."""
    names = ("mean", "log_std", "actions", "old_log_prob", "advantages", "value", "old_values", "returns", "d_mean", "d_value", "d_log_std", "stats")
    p = {name: (i + 1) << 40 for i, name in enumerate(names)}
    if set(ptrs) - set(names):
        raise TypeError(f"ppo_loss_desc: unknown arguments {sorted(set(ptrs) - set(names))}")
    p.update(ptrs)
    a = int(a)
    st = lambda v: a if v is None else int(v)
    return PpoLossDesc(int(m), a, p["mean"], st(mean_stride), p["log_std"], p["actions"], st(actions_stride), p["old_log_prob"], p["advantages"], p["value"],
                       p["old_values"], p["returns"], 1, -20.0, 2.0, REDUCTIONS["sum"], 0.2, 0.2, 1, 0.0, 1.0, p["d_mean"], st(d_mean_stride), p["d_value"],
                       p["d_log_std"], p["stats"])


PRECISIONS = ("f32", "bf16")


def _precision_suffix(precision):
    """"" / "_bf16": the suffix of the entry points of ``precision`` (rover_mlp_chain_forward / rover_mlp_chain_forward_bf16, rover_gru_cell /
    rover_gru_cell_bf16, rover_linear_forward / rover_linear_forward_bf16 and their route queries)."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, not {precision!r}")
    return "" if precision == "f32" else "_bf16"


def chain_act_route(m, k0, widths, activations, head=None, precision="f32"):
    """rover_mlp_chain_act_route: "mlp_small+gauss" / "chain16<16,10,8,1>+gauss" (the head inside the chain's last kernel),
    "<chain route>;gauss" (the head as a launch of its own), "none" for m = 0, None where rover_mlp_chain_act would refuse the call.
    ``head``: a GaussHead (gauss_head_desc) — default: the reference's settings with A = widths[-1].  ``precision="bf16"``:
    rover_mlp_chain_act_route_bf16 ("chain_bf16<16,10,8,1>+gauss", ...)."""
    k0, n, w, a = LearnEngine._chain_shape(k0, widths, activations)
    if head is None:
        head = gauss_head_desc(widths[-1])
    return route_query("rover_mlp_chain_act_route" + _precision_suffix(precision), int(m), k0, n, w, a, C.byref(head))


def bf16_round(values):
    """rover_bf16_round: ``values`` (anything numpy turns into float32) rounded to bf16 as the bf16 chain kernels round their inputs,
    weights and hidden activations -> a float32 array of the same shape.  Host only."""
    x = np.ascontiguousarray(values, dtype=np.float32)
    out = np.empty_like(x)
    host_call("rover_bf16_round", x.ctypes.data, x.size, out.ctypes.data)
    return out


class LearnEngine(EngineBase):
    ACTIVATIONS = {"none": 0, None: 0, "leakyrelu": 1, "tanh": 2, "relu": 3, "elu": 4}

    def linear_forward(self, x, weight, bias, activation, out, precision="f32"):
        """out[:, :N] = act(x[:, :K] @ weight.T + bias); x / out may be column slices of wider row-major tensors.
        ``precision="bf16"``: x and weight rounded to bf16 as they are read, f32 accumulation, bias, activation and output
        (rover_linear_forward_bf16; the arithmetic is stated in rover_step.h)."""
        name = "rover_linear_forward" + _precision_suffix(precision)
        m, k = x.shape
        n = weight.shape[0]
        self._f32_rows(x, "x", "linear_forward")
        self._f32_rows(out, "out", "linear_forward")
        if k > 0:
            self._chk(weight, (n, k), torch.float32, "weight")
        self._chk(bias, (n,), torch.float32, "bias")
        if out.shape[0] != m or out.shape[1] != n:
            raise RoverError(f"linear_forward: out must be [{m},{n}]")
        self._call(name, *_rows(x, k, m), m, k, _ptr(weight), _ptr(bias), n, self.ACTIVATIONS[activation], *_rows(out, n, m))
        return out

    @staticmethod
    def chain_shape(layers):
        """(k0, widths, activations) of ``layers`` (objects with .weight [n, k], .activation): what the chain route queries take."""
        return layers[0].weight.shape[1], [l.weight.shape[0] for l in layers], [l.activation for l in layers]

    @classmethod
    def chain_fits(cls, layers):
        """True if ``layers`` can run as one rover_mlp_chain_forward launch — the library's answer: rover_mlp_chain_route names a kernel.
        Whether a chain fits does not depend on the number of rows (only which kernel runs it does): asked at one fixed row count."""
        return len(layers) > 0 and cls.chain_route(1, *cls.chain_shape(layers)) is not None

    def _chain(self, what, x, layers, out, keep, out_name="out"):
        """-> the ChainDesc of ``layers`` (objects with .weight [n, k], .bias [n], .activation) from x [m, k0] to out [m, n_last], all checked
        (errors under ``what``, the calling method's name).  The arrays it points at go into ``keep``: they live until the call returns."""
        m, k0 = x.shape
        self._f32_rows(x, "x", what)
        self._f32_rows(out, out_name, what)
        n, k = len(layers), k0
        for l in layers:
            self._chk(l.weight, (l.weight.shape[0], k), torch.float32, "weight")
            self._chk(l.bias, (l.weight.shape[0],), torch.float32, "bias")
            k = l.weight.shape[0]
        if out.shape[0] != m or out.shape[1] != k:
            raise RoverError(f"{what}: {out_name} must be [{m},{k}]")
        w = (C.c_void_p * n)(*[_ptr(l.weight) for l in layers])
        b = (C.c_void_p * n)(*[_ptr(l.bias) for l in layers])
        widths = (C.c_int32 * n)(*[l.weight.shape[0] for l in layers])
        acts = (C.c_int32 * n)(*[self.ACTIVATIONS[l.activation] for l in layers])
        keep.extend((w, b, widths, acts))
        return ChainDesc(*_rows(x, k0, m), k0, n, C.addressof(w), C.addressof(b), C.addressof(widths), C.addressof(acts), *_rows(out, k, m))

    def chain_forward(self, x, layers, out, precision="f32"):
        """out = layers[-1](... layers[0](x)) in one kernel; ``layers``: objects with .weight [n, k], .bias [n], .activation.
        ``precision="bf16"``: bf16 operands, f32 accumulation (rover_mlp_chain_forward_bf16; the arithmetic is stated in rover_step.h)."""
        name = "rover_mlp_chain_forward" + _precision_suffix(precision)
        keep = []
        d = self._chain("chain_forward", x, layers, out, keep)
        self._call(name, d.x, d.x_stride, x.shape[0], d.K0, d.n_layers, d.weights, d.biases, d.widths, d.activations, d.y, d.y_stride)
        return out

    def chain_pair_forward(self, xa, layers_a, out_a, xb, layers_b, out_b, copy_src=None, copy_dst=None, copy_cols=0):
        """Two 2-layer chains over the same rows (the two encoders: rover_mlp_chain_pair_forward) and, optionally,
        copy_dst[:, :copy_cols] = copy_src[:, :copy_cols] — side by side in one launch per stage at small batches."""
        if xa.shape[0] != xb.shape[0]:
            raise RoverError("chain_pair_forward: the two chains must have the same number of rows")
        keep = []
        da, db = self._chain("chain_pair_forward", xa, layers_a, out_a, keep), self._chain("chain_pair_forward", xb, layers_b, out_b, keep)
        if copy_cols:
            for t, name in ((copy_src, "copy_src"), (copy_dst, "copy_dst")):
                if self._f32_rows(t, name, "chain_pair_forward").shape[0] != xa.shape[0] or t.shape[1] < copy_cols:
                    raise RoverError(f"chain_pair_forward: {name} must have the same rows and >= copy_cols columns")
        copy = lambda t: _rows(t if copy_cols else None, int(copy_cols), xa.shape[0])
        self._call("rover_mlp_chain_pair_forward", xa.shape[0], C.byref(da), C.byref(db), *copy(copy_src), *copy(copy_dst), int(copy_cols))

    # ---- the actor's Gaussian head (rover_gauss_head) --------------------------------------------------
    def _gauss_head(self, what, m, log_std, actions, log_prob, mean=None, taken_actions=None, step_dev=None, reduction="sum", **kw):
        """-> GaussHead over checked tensors (log_std [A]; actions [m, A]; log_prob [m, 1], or [m, A] with reduction None)."""
        a = int(log_std.numel())
        self._chk(log_std, (a,), torch.float32, "log_std")
        if reduction not in REDUCTIONS:
            raise RoverError(f"{what}: unknown reduction {reduction!r}")
        self._f32_rows(actions, "actions", what, (m, a))
        self._f32_rows(log_prob, "log_prob", what, (m, a if REDUCTIONS[reduction] == 5 else 1))
        if taken_actions is not None:
            self._f32_rows(taken_actions, "taken_actions", what, (m, a))
        if mean is not None:
            self._f32_rows(mean, "mean", what, (m, a))
        if step_dev is not None and (not step_dev.is_cuda or step_dev.dtype != torch.int64 or step_dev.numel() != 1):
            raise RoverError(f"{what}: step_dev must be one int64 word on the GPU (read as uint64)")
        dp = lambda t: None if t is None else t.data_ptr()
        (tp, ts), (ap, as_), (lp, ls), (mp, ms) = (_rows(t, cols, m) for t, cols in ((taken_actions, a), (actions, a), (log_prob, log_prob.shape[1]), (mean, a)))
        return gauss_head_desc(a, dp(log_std), ap, lp, reduction=reduction, step_dev=dp(step_dev), taken_actions=tp, taken_stride=ts, actions_stride=as_,
                               log_prob_stride=ls, mean=mp, mean_stride=ms, **kw)

    def chain_act(self, x, layers, mean_out, log_std, actions, log_prob, precision="f32", **head):
        """chain_forward with the Gaussian head on its output (rover_mlp_chain_act): ``mean_out`` receives what chain_forward writes,
        ``actions`` / ``log_prob`` the head's results.  ``head``: taken_actions, step_dev, reduction and the scalar fields of
        gauss_head_desc (seed, step, row_offset, deterministic, clip_*, ...).  ``precision="bf16"``: rover_mlp_chain_act_bf16 (the f32
        head on the bf16 chain's f32 mean)."""
        name = "rover_mlp_chain_act" + _precision_suffix(precision)
        keep = []
        d = self._chain("chain_act", x, layers, mean_out, keep, "mean_out")
        desc = self._gauss_head("chain_act", x.shape[0], log_std, actions, log_prob, **head)
        self._call(name, d.x, d.x_stride, x.shape[0], d.K0, d.n_layers, d.weights, d.biases, d.widths, d.activations, d.y, d.y_stride,
                   C.byref(desc))
        return actions, log_prob

    def gaussian_head(self, mean, log_std, actions, log_prob, **head):
        """The head on a given ``mean`` [m, A], A <= 16 (rover_gaussian_head): one launch."""
        self._f32_rows(mean, "mean", "gaussian_head")
        desc = self._gauss_head("gaussian_head", mean.shape[0], log_std, actions, log_prob, mean=mean, **head)
        self._call("rover_gaussian_head", mean.shape[0], C.byref(desc))
        return actions, log_prob

    def policy_noise(self, m, a, seed=0, step=0, step_dev=None, row_offset=0, out=None):
        """eps [m, a] as the head draws it for (seed, step + *step_dev, row_offset) (rover_policy_noise)."""
        if out is None:
            out = torch.empty(int(m), int(a), device=self.device)
        self._f32_rows(out, "out", "policy_noise", (int(m), int(a)))
        self._call("rover_policy_noise", int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), _ptr(step_dev), int(row_offset), int(m), int(a),
                   *_rows(out, int(a), int(m)))
        return out

    chain_act_route = staticmethod(chain_act_route)
    bf16_round = staticmethod(bf16_round)

    # ---- the student's recurrent block (rover_gru_cell, rover_gated_sum) -------------------------------------
    def _gru_operands(self, what, m, rows, w_hh, reset_mask, k=0, w_ih=None, b_ih=None, b_hh=None):
        """The operand checks the three GRU calls share -> (h, the reset mask as the uint8 tensor the C ABI reads).  h is w_hh's width;
        ``rows``: (tensor, name, c) triples, each a float32 matrix [m, c h]; w_ih [3h, k] (not read with k = 0), w_hh [3h, h], b_ih / b_hh
        [3h] or None; ``reset_mask``: optional [m] bool / uint8."""
        hd = w_hh.shape[1] if w_hh is not None and w_hh.dim() == 2 else -1
        for t, name, c in rows:
            self._f32_rows(t, name, what, (m, c * hd))
        if k > 0:
            self._chk(w_ih, (3 * hd, k), torch.float32, "w_ih")
        self._chk(w_hh, (3 * hd, hd), torch.float32, "w_hh")
        self._chk(b_ih, (3 * hd,), torch.float32, "b_ih")
        self._chk(b_hh, (3 * hd,), torch.float32, "b_hh")
        if reset_mask is not None:
            if reset_mask.dtype == torch.bool:
                reset_mask = reset_mask.view(torch.uint8)
            self._chk(reset_mask, (m,), torch.uint8, "reset_mask")
        return hd, reset_mask

    def _gru_forward(self, name, x, h_in, w_ih, w_hh, b_ih, b_hh, h_out, reset_mask, *more):
        """gru_cell and gru_cell_train: the checks, then the entry point ``name``; ``more``: the (tensor, name, c) rows it takes behind h_out."""
        what = name[len("rover_"):]
        self._f32_rows(x, "x", what)
        m, k = x.shape
        hd, reset_mask = self._gru_operands(what, m, ((h_in, "h_in", 1), (h_out, "h_out", 1)) + more, w_hh, reset_mask, k, w_ih, b_ih, b_hh)
        self._call(name, *_rows(x, k, m), *_rows(h_in, hd, m), m, k, hd, _ptr(w_ih) if k > 0 else None, _ptr(w_hh), _ptr(b_ih), _ptr(b_hh),
                   _ptr(reset_mask), *_rows(h_out, hd, m), *[v for t, _, c in more for v in _rows(t, c * hd, m)])
        return h_out

    def gru_cell(self, x, h_in, w_ih, w_hh, b_ih, b_hh, h_out, reset_mask=None, precision="f32"):
        """One layer of torch.nn.GRU for one time step (rover_gru_cell): h_out = cell(x [m, k], h_in [m, h]); w_ih [3h, k], w_hh [3h, h],
        b_ih / b_hh [3h] or None.  x, h_in and h_out may be column slices / padded rows; ``reset_mask``: optional [m] bool / uint8 —
        marked rows read h_in as zero.  h_out must not overlap h_in (the library refuses it).  ``precision="bf16"``: the operands of the
        matrix products rounded to bf16 as they are read; gates, blend and h_out in f32 on the unrounded h_in (rover_gru_cell_bf16)."""
        return self._gru_forward("rover_gru_cell" + _precision_suffix(precision), x, h_in, w_ih, w_hh, b_ih, b_hh, h_out, reset_mask)

    @classmethod
    def gru_cell_route(cls, m, k, h, precision="f32"):
        """The instantiation gru_cell runs for [m, k] inputs and a hidden width h ("gru_cell<4>", "gru_cell<1>"; ``precision="bf16"``:
        "gru_cell_bf16<128,64>"); "none" for m = 0, None where the call would be refused.  Host only."""
        return route_query("rover_gru_cell_route" + _precision_suffix(precision), int(m), int(k), int(h))

    def gru_cell_train(self, x, h_in, w_ih, w_hh, b_ih, b_hh, h_out, gates, reset_mask=None):
        """gru_cell that also stores ``gates`` [m, 4h] = r | z | n | q for gru_cell_backward (rover_gru_cell_train); h_out has gru_cell's bits."""
        return self._gru_forward("rover_gru_cell_train", x, h_in, w_ih, w_hh, b_ih, b_hh, h_out, reset_mask, (gates, "gates", 4))

    def gru_cell_backward(self, dh_above, dh_next, gates, h_in, w_hh, dgi, dgh, dh_in, reset_mask=None):
        """rover_gru_cell_backward: one layer, one time step, one launch.  dh_above / dh_next (or None) / h_in / dh_in [m, h], gates
        [m, 4h] as gru_cell_train stored them, dgi / dgh [m, 3h]; all float32 rows with unit column stride (slices will do)."""
        what = "gru_cell_backward"
        m = self._f32_rows(dh_above, "dh_above", what).shape[0]
        rows = ((dh_above, "dh_above", 1), (gates, "gates", 4), (h_in, "h_in", 1), (dgi, "dgi", 3), (dgh, "dgh", 3), (dh_in, "dh_in", 1))
        hd, reset_mask = self._gru_operands(what, m, rows + (() if dh_next is None else ((dh_next, "dh_next", 1),)), w_hh, reset_mask)
        self._call("rover_gru_cell_backward", *_rows(dh_above, hd, m), *_rows(dh_next, hd, m), *_rows(gates, 4 * hd, m), *_rows(h_in, hd, m),
                   _ptr(reset_mask), _ptr(w_hh), m, hd, *_rows(dgi, 3 * hd, m), *_rows(dgh, 3 * hd, m), *_rows(dh_in, hd, m))
        return dh_in

    @classmethod
    def gru_cell_backward_route(cls, m, h):
        """The instantiation gru_cell_backward runs ("gru_bwd<4>", "gru_bwd<1>"); "none" for m = 0, None where refused.  Host only."""
        return route_query("rover_gru_cell_backward_route", int(m), int(h))

    def gated_sum_backward(self, d_out, mul, pre, d_mul=None, d_pre=None):
        """rover_gated_sum_backward: d_mul = d_out * sigmoid(pre), d_pre = (d_out * mul) * s (1 - s) over [m, n]; each output optional.
        mul / pre may be one row expanded over the rows (row stride 0); the outputs are per row."""
        what = "gated_sum_backward"
        m, n = self._f32_rows(d_out, "d_out", what).shape
        self._f32_rows(pre, "pre", what, (m, n))
        for t, name in ((mul, "mul"), (d_mul, "d_mul"), (d_pre, "d_pre")):
            if t is not None:
                self._f32_rows(t, name, what, (m, n))
        if d_pre is not None and mul is None:
            raise RoverError(f"{what}: d_pre needs mul")
        self._call("rover_gated_sum_backward", *_rows(d_out, n, m), *_rows(mul, n, m), *_rows(pre, n, m), m, n, *_rows(d_mul, n, m), *_rows(d_pre, n, m))

    def linear_dgrad(self, y, dy, weight, activation, dx):
        """rover_linear_dgrad: dx = (dy * act'(y)) @ weight for any widths; ``y`` may be None with activation None.  Enqueues only."""
        what = "linear_dgrad"
        n, k = weight.shape
        m = self._f32_rows(dy, "dy", what).shape[0]
        if dy.shape[1] != n:
            raise RoverError(f"{what}: dy must be [{m},{n}]")
        if y is not None or self.ACTIVATIONS[activation] != 0:
            self._f32_rows(y, "y", what, (m, n))
        self._chk(weight, (n, k), torch.float32, "weight")
        self._f32_rows(dx, "dx", what, (m, k))
        self._call("rover_linear_dgrad", *_rows(y, n, m), *_rows(dy, n, m), m, k, _ptr(weight), n, self.ACTIVATIONS[activation], *_rows(dx, k, m))
        return dx

    @classmethod
    def linear_dgrad_route(cls, m, k, n):
        """What linear_dgrad launches ("dgrad<1,1>x10", ...); "none" for m = 0, None where the call would be refused.  Host only."""
        return route_query("rover_linear_dgrad_route", int(m), int(k), int(n))

    def gated_sum(self, add, mul, pre, out):
        """out = add + mul * sigmoid(pre) over [m, n] (rover_gated_sum), one launch.  All four are float32 GPU matrices with unit column
        stride; an input may be a one-row matrix expanded over the rows (row stride 0)."""
        what = "gated_sum"
        self._f32_rows(out, "out", what)
        m, n = out.shape
        for t, name in ((add, "add"), (mul, "mul"), (pre, "pre")):
            self._f32_rows(t, name, what, (m, n))
        self._call("rover_gated_sum", *_rows(add, n, m), *_rows(mul, n, m), *_rows(pre, n, m), m, n, *_rows(out, n, m))
        return out

    # ---- the rollout side of PPO (rover_gae) -------------------------------------------------------------
    def _gae_rows(self, t, name, dtype, T=None, E=None):
        """``t`` must be a [T, E] or skrl-shaped [T, E, 1] GPU tensor of ``dtype`` with unit env stride (a padded buffer's view will do)
        -> (pointer, time stride in elements, T, E)."""
        ok = t is not None and t.is_cuda and t.device == self.device and t.dtype == dtype and (t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 1))
        if ok:
            sh = (int(t.shape[0]), int(t.shape[1]))
            ok = (sh[1] <= 1 or t.stride(1) == 1) and (T is None or sh == (T, E)) and (sh[0] <= 1 or t.stride(0) >= sh[1])
        if not ok:
            raise RoverError(f"gae: {name} must be a {dtype} tensor{'' if T is None else ' [%d,%d] or [%d,%d,1]' % (T, E, T, E)} on {self.device} "
                             "with unit env stride and a time stride >= E")
        return (*_rows(t, sh[1], sh[0]), sh[0], sh[1])

    def _gae_stats(self, t, name):
        if t is not None and (not t.is_cuda or t.device != self.device or t.dtype != torch.float64 or t.numel() != 3 or not t.is_contiguous()):
            raise RoverError(f"gae: {name} must be 3 contiguous float64 words (count, mean, M2) on {self.device}")
        return None if t is None else t.data_ptr()

    def gae(self, rewards, values, dones, last_values, returns, advantages, gamma=0.99, lam=0.95, normalize=True, stats_out=None, stats_in=None):
        """rover_gae: returns and advantages of a stored rollout in one pass.  rewards / values / returns / advantages: float32 [T, E] or
        [T, E, 1]; dones: torch.bool or uint8 of that shape; last_values: float32 [E] or [E, 1], contiguous.  Time strides are taken from
        the tensors (padded buffers and skrl-shaped storage work in place); ``returns`` may be ``values``.  ``normalize``: False = raw A,
        True = (A - mean) / (std + 1e-8) with this call's own moments — or, when ``stats_in`` (3 float64 on the device) is given, with
        those.  ``stats_out`` (3 float64 on the device) receives (count, mean, M2) of this call's raw A.  Enqueues only."""
        rp, rs, T, E = self._gae_rows(rewards, "rewards", torch.float32)
        vp, vs, _, _ = self._gae_rows(values, "values", torch.float32, T, E)
        if dones is not None and dones.dtype == torch.bool:
            dones = dones.view(torch.uint8)
        dp, ds, _, _ = self._gae_rows(dones, "dones", torch.uint8, T, E)
        op, os_, _, _ = self._gae_rows(returns, "returns", torch.float32, T, E)
        ap, as_, _, _ = self._gae_rows(advantages, "advantages", torch.float32, T, E)
        if last_values is None or tuple(last_values.shape) not in ((E,), (E, 1)):
            raise RoverError(f"gae: last_values must be [{E}] or [{E},1]")
        self._chk(last_values, tuple(last_values.shape), torch.float32, "last_values")
        if stats_in is not None and not normalize:
            raise RoverError("gae: stats_in is only read when normalize is set")
        mode = GAE_RAW if not normalize else (GAE_NORMALIZE if stats_in is None else GAE_NORMALIZE_GIVEN)
        d = GaeDesc(T, E, float(gamma), float(lam), rp, rs, vp, vs, dp, ds, last_values.data_ptr(), op, os_, ap, as_, mode,
                    self._gae_stats(stats_out, "stats_out"), self._gae_stats(stats_in, "stats_in"))
        self._call("rover_gae", C.byref(d))
        return returns, advantages

    # ---- the learner side of PPO (rover_linear_backward, rover_ppo_loss) ---------------------------------
    def linear_backward(self, x, y, dy, weight, activation, dx=None, dweight=None, dbias=None):
        """rover_linear_backward: the backward of ``y = act(x @ weight.T + bias)``.  ``y`` is the layer's output as linear_forward wrote
        it, ``dy`` the gradient at it; x / y / dy / dx may be column slices of wider row-major tensors; ``dweight`` [n, k] and ``dbias``
        [n] are contiguous.  Each output is optional (None: not computed); ``x`` may be None without ``dweight``, ``y`` with activation None.
        Enqueues only."""
        what = "linear_backward"
        n, k = weight.shape
        m = self._f32_rows(dy, "dy", what).shape[0]
        if dy.shape[1] != n:
            raise RoverError(f"{what}: dy must be [{m},{n}]")
        if y is not None or self.ACTIVATIONS[activation] != 0:        # without an activation the derivative needs no y
            self._f32_rows(y, "y", what, (m, n))
        if k > 0:
            self._chk(weight, (n, k), torch.float32, "weight")
        if x is not None:
            self._f32_rows(x, "x", what, (m, k))
        elif dweight is not None and k > 0:
            raise RoverError(f"{what}: dweight needs x")
        if dx is not None:
            self._f32_rows(dx, "dx", what, (m, k))
        if dweight is not None and k > 0:
            self._chk(dweight, (n, k), torch.float32, "dweight")
        if dbias is not None:
            self._chk(dbias, (n,), torch.float32, "dbias")
        self._call("rover_linear_backward", *_rows(x, k, m), *_rows(y, n, m), *_rows(dy, n, m), m, k, _ptr(weight), n, self.ACTIVATIONS[activation],
                   *_rows(dx, k, m), _ptr(dweight), _ptr(dbias))

    def ppo_loss(self, mean, log_std, actions, old_log_prob, advantages, value, old_values, returns, d_mean, d_value, d_log_std, stats,
                 ratio_clip=0.2, value_clip=0.2, clip_predicted_values=True, entropy_loss_scale=0.0, value_loss_scale=1.0, clip_log_std=True,
                 min_log_std=-20.0, max_log_std=2.0, reduction="sum"):
        """rover_ppo_loss: the PPO minibatch loss at the nets' outputs and its gradients.  mean / actions / d_mean: float32 [m, A] (column
        slices will do); the per-row arrays float32 [m] or [m, 1], contiguous; log_std / d_log_std [A]; ``stats``: 4 float64 on the
        device, receives (policy_loss, value_loss, entropy_loss, kl).  Enqueues only; capturable."""
        what = "ppo_loss"
        m, a = self._f32_rows(mean, "mean", what).shape
        self._f32_rows(actions, "actions", what, (m, a))
        self._f32_rows(d_mean, "d_mean", what, (m, a))
        for t, name in ((old_log_prob, "old_log_prob"), (advantages, "advantages"), (value, "value"), (old_values, "old_values"), (returns, "returns"),
                        (d_value, "d_value")):
            if t is None or tuple(t.shape) not in ((m,), (m, 1)):
                raise RoverError(f"{what}: {name} must be [{m}] or [{m},1]")
            self._chk(t, tuple(t.shape), torch.float32, name)
        self._chk(log_std, (a,), torch.float32, "log_std")
        self._chk(d_log_std, (a,), torch.float32, "d_log_std")
        if stats is None or not stats.is_cuda or stats.dtype != torch.float64 or stats.numel() != 4 or not stats.is_contiguous():
            raise RoverError(f"{what}: stats must be 4 contiguous float64 words on the GPU")
        if reduction not in REDUCTIONS:
            raise RoverError(f"{what}: unknown reduction {reduction!r}")
        d = PpoLossDesc(m, a, *_rows(mean, a, m), log_std.data_ptr(), *_rows(actions, a, m),
                        old_log_prob.data_ptr(), advantages.data_ptr(), value.data_ptr(), old_values.data_ptr(), returns.data_ptr(),
                        int(bool(clip_log_std)), float(min_log_std), float(max_log_std), REDUCTIONS[reduction], float(ratio_clip), float(value_clip),
                        int(bool(clip_predicted_values)), float(entropy_loss_scale), float(value_loss_scale), *_rows(d_mean, a, m), d_value.data_ptr(), d_log_std.data_ptr(), stats.data_ptr())
        self._call("rover_ppo_loss", C.byref(d))
        return stats

    # ---- the optimiser step (rover_optim_*) ---------------------------------------------------------------
    @classmethod
    def optim_plan(cls, numel):
        """rover_optim_plan: the chunks the optimiser kernels walk for tensors of ``numel`` elements -> [(tensor, first, length)], in
        tensor order then element order.  Host only: no ctx, no device.  The chunk length is the library's constant: read it off the
        plan of one long tensor."""
        sizes = [int(v) for v in numel]
        arr = (C.c_int64 * max(len(sizes), 1))(*sizes)
        n = C.c_int64(0)
        host_call("rover_optim_plan", len(sizes), arr, None, 0, C.byref(n))
        chunks = (OptimChunk * max(n.value, 1))()
        host_call("rover_optim_plan", len(sizes), arr, chunks, n.value, C.byref(n))
        return [(int(c.tensor), int(c.first), int(c.length)) for c in chunks[:n.value]]

    def _optim_word(self, t, name, dtype, what):
        if t is None or not t.is_cuda or t.device != self.device or t.dtype != dtype or t.numel() != 1:
            raise RoverError(f"{what}: {name} must be one {dtype} word on {self.device}")
        return t.data_ptr()

    def optim_create(self, params, grads, exp_avg, exp_avg_sq, step, stopped):
        """rover_optim_create: binds contiguous float32 ``params`` and their ``grads`` (two lists of GPU tensors, pairwise of one shape;
        empty tensors are allowed) to the caller's state — ``exp_avg`` / ``exp_avg_sq``: flat float32 of sum(numel) elements in tensor
        order, zeroed; ``step``: one int64; ``stopped``: one int32 — and returns the handle.  Every tensor must stay alive, and stay
        the same storage, as long as the handle is used."""
        what = "optim_create"
        params, grads = list(params), list(grads)
        if len(params) != len(grads):
            raise RoverError(f"{what}: {len(params)} params but {len(grads)} grads")
        for i, (p, g) in enumerate(zip(params, grads)):
            self._chk(p, tuple(p.shape), torch.float32, f"params[{i}]")
            self._chk(g, tuple(p.shape), torch.float32, f"grads[{i}]")
        n = len(params)
        numel = [p.numel() for p in params]
        total = sum(numel)
        self._chk(exp_avg, (total,), torch.float32, "exp_avg")
        self._chk(exp_avg_sq, (total,), torch.float32, "exp_avg_sq")
        ptrs = lambda ts: (C.c_void_p * max(n, 1))(*[t.data_ptr() if t.numel() else None for t in ts])
        pa, ga, na = ptrs(params), ptrs(grads), (C.c_int64 * max(n, 1))(*numel)
        d = OptimDesc(n, C.cast(pa, C.c_void_p), C.cast(ga, C.c_void_p), C.cast(na, C.c_void_p), exp_avg.data_ptr() if total else None,
                      exp_avg_sq.data_ptr() if total else None, self._optim_word(step, "step", torch.int64, what),
                      self._optim_word(stopped, "stopped", torch.int32, what))
        h = C.c_int32(-1)
        self._call("rover_optim_create", C.byref(d), C.byref(h))
        return int(h.value)

    def optim_destroy(self, handle):
        self._call("rover_optim_destroy", int(handle))

    def optim_step(self, handle, lr, beta1=0.9, beta2=0.999, eps=1e-8, grad_norm_clip=0.0, gate=None, gate_threshold=0.0, norm_out=None):
        """rover_optim_step: clip_grad_norm_ (``grad_norm_clip`` <= 0: none) and one Adam step over the handle's tensors in two launches.
        ``gate`` (one float64 on the device, e.g. ``stats[3:]`` of ppo_loss): the step is skipped, and the handle's ``stopped`` latch
        set, when the latch is set already or ``gate > gate_threshold``.  ``norm_out`` (one float64 on the device) receives the
        gradient norm before clipping.  Enqueues only; capturable."""
        what = "optim_step"
        d = OptimStepDesc(float(lr), float(beta1), float(beta2), float(eps), float(grad_norm_clip),
                          None if gate is None else self._optim_word(gate, "gate", torch.float64, what), float(gate_threshold),
                          None if norm_out is None else self._optim_word(norm_out, "norm_out", torch.float64, what))
        self._call("rover_optim_step", int(handle), C.byref(d))

    @classmethod
    def linear_backward_route(cls, m, k, n, want_dx):
        """What linear_backward launches ("wgrad<3,4>/64;dgrad<1,4>", ...: the weight-gradient instantiation and its M-split, then the
        dx kernel); "zero" for m = 0, None where the call would be refused."""
        return route_query("rover_linear_backward_route", int(m), int(k), int(n), int(bool(want_dx)))

    # ---- which kernel a forward call runs (host only: no ctx, no launch) ----------------------------
    _route = staticmethod(_route)

    @classmethod
    def _chain_shape(cls, k0, widths, activations):
        n = len(widths)
        if len(activations) != n:
            raise RoverError("chain route: one activation per layer")
        return (int(k0), n, (C.c_int32 * n)(*[int(w) for w in widths]),
                (C.c_int32 * n)(*[a if isinstance(a, int) else cls.ACTIVATIONS[a] for a in activations]))

    @classmethod
    def linear_route(cls, m, k, n, precision="f32"):
        """The instantiation linear_forward runs for an [m, k] x [n, k]^T layer ("linear_act<3,4>x2", ...; ``precision="bf16"``:
        "linear_bf16<128,128>"); "none" for m = 0, None where the call would be refused."""
        return route_query("rover_linear_route" + _precision_suffix(precision), int(m), int(k), int(n))

    @classmethod
    def chain_route(cls, m, k0, widths, activations, precision="f32"):
        """The kernel chain_forward runs ("splitk<6,2>", "mlp_small", "chain16<16,10,8,1>", ...; ``precision="bf16"``:
        "chain_bf16<5,4,0,0>", ...); activations: names or codes."""
        k0, n, w, a = cls._chain_shape(k0, widths, activations)
        return route_query("rover_mlp_chain_route" + _precision_suffix(precision), int(m), k0, n, w, a)

    @classmethod
    def chain_pair_route(cls, m, a, b):
        """The launches of chain_pair_forward: "pair(splitk<TN,RT>)" or "seq(<a>;<b>)"; a, b = (k0, widths, activations)."""
        descs = []
        for k0, widths, acts in (a, b):
            k0, n, w, ac = cls._chain_shape(k0, widths, acts)
            descs.append((ChainDesc(None, k0, k0, n, None, None, C.addressof(w), C.addressof(ac), None, 0), w, ac))
        return route_query("rover_mlp_chain_pair_route", int(m), C.byref(descs[0][0]), C.byref(descs[1][0]))
