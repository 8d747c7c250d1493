"""Reference for the bf16 chain kernels (csrc/rover_mlp.hip, chain_bf16<...>; the arithmetic is stated in include/rover_step.h).

The f32 accumulation order of the hardware cannot be reproduced on the CPU, and a worst-case bound through three bf16 roundings is
nearly useless (median 0.13 against |y| <= 1 on 124 -> 256 -> 160 -> 128 -> 2).  So the weight of the testing rests on LATTICE data, for
which the arithmetic is exact:

  * x integer-valued, weights in {-1, 0, +1}, integer biases, activations none / ReLU; lattice() asserts, in float64, that
    sum |w| |h| + |b| < 2^24 on every row of every layer.  Every f32 partial sum is then an exact integer in ANY order, so the kernel's
    result is determined bit for bit and compared with ==.  (LeakyReLU on the last layer is one f32 multiply: still exact; a tanh
    head's last layer is scaled by a power of two and compared within 8 u |y|.)
  * lattice() also asserts that at least one hidden value of every rounded layer is not bf16-representable — otherwise a kernel that
    truncated, or did not round at all, would pass.

For arbitrary data (LeakyReLU, real weights) reference() propagates mlp_ref.reference's f32 bound e within a layer and, at each
rounding, takes h <- rd(h), e <- rd(h + e) - rd(h - e): rounding is monotone, so the kernel's rounded value and the reference's both lie
between those two.  Derived, not fitted.

Everything here runs on the CPU in float64 (torch), whatever device the inputs live on.
"""
import numpy as np
import torch

import mlp_ref as R

_LOW = (1 << 45) - 1                 # the 45 mantissa bits of a float64 that a bf16 does not have
BF16_MAX = float.fromhex("0x1.fep+127")


def _rd_bits(x64, round_up_half):
    bits = x64.contiguous().view(torch.int64)
    if round_up_half:                # round to nearest even on the bits: no double rounding through float32
        bits = bits + ((1 << 44) - 1 + ((bits >> 45) & 1))
    return (bits & ~_LOW).view(torch.float64)


def rd(x, truncate=False):
    """x (float64 tensor, or anything torch.as_tensor takes) rounded to the nearest bf16, ties to even -> float64.  NaN stays NaN,
    +-Inf stays +-Inf, a finite value that rounds past the largest bf16 becomes +-Inf; below 2^-126 the spacing is the subnormals'
    2^-133.  ``truncate``: round toward zero instead (what the tests make sure a kernel is NOT doing)."""
    x = torch.as_tensor(x, dtype=torch.float64)
    finite = torch.isfinite(x)
    safe = torch.where(finite, x, torch.zeros_like(x))
    r = _rd_bits(safe, not truncate)
    sub = safe.abs() < 2.0 ** -126
    q = safe * 2.0 ** 133
    r = torch.where(sub, (torch.trunc(q) if truncate else torch.round(q)) * 2.0 ** -133, r)     # torch.round: half to even
    r = torch.where(r.abs() > BF16_MAX, torch.copysign(torch.full_like(r, float("inf")), r), r)
    return torch.where(finite, r, x)


def representable(x):
    return rd(x) == torch.as_tensor(x, dtype=torch.float64)


def _cpu64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


# ---- lattice data: the result is determined bit for bit ----------------------------------------------------------------------
class _AllRepresentable(AssertionError):
    pass


def lattice(m, k0, widths, acts, seed, nnz=16, device="cpu", tries=40):
    """_lattice() at the first seed from ``seed`` on whose hidden layers each hold a value that is not bf16-representable."""
    for s in range(seed, seed + tries):
        try:
            return _lattice(m, k0, widths, acts, s, nnz, device)
        except _AllRepresentable as e:
            last = e
    raise AssertionError(f"no seed in [{seed}, {seed + tries}): {last}")


def _lattice(m, k0, widths, acts, seed, nnz, device):
    """-> (x [m, k0] f32, layers [(W, b, act)] f32, want [m, n_last] float64): integer x in mlp_ref.make_data's pattern (row r % 5 == 2
    all zero, row r % 7 == 4 at +-64, a last column that is never 0 elsewhere), W in {-1, 0, +1} with <= nnz non-zeros per row that
    always include the last column (the FIRST layer of a 2-layer chain is dense), integer biases; ``acts``: 'none' / 'relu' on hidden
    layers, anything on the last ('tanh': the last layer is scaled by a power of two so that |z| <= 2).  Asserts the two conditions of
    this module's docstring."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    sign = lambda *s: ri(0, 1, *s) * 2 - 1
    x = ri(-4, 4, m, k0)
    if k0 > 0:
        x[:, -1] = sign(m) * ri(1, 4, m)
    r = torch.arange(m)
    x[r % 5 == 2] = 0.0
    big = r % 7 == 4
    x[big] = 64.0 * sign(int(big.sum()), k0)
    assert all(a in ("none", "relu") for a in acts[:-1]), "hidden activations must keep the lattice: none / relu"
    layers, k = [], k0
    for i, (n, act) in enumerate(zip(widths, acts)):
        if i == 0 and len(widths) == 2:
            w = ri(-1, 1, n, k)                                          # dense
        else:
            w = torch.zeros(n, k, dtype=torch.float64)
            for row in range(n):
                cols = torch.randperm(k, generator=g)[:max(nnz - 1, 0)]
                w[row, cols] = sign(len(cols))
        if k > 0:
            w[:, -1] = sign(n)
        layers.append([w, ri(-400, 400, n), act])
        k = n
    # the forward in float64, with the two assertions
    h = x.clone()
    last = len(layers) - 1
    for i, (w, b, act) in enumerate(layers):
        assert bool(representable(w).all()) and bool(representable(h).all())
        mag = h.abs() @ w.abs().T + b.abs()
        assert float(mag.max()) < 2.0 ** 24, f"layer {i}: a partial sum may reach {float(mag.max()):.3g} >= 2^24"
        z = h @ w.T + b
        if i == last and act == "tanh":
            s = 2.0 ** -max(int(np.ceil(np.log2(max(float(z.abs().max()), 1.0)))) - 1, 0)
            layers[i][0], layers[i][1] = w * s, b * s
            z = z * s
        h = R.act64(z, act)
        if i < last:
            if bool(representable(h).all()):
                raise _AllRepresentable(f"layer {i}: every hidden value is bf16-representable (truncation would pass)")
            h = rd(h)
    if acts[-1] == "leakyrelu":
        h = h.float().double()                                           # one f32 multiply, rounded once
    f32 = lambda t: t.float().to(device)
    return f32(x), [(f32(w), f32(b), act) for w, b, act in layers], h


def check_exact(y, want, act_last, label=""):
    """y == want on every element (a tanh head: within 8 u |want|)."""
    y = _cpu64(y)
    if act_last in ("tanh", "elu"):
        bad = ~((y - want).abs() <= 8 * R.U * want.abs() + R.TINY)
    else:
        bad = ~(y == want)
    if bool(bad.any()):
        idx = tuple(int(i) for i in torch.nonzero(bad)[0])
        raise AssertionError(f"{label}: {int(bad.sum())} of {y.numel()} outputs differ from the exact result; first at {idx}: "
                             f"got {float(y[idx])!r}, want {float(want[idx])!r}")


# ---- arbitrary data: float64 reference with an interval bound ------------------------------------------------------------------
def reference(x, layers, rounding=rd, e0=None):
    """-> (y, e) float64 on the CPU: the bf16 chain's forward of ``layers`` [(W, b, act)] on x and a bound |kernel - y| <= e.
    ``e0``: a bound on the error of x itself (x is the output of earlier chains), carried through the input rounding."""
    h = _cpu64(x)
    e = torch.zeros_like(h) if e0 is None else _cpu64(e0)
    h, e = rounding(h), rounding(h + e) - rounding(h - e)
    last = len(layers) - 1
    for i, (w, b, act) in enumerate(layers):
        w64 = rounding(_cpu64(w))
        aw = w64.abs()
        b64 = _cpu64(b) if b is not None else torch.zeros(w.shape[0], dtype=torch.float64)
        z = h @ w64.T + b64
        bz = e @ aw.T + R.gamma(w.shape[1] + 18) * ((h.abs() + e) @ aw.T + b64.abs())
        h = R.act64(z, act)
        e = bz + 8 * R.U * h.abs() + R.TINY
        if i < last:
            lo, hi = rounding(h - e), rounding(h + e)
            h, e = rounding(h), hi - lo
    return h, e


def check(y, want, bound, label=""):
    """|y - want| <= bound everywhere -> the worst |y - want| / bound."""
    y = _cpu64(y)
    R.check(y, want, bound, label)
    return float(((y - want).abs() / bound).max())


def rejected(x, layers, want, bound):
    """Names of mlp_ref.mutations that move some output by more than twice the bound -> {name: worst distance / (2 bound)}."""
    out = {}
    for name, (xm, lm) in R.mutations(x, layers).items():
        ym, _ = reference(xm, lm)
        out[name] = float(((ym - want).abs() / (2 * bound)).max())
    return out


# ---- an f32 emulation of the kernels' arithmetic with a chosen summation order ------------------------------------------------
def emulate(x, layers, chunk=32, reverse=False, truncate=False):
    """The arithmetic of rover_step.h in numpy float32: bf16-rounded operands, f32 products (exact), f32 sums over k in chunks of
    ``chunk`` taken in forward or reverse order, f32 bias and activation, bf16 rounding between layers -> float64 tensor."""
    r32 = lambda t: rd(_cpu64(t), truncate).numpy().astype(np.float32)
    h = r32(x)
    last = len(layers) - 1
    for i, (w, b, act) in enumerate(layers):
        w32 = r32(w)
        k = w32.shape[1]
        acc = np.zeros((h.shape[0], w32.shape[0]), dtype=np.float32)
        starts = list(range(0, k, chunk))
        for s in (reversed(starts) if reverse else starts):
            cols = range(s, min(s + chunk, k))
            for c in (reversed(cols) if reverse else cols):
                acc = acc + h[:, c:c + 1] * w32[:, c][None, :]
        z = acc + (b.detach().cpu().numpy().astype(np.float32) if b is not None else np.float32(0))
        z = torch.from_numpy(z)
        if act == "leakyrelu":
            a = torch.where(z > 0, z, torch.tensor(np.float32(0.01)) * z)
        else:
            a = R.act64(z.double(), act).float()
        h = a.numpy()
        if i < last:
            h = r32(torch.from_numpy(h))
    return torch.from_numpy(h).double()
