"""Float64 reference, a rigorous per-element error bound and NaN / canary traps for the policy-net kernels (csrc/rover_mlp.hip).

Every kernel path there computes each layer as fp32 sums of exact fp32 products in some fixed order (an f32-input MFMA is a k-ordered
fmaf chain; split-k adds up to 16 partial sums in a fixed order; the split-k finish layer is a plain fmaf chain), adds the bias and
applies an activation whose Lipschitz constant is <= 1.  With u = 2^-24, gamma_n = n u / (1 - n u) and e_0 = 0, layer by layer:

    B_z = |W| e + gamma_{K+18} (|W| (|h| + e) + |b|)       K + 18: any summation order, up to 16 partial sums and the bias add
    h'  = act(W h + b)                                      in float64, from the exact fp32 inputs, weights and biases
    e'  = B_z + 8 u |h'| + 2^-120                           8 u |h'|: up to 4 ulp of tanhf / expm1f (and the LeakyReLU product)

so |y - h_L| <= e_L on every element, whatever the kernel's summation order.  Torch, on the CPU or the GPU alike.
"""
import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -120
LEAKY_SLOPE = float(np.float32(0.01))          # the kernels' 0.01f
ACTS = ("none", "leakyrelu", "tanh", "relu", "elu")
CANARY = -31337.0


def gamma(n):
    return n * U / (1.0 - n * U)


def act64(z, act):
    if act in (None, "none"):
        return z
    if act == "leakyrelu":
        return torch.where(z > 0, z, LEAKY_SLOPE * z)
    if act == "tanh":
        return torch.tanh(z)
    if act == "relu":
        return torch.clamp_min(z, 0.0)
    if act == "elu":
        return torch.where(z > 0, z, torch.expm1(z))
    raise ValueError(act)


def reference(x, layers):
    """-> (y, e): the float64 forward of ``layers`` [(W [n, k] fp32, b [n] fp32 or None, act)] on x [M, K0] and its error bound."""
    h = x.double()
    e = torch.zeros_like(h)
    for w, b, act in layers:
        aw = w.double().abs()
        b64 = b.double() if b is not None else torch.zeros(w.shape[0], dtype=torch.float64, device=w.device)
        z = h @ w.double().T + b64
        bz = e @ aw.T + gamma(w.shape[1] + 18) * ((h.abs() + e) @ aw.T + b64.abs())
        h = act64(z, act)
        e = bz + 8 * U * h.abs() + TINY
    return h, e


def check(y, want, bound, label=""):
    """|y - want| <= bound on every element (a NaN in y fails)."""
    y = y.double()
    d = (y - want).abs()
    bad = ~(d <= bound)
    if bool(bad.any()):
        idx = tuple(int(i) for i in torch.nonzero(bad)[0])
        raise AssertionError(f"{label}: {int(bad.sum())} of {y.numel()} outputs outside the float64 bound; first at {idx}: "
                             f"got {float(y[idx])!r}, want {float(want[idx])!r} +- {float(bound[idx]):.3e}")


# ---- sensitivity guard: mutated references that a tail / row / bias bug would compute ---------------------------------------
def _neighbour(n):
    """index n ^ 1, clamped to n - 1 (the neighbouring feature or row)."""
    return torch.clamp(torch.arange(n) ^ 1, max=n - 1)


def mutations(x, layers):
    """-> {name: (x', layers')}: the last input column of layer 1 dropped; the bias of feature n of the first (and the last) layer
    read from feature n ^ 1; row r of the input read from row r ^ 1.  Each only where it can change something."""
    out = {}
    w0, b0, a0 = layers[0]
    if w0.shape[1] > 0:
        w = w0.clone()
        w[:, -1] = 0.0
        out["drop_last_column"] = (x, [(w, b0, a0)] + list(layers[1:]))
    for li in sorted({0, len(layers) - 1}):
        w, b, a = layers[li]
        if b is not None and b.numel() > 1:
            mut = list(layers)
            mut[li] = (w, b[_neighbour(b.numel()).to(b.device)], a)
            out[f"bias{li}_neighbour"] = (x, mut)
    if x.shape[0] > 1 and x.shape[1] > 0:
        out["row_neighbour"] = (x[_neighbour(x.shape[0]).to(x.device)], list(layers))
    return out


def insensitive(x, layers, want, bound):
    """Names of the mutations that do NOT move some output by more than twice the bound (a kernel computing the mutated net
    would then pass): empty when the data rejects every one."""
    miss = []
    for name, (xm, lm) in mutations(x, layers).items():
        ym, _ = reference(xm, lm)
        if not bool(((ym - want).abs() > 2 * bound).any()):
            miss.append(name)
    return miss


# ---- data --------------------------------------------------------------------------------------------------------------------
def make_data(m, k0, widths, acts, seed, device):
    """x [m, k0] from [-2, 2] (the last column at magnitude 0.5-2, row r % 5 == 2 exactly 0, row r % 7 == 4 at +-64) and layers
    [(W, b, act)]: W uniform / sqrt(fan_in) (the first layer's last column at magnitude 0.5-1), b from [-1, 1] — the negative
    branches of ReLU / LeakyReLU / ELU and a saturated tanh are all reached."""
    g = torch.Generator(device=device).manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, device=device)
    sign = lambda *s: torch.where(rnd(*s) < 0.5, -1.0, 1.0)
    x = rnd(m, k0) * 4 - 2
    if k0 > 0:
        x[:, -1] = sign(m) * (0.5 + 1.5 * rnd(m))
    r = torch.arange(m, device=device)
    x[r % 5 == 2] = 0.0
    big = r % 7 == 4
    x[big] = 64.0 * sign(int(big.sum()), k0)
    layers, k = [], k0
    for i, (n, act) in enumerate(zip(widths, acts)):
        w = (rnd(n, k) * 2 - 1) / max(k, 1) ** 0.5
        if i == 0 and k > 0:
            w[:, -1] = sign(n) * (0.5 + 0.5 * rnd(n))
        layers.append((w, rnd(n) * 2 - 1, act))
        k = n
    return x, layers


def sensitive_data(m, k0, widths, acts, seed, device, tries=40):
    """make_data() at the first seed from ``seed`` on whose data every mutation is rejected -> (x, layers, want, bound)."""
    for s in range(seed, seed + tries):
        x, layers = make_data(m, k0, widths, acts, s, device)
        want, bound = reference(x, layers)
        if not insensitive(x, layers, want, bound):
            return x, layers, want, bound
    raise AssertionError(f"no seed in [{seed}, {seed + tries}) makes M={m} K0={k0} {widths} {acts} reject every mutation")


# ---- traps -------------------------------------------------------------------------------------------------------------------
def nan_head(t, pad=512):
    """t as the head of a NaN-filled buffer: any read past its end returns NaN."""
    buf = torch.full((t.numel() + pad,), float("nan"), device=t.device)
    buf[:t.numel()] = t.reshape(-1)
    return buf[:t.numel()].view(t.shape)


def trapped_input(x, offset):
    """x as a column slice at ``offset`` (odd) of a wider tensor with an odd row stride, NaN in every other column and in the rows
    past x's."""
    m, k = x.shape
    stride = k + offset + 2
    stride += 1 - stride % 2
    buf = torch.full((m + 5, stride), float("nan"), device=x.device)
    buf[:m, offset:offset + k] = x
    return buf[:m, offset:offset + k]


class Canary:
    """An [m, n] output as a column slice of a CANARY-filled tensor with extra rows and columns (odd row stride)."""

    def __init__(self, m, n, device, offset=1):
        stride = n + offset + 3
        stride += 1 - stride % 2
        self.buf = torch.full((m + 3, stride), CANARY, device=device)
        self.m, self.n, self.off = m, n, offset
        self.y = self.buf[:m, offset:offset + n]

    def intact(self):
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        mask[:self.m, self.off:self.off + self.n] = False
        return bool((self.buf[mask] == CANARY).all())


class Layer:
    """What _lib.Engine.chain_forward reads: .weight, .bias, .activation."""

    def __init__(self, weight, bias, activation):
        self.weight, self.bias, self.activation = weight, bias, activation


def trapped_layers(layers):
    return [Layer(nan_head(w), nan_head(b) if b is not None else None, a) for w, b, a in layers]


def splitk_chunks(m, k):
    """-> (S, chunk): the split-k partition of a first layer of k inputs at m rows (csrc/rover_mlp.hip splitk_chunks)."""
    rt = 2 if m >= 2048 else 1
    tiles = (m + 16 * rt - 1) // (16 * rt)
    s = min(max(min((1024 + tiles - 1) // tiles, (k + 63) // 64), 1), 16)
    c = ((k + s - 1) // s + 15) // 16 * 16
    return (k + c - 1) // c, c
