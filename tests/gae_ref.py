"""Independent restatement of rover_gae (include/rover_step.h; csrc/rover_rollout.hip) in float64 numpy, the error bound a float32
evaluation is held to, and the traps the GPU tests put round the buffers.  Nothing here is fitted to what a kernel returns.

Definition (restated from a reading of skrl 0.10 / 1.x's compute_gae; this project's definition).  rewards, values [T, E] f32, dones
[T, E] (non-zero = done), last_values [E] f32; gamma and lam are the f32 values the C ABI takes:

    adv = 0;  for t = T-1 .. 0:  nv = values[t+1] (t = T-1: last_values)
        adv = rewards[t] - values[t] + gamma (dones[t] ? 0 : 1) (nv + lam adv);  A[t] = adv
    returns = A + values;   advantages = (A - mean(A)) / (std(A, ddof=1) + 1e-8)

Bound of an f32 evaluation, u = 2^-24, gamma_k = k u / (1 - k u), carried down the recursion (b' = the bound of step t+1, A' its exact
value, g = gamma (1 - done)):

    m_z = g (|nv| + lam |A'|)                          the magnitude the bootstrap term's roundings act on
    e_z = g lam b' + gamma_4 (m_z + g lam b')          lam adv, nv + ., g . — or g nv + (g lam) adv: at most 4 roundings of pieces <= m_z
    b   = e_z + gamma_2 (|r| + |v| + m_z + e_z) + 2^-120        r, -v and z summed in any order: two additions
    returns:  b_ret = b + u (|A| + |v| + b) + 2^-120            one more addition

Moments.  The kernel accumulates (count, mean, M2) of ITS raw A in float64 (u64 = 2^-53): per column sums of d = A - A[T-1] and d^2
(sum d^2 <= (2 + 2 T) sum A^2 of the column), then Chan's pairwise merges, whose M2 update adds non-negative terms only.  No value
passes through more than P = T + ceil(E / 131 072) + 32 merges or additions (a thread's columns, a 6-level lane tree, 8 partials per
thread and an 8-level tree in the finishing kernel, the caller's combine), each of at most 8 roundings:

    |mean_dev - mean64(A_dev)| <= 8 P u64 max|A_dev|            |M2_dev - M2_64(A_dev)| <= 8 P u64 (2 + 2 T) sum A_dev^2

Normalised advantages, n = T E, m and s = std + 1e-8 of the float64 A, out = (A - m) / s.  The device subtracts fl32(mean_dev) and
divides by fl32(std_dev + 1e-8), moments of ITS A (each element within b of the exact one):

    dm  = mean(b) + 8 P u64 max|A|                              ds = sqrt(sum b^2 / (n - 1)) + dM2 / ((n - 1) std)
    e_N = b + dm + u |m|;   e_N' = e_N + u (|A - m| + e_N)      the rounded mean, the subtraction
    e_D = ds + u (s + ds)                                       the rounded denominator
    b_norm = (e_N' + |out| e_D) / (s - e_D) + 2 u |out| + 2^-120      (infinite where s <= e_D: a degenerate rollout)

(|std(x) - std(y)| <= ||x - y|| / sqrt(n - 1) by the triangle inequality on the centred vectors; |sqrt a - sqrt b| <= |a - b| / sqrt b.)
"""
import numpy as np
import torch

U = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -120
CANARY = -31337.0


def gamma_k(k):
    return k * U / (1.0 - k * U)


def f32_param(x):
    """The value the C ABI receives for gamma / lam: rounded to float32."""
    return float(np.float32(x))


def merge_path(T, E):
    return T + (E + 131071) // 131072 + 32


def reference(rewards, values, dones, last_values, gamma=0.99, lam=0.95):
    """-> dict of float64 arrays: A, bA (bound of the raw advantages), returns, b_returns.  Inputs: numpy / torch, [T, E] or [T, E, 1]."""
    as_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    r = as_np(rewards).astype(np.float64)
    v = as_np(values).astype(np.float64)
    d = as_np(dones)
    T, E = r.shape[0], r.shape[1]
    r, v, d = r.reshape(T, E), v.reshape(T, E), d.reshape(T, E) != 0
    lv = as_np(last_values).astype(np.float64).reshape(E)
    g0, lam = f32_param(gamma), f32_param(lam)
    A = np.empty((T, E))
    bA = np.empty((T, E))
    adv, b = np.zeros(E), np.zeros(E)
    for t in range(T - 1, -1, -1):
        nv = v[t + 1] if t < T - 1 else lv
        g = g0 * np.where(d[t], 0.0, 1.0)
        m_z = g * (np.abs(nv) + lam * np.abs(adv))
        e_z = g * lam * b + gamma_k(4) * (m_z + g * lam * b)
        b = e_z + gamma_k(2) * (np.abs(r[t]) + np.abs(v[t]) + m_z + e_z) + TINY
        adv = r[t] - v[t] + g * (nv + lam * adv)
        A[t], bA[t] = adv, b
    ret = A + v
    return {"A": A, "bA": bA, "returns": ret, "b_returns": bA + U * (np.abs(A) + np.abs(v) + bA) + TINY}


def moments(a):
    """(count, mean, M2) of an array in float64 (two-pass)."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    m = a.mean() if a.size else 0.0
    return np.array([float(a.size), m, float(((a - m) ** 2).sum())])


def moments_bound(a_dev, T, E):
    """-> (d_mean, d_M2): how far the device's stats_out may be from moments(a_dev), its own raw A."""
    a = np.asarray(a_dev, dtype=np.float64)
    p = merge_path(T, E)
    return 8 * p * U64 * float(np.abs(a).max()), 8 * p * U64 * (2 + 2 * T) * float((a * a).sum())


def normalized(A, bA, stats=None):
    """-> (out, bound): (A - m) / (std + 1e-8) in float64 and b_norm, m and std those of A itself — or, with ``stats`` = (A, bA) of the
    WHOLE rollout this one is a shard of, the whole's (a shard normalised with the combined moments)."""
    whole_A, whole_b = (A, bA) if stats is None else stats
    T, E = whole_A.shape
    n = whole_A.size
    m = whole_A.mean()
    std = np.sqrt(((whole_A - m) ** 2).sum() / (n - 1))
    s = std + 1e-8
    out = (A - m) / s
    p = merge_path(T, E)
    d_m2 = 8 * p * U64 * (2 + 2 * T) * float(((np.abs(whole_A) + whole_b) ** 2).sum())
    dm = whole_b.mean() + 8 * p * U64 * float((np.abs(whole_A) + whole_b).max())
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.sqrt((whole_b ** 2).sum() / (n - 1)) + (d_m2 / ((n - 1) * std) if std > 0 else np.inf)
        e_n = bA + dm + U * abs(m)
        e_n = e_n + U * (np.abs(A - m) + e_n)
        e_d = ds + U * (s + ds)
        bound = np.where(s > e_d, (e_n + np.abs(out) * e_d) / (s - e_d) + 2 * U * np.abs(out) + TINY, np.inf)
    return out, bound


def check(got, want, bound, label=""):
    """|got - want| <= bound on every element (a NaN in got fails); prints max |d| / bound like the other GPU tests -> that ratio."""
    got = (got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)).astype(np.float64).reshape(want.shape)
    d = np.abs(got - want)
    bad = ~(d <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.nanmax(np.where(bound > 0, d / bound, 0.0))) if d.size else 0.0
    print(f"{label}: max |d| / bound = {ratio:.3f}")
    if bad.any():
        idx = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{label}: {int(bad.sum())} of {d.size} outputs outside the float64 bound; first at {idx}: got {got[idx]!r}, "
                             f"want {want[idx]!r} +- {bound[idx]:.3e}")
    return ratio


# ---- data and traps -----------------------------------------------------------------------------------------------------------------
DONE_PATTERNS = ("none", "all", "random", "last", "first")


def make_case(T, E, pattern="random", scale=1.0, seed=0, rate=0.02):
    """float32 rewards, values [T, E], bool dones [T, E], last_values [E] (numpy), seeded."""
    rng = np.random.default_rng(seed)
    r = (rng.standard_normal((T, E)) * scale).astype(np.float32)
    v = (rng.standard_normal((T, E)) * scale).astype(np.float32)
    lv = (rng.standard_normal(E) * scale).astype(np.float32)
    d = np.zeros((T, E), dtype=bool)
    if pattern == "all":
        d[:] = True
    elif pattern == "random":
        d = rng.random((T, E)) < rate
    elif pattern == "last":
        d[T - 1] = True
    elif pattern == "first":
        d[0] = True
    elif pattern != "none":
        raise ValueError(pattern)
    return r, v, d, lv


def nonfinite_case(T, E, seed=0):
    """make_case("random") with two poisoned columns (T >= 5, E >= 8) -> (r, v, d, lv, cols).  Column cols["inf"]: a +Inf reward at
    t = 3 whose done is set (g = 0 times a finite bootstrap: A = +Inf there), no done at t = 2 (A stays +Inf), a done at t = 1
    (0 * Inf = NaN from there down), none at t = 0 and t = 4.  Column cols["nan"]: a NaN value at t = 2 and no done at all (A is NaN at
    t = 2, where the value is subtracted, and below, where it is the bootstrap)."""
    assert T >= 5 and E >= 8
    r, v, d, lv = make_case(T, E, "random", seed=seed)
    cols = {"inf": E // 3, "nan": E - 1}                                # the last env: at E = 131 073 the one lane of the scan's second trip
    d[:, cols["inf"]] = False
    d[[1, 3], cols["inf"]] = True
    r[3, cols["inf"]] = np.inf
    d[:, cols["nan"]] = False
    v[2, cols["nan"]] = np.nan
    return r, v, d, lv, cols


def cleaned(r, v, d, lv, cols):
    """The same rollout with the two non-finite entries of nonfinite_case made finite; every other element unchanged."""
    r, v = r.copy(), v.copy()
    r[3, cols["inf"]] = 1.0
    v[2, cols["nan"]] = 0.5
    return r, v, d, lv, cols


def reference_nonfinite(rewards, values, dones, last_values, gamma=0.99, lam=0.95):
    """reference() on inputs that hold Inf / NaN: IEEE arithmetic says where A and returns are +-Inf or NaN (0 * Inf = NaN); the
    bounds of those columns mean nothing."""
    with np.errstate(all="ignore"):
        return reference(rewards, values, dones, last_values, gamma, lam)


def nonfinite_pattern(a):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN per element."""
    a = (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)
    return np.select([np.isnan(a), a == np.inf, a == -np.inf], [3, 1, 2], 0)


class Guarded:
    """A [T, E] array of ``dtype`` on ``device`` inside a trap-filled allocation with guard rows before and after and a time stride of
    ``E + pad`` elements (the pad columns hold the trap too).  layout "plain": .t is [T, E]; "skrl": .t is [T, E, 1] (pad must be 0 — the
    shape fixes the stride; the guard rows remain).  fill: the trap value — NaN round inputs, CANARY round outputs."""

    def __init__(self, T, E, device, dtype=torch.float32, pad=0, layout="plain", fill=CANARY, data=None):
        assert layout == "plain" or pad == 0
        stride = E + pad
        self.T, self.E = T, E
        self.fill = fill = True if dtype == torch.bool else (1 if dtype == torch.uint8 else fill)      # a done flag's trap: "done"
        self.buf = torch.full((T + 2, max(stride, 1)), fill, dtype=dtype, device=device)
        self.t = self.buf[1:T + 1, :E]
        if data is not None:
            self.t.copy_(torch.as_tensor(data).to(device))
        if layout == "skrl":
            self.t = self.t.unsqueeze(-1)

    def intact(self):
        """Everything outside the [T, E] window still holds the trap value."""
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        mask[1:self.T + 1, :self.E] = False
        rest = self.buf[mask]
        if self.buf.dtype == torch.float32 and self.fill != self.fill:
            return bool(torch.isnan(rest).all())
        return bool((rest == self.fill).all())

    def untouched(self):
        """The window itself still holds the trap value (an output no kernel wrote)."""
        return bool((self.buf[1:self.T + 1, :self.E] == self.fill).all())
