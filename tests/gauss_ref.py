"""Independent restatement of the actor's Gaussian head (include/rover_step.h, rover_gauss_head; csrc/rover_mlp.hip gaussian_head):
the noise in numpy, the distribution in float64 ``torch.distributions.Normal``, and the bounds the tests hold the device to.

Noise (normative).  Philox4x32-10 (Salmon et al. 2011) on counter (g, t & 0xffffffff, t >> 32, 0x50000000 | p), key (seed lo, seed hi)
for global row g, call counter t, component pair p = j // 2; u0 = ((w0 >> 8) + 1) 2^-24 in (0, 1], u1 = (w1 >> 8) 2^-24 in [0, 1);
rad = sqrt(-2 ln u0); eps[2p] = rad cos(2 pi u1), eps[2p + 1] = rad sin(2 pi u1).  u0 >= 2^-24, so |eps| <= sqrt(48 ln 2) = EPS_MAX.

Caps on the generator at N = 2^20 samples (conditions on the DEFINITION, each 6 standard errors of an ideal N(0, 1) sample):
    |mean| <= 6 / sqrt(N) = 0.0059         |var - 1| <= 6 sqrt(2 / N) = 0.0083         |correlation| <= 6 / sqrt(N) = 0.0059
    KS distance to Phi <= sqrt(ln(2 / 1e-9) / (2 N)) = 0.0032      (the 1e-9 critical value of the one-sample statistic)

Device noise against this restatement, u = 2^-24, one ulp <= 2 u relative.  The kernel takes the angle in half turns (sincospif(2 u1),
2 u1 exact), so no rounding of 2 pi u1 enters.  With logf and sincospif within 2 ulp, sqrtf and the products correctly rounded:
rad carries (4 u) / 2 + u = 3 u relative, the sine / cosine 4 u of a value <= 1, the product u: |eps_dev - eps| <= (3 + 4 + 1) u rad
= 8 u rad.  NOISE_ULPS = 16 states that with a factor 2 of room, as 16 u (1 + rad) — half of the 32 u (1 + rad) that a formulation
rounding the angle would need.

Head arithmetic (x: the returned or the taken f32 action, sigma = exp(ls') in float64, z = (x - mean) / sigma):
    |actions - (mean + sigma eps_dev)|  <= 4 u (|mean| + sigma |eps_dev|)      expf <= 1 ulp = 2 u, a product, a sum
    per-term     b_j = 16 u (z_j^2 / 2 + |ls'_j| + 0.9190) + 2^-120            one rounding in x - mean, <= 2 ulp in expf, a quotient,
                                                                               a square, the three-term sum and the reduction's adds
    "sum"   sum_j b_j        "mean"  sum_j b_j / A        "max" / "min"  max_j b_j  (|max a - max b| <= max |a_j - b_j|)
    None    b_j per element  "prod"  prod_j (|t_j| + b_j) - prod_j |t_j| + A u prod_j (|t_j| + b_j)   (A - 1 rounded products)
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -120
EPS_MAX = math.sqrt(48.0 * math.log(2.0))            # 5.7681
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)         # 0.91894
NOISE_ULPS = 16.0
N_STAT = 1 << 20
CAP_MEAN = 6.0 / math.sqrt(N_STAT)
CAP_VAR = 6.0 * math.sqrt(2.0 / N_STAT)
CAP_CORR = 6.0 / math.sqrt(N_STAT)
CAP_KS = math.sqrt(math.log(2.0 / 1e-9) / (2.0 * N_STAT))
REDUCTIONS = ("sum", "mean", "prod", "max", "min", None)

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

_M32 = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two -> four uint32 arrays.  Random123's philox4x32 round, ten times."""
    c = [np.asarray(v, dtype=np.uint64) & _M32 for v in counter]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & _M32 for v in key)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & _M32, (p0 >> s32) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return [v.astype(np.uint32) for v in c]


def noise(seed, t, rows, a):
    """-> (eps [n, a], rad [n, a]) float64 for global rows ``rows`` (int array), call counter t, a components."""
    rows = np.asarray(rows, dtype=np.uint64)
    seed, t = int(seed) & (2 ** 64 - 1), int(t) & (2 ** 64 - 1)
    eps = np.empty((len(rows), a), dtype=np.float64)
    rad_out = np.empty_like(eps)
    for p in range((a + 1) // 2):
        w = philox4x32_10((rows, t & 0xffffffff, t >> 32, 0x50000000 | p), (seed & 0xffffffff, seed >> 32))
        u0 = ((w[0] >> np.uint32(8)).astype(np.float64) + 1.0) * U
        u1 = (w[1] >> np.uint32(8)).astype(np.float64) * U
        rad = np.sqrt(-2.0 * np.log(u0))
        eps[:, 2 * p] = rad * np.cos(2.0 * np.pi * u1)
        rad_out[:, 2 * p] = rad
        if 2 * p + 1 < a:
            eps[:, 2 * p + 1] = rad * np.sin(2.0 * np.pi * u1)
            rad_out[:, 2 * p + 1] = rad
    return eps, rad_out


def noise_bound(rad):
    return NOISE_ULPS * U * (1.0 + rad)


def ks_distance(x):
    """sup |F_n - Phi| of a 1-d sample."""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = len(x)
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(x) / math.sqrt(2.0))).numpy()
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max(np.max(i / n - cdf), np.max(cdf - (i - 1) / n)))


def corr(a, b):
    return float(np.corrcoef(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))[0, 1])


# ---- the head in float64 ------------------------------------------------------------------------------------------------------------
def clipped_log_std(log_std, clip_log_std=True, min_log_std=-20.0, max_log_std=2.0):
    ls = log_std.double()
    return torch.clamp(ls, min_log_std, max_log_std) if clip_log_std else ls


def actions_reference(mean, ls_c, eps, clip_actions=False, low=-1.0, high=1.0, deterministic=False):
    """-> (want, bound) float64 from the device's own f32 mean and eps."""
    mean, eps = mean.double(), eps.double()
    sigma = torch.exp(ls_c)
    if deterministic:
        return mean, torch.zeros_like(mean)
    want = mean + sigma * eps
    bound = 4.0 * U * (mean.abs() + sigma * eps.abs())
    if clip_actions:
        want = torch.clamp(want, low, high)          # 1-Lipschitz: the bound carries over
    return want, bound


def log_prob_reference(mean, ls_c, x, reduction="sum"):
    """-> (want, bound) float64: Normal(mean_f32, exp(ls')).log_prob(x_f32), reduced over the components as torch would."""
    mean, x = mean.double(), x.double()
    sigma = torch.exp(ls_c).expand_as(mean)
    t = torch.distributions.Normal(mean, sigma).log_prob(x)
    z = (x - mean) / sigma
    b = 16.0 * U * (0.5 * z * z + ls_c.abs() + 0.9190) + TINY
    a = mean.shape[-1]
    if reduction is None:
        return t, b
    if reduction == "sum":
        return t.sum(-1, keepdim=True), b.sum(-1, keepdim=True)
    if reduction == "mean":
        return t.mean(-1, keepdim=True), b.sum(-1, keepdim=True) / a
    if reduction == "prod":
        hi = (t.abs() + b).prod(-1, keepdim=True)
        return t.prod(-1, keepdim=True), hi - t.abs().prod(-1, keepdim=True) + a * U * hi
    if reduction == "max":
        return t.max(-1, keepdim=True).values, b.max(-1, keepdim=True).values
    if reduction == "min":
        return t.min(-1, keepdim=True).values, b.max(-1, keepdim=True).values
    raise ValueError(reduction)
