"""The running standard scaler as DEFINED (include/rover_step.h, rover_scaler_update / rover_scaler_apply; skrl's RunningStandardScaler,
restated: skrl is not installed) in numpy, the error bound of the device's moment reduction with its derivation, and KLAdaptiveRL's rule.

Statistics: float64.  Forward / inverse: float32 with one rounding per operation, in the written order.

The bound.  u = 2^-53, g(k) = k u / (1 - k u).  The device forms, per chunk of rows and per column, S1 = sum x and S2 = sum x*x in f64
(x widened first, so every product is exact); every x reaches its sum through at most A = 136 additions (wide route: a thread walks at
most 128 rows in order; narrow route: at most 64 rows per thread, then 8 levels of a binary tree).  Hence, per chunk,
    |dS1| <= g(A) sum|x|          |dS2| <= g(A) sum x^2
and for mean = S1 / n, M2 = S2 - (S1 S1) / n (three more roundings, S1^2 / n <= sum x^2 by Cauchy-Schwarz, and the error of S1 enters
S1^2 / n as 2 |S1| |dS1| / n <= 2 g(A) (sum|x|)^2 / n <= 2 g(A) sum x^2):
    |d mean| <= g(A + 1) sum|x| / n          |d M2| <= 4 g(A + 3) sum x^2.
The max(., 0) on M2 only moves a negative (impossible exactly) value towards the truth.  The C chunks are merged in order by Chan's
update; one merge makes at most 5 roundings on M2, each relative to a quantity of at most 2 sum x^2 (a sum of squares about a point of the
data's hull is at most sum x^2 + n mean^2 <= 2 sum x^2) — 10 u sum x^2 —, and at most 4 on the mean, each relative to at most sum|x| / n.
The chunk errors add (the merge is linear in M2_k, and its mean terms are convex combinations).  Over the whole batch:
    |d mb|  <= (g(A + 1) + 4 C u) sum|x| / M
    |d M2b| <= (4 g(A + 3) + 10 C u) sum x^2  +  2 M |mb| |d mb| + M |d mb|^2        (the mean's error moves the point M2 is taken about)
The fold into the state is the same dozen f64 operations here and on the device, so its own rounding is at most 8 u of each result,
and the batch's errors enter it linearly:
    |d mean'| <= |d mb| M / total + 8 u |mean'|
    |d var'|  <= (|d M2b| M / (M - 1) + 2 |delta| |d mb| count M / total) / total + 8 u var'
The restatement itself (two passes, numpy's pairwise sums along a contiguous axis, in long double where there is one) errs by at most
g(log2(M) + 8) of the same quantities even in plain float64; that is added.
"""
import math

import numpy as np

U = 2.0 ** -53
A = 136


def g(k):
    return k * U / (1.0 - k * U)


def fresh(size):
    """skrl's initial state: (running_mean, running_variance, current_count)."""
    return np.zeros(size, dtype=np.float64), np.ones(size, dtype=np.float64), 1.0


def batch_moments(x):
    """Column means and UNBIASED variances of x [M, N] in float64 (torch.mean / torch.var over dim 0)."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    # numpy sums pairwise only along the contiguous axis (down the rows of a [M, N] array it accumulates naively, and M equal terms then
    # round the same way M times): one column per contiguous row, in long double where the platform has one
    xt = np.ascontiguousarray(x.T).astype(np.longdouble)
    mb = xt.sum(axis=1) / x.shape[0]
    vb = ((xt - mb[:, None]) ** 2).sum(axis=1) / (x.shape[0] - 1)
    return mb.astype(np.float64), vb.astype(np.float64)


def update(state, x):
    """One train call: the definition's formula, operation for operation, in float64 -> the new (mean, var, count)."""
    mean, var, count = state
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    M = float(x.shape[0])
    if M < 2:
        raise ValueError("a train call needs at least 2 rows")
    mb, vb = batch_moments(x)
    delta = mb - mean
    total = count + M
    m2 = var * count + vb * M + delta ** 2 * count * M / total
    return mean + delta * M / total, m2 / total, total


def forward(x, mean, var, epsilon=1e-8, clip=5.0):
    """y = clamp((x - f32(mean)) / (sqrt(f32(var)) + f32(eps)), -clip, clip) in float32; a NaN stays a NaN (np.clip propagates it)."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    with np.errstate(all="ignore"):
        scale = np.sqrt(np.asarray(var).astype(f)) + f(epsilon)
        return np.clip((x - np.asarray(mean).astype(f)) / scale, f(-clip), f(clip)).astype(f)


def inverse(x, mean, var, clip=5.0):
    """y = sqrt(f32(var)) * clamp(x, -clip, clip) + f32(mean) in float32."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    with np.errstate(all="ignore"):
        return (np.sqrt(np.asarray(var).astype(f)) * np.clip(x, f(-clip), f(clip)) + np.asarray(mean).astype(f)).astype(f)


def moment_bound(M, sum_abs, sum_sq, n_chunks, mb=None):
    """(|d mb|, |d M2b|) of the device's batch moments per column, from M, sum|x|, sum x^2 and the plan's chunk count (derivation above),
    plus the restatement's own error."""
    sum_abs, sum_sq = np.asarray(sum_abs, dtype=np.float64), np.asarray(sum_sq, dtype=np.float64)
    own = g(math.log2(max(M, 2)) + 8)
    d_mb = (g(A + 1) + 4 * n_chunks * U + own) * sum_abs / M
    mb = sum_abs / M if mb is None else np.abs(mb)
    d_m2 = (4 * g(A + 3) + 10 * n_chunks * U + 4 * own) * sum_sq + 2 * M * mb * d_mb + M * d_mb ** 2
    return d_mb, d_m2


def update_bound(state, x, n_chunks):
    """(|d mean'|, |d var'|) per column of one train call on x from ``state`` (derivation above)."""
    mean, var, count = state
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    M = float(x.shape[0])
    mb, _ = batch_moments(x)
    d_mb, d_m2 = moment_bound(M, np.abs(x).sum(axis=0), (x * x).sum(axis=0), n_chunks, mb)
    new_mean, new_var, total = update(state, x)
    delta = np.abs(mb - mean)
    d_mean = d_mb * M / total + 8 * U * np.abs(new_mean)
    d_var = (d_m2 * M / (M - 1) + 2 * delta * d_mb * count * M / total) / total + 8 * U * new_var
    return d_mean, d_var


CAP = 1e-9          # the bound is never allowed above CAP * (var + mean^2): a loose derivation cannot hide a wrong kernel


def capped(d_mean, d_var, new_mean, new_var):
    """The bounds the GPU tests use: the derived ones, capped at CAP relative to var + mean^2 (for the mean: to its square root)."""
    scale = new_var + new_mean ** 2
    return np.minimum(d_mean, CAP * np.sqrt(scale)), np.minimum(d_var, CAP * scale)


def kl_adaptive(lr, kl, kl_threshold=0.008, min_lr=1e-6, max_lr=1e-2, kl_factor=2, lr_factor=1.5):
    """skrl's KLAdaptiveRL: one step of the learning rate for the epoch's mean KL."""
    if kl > kl_threshold * kl_factor:
        return max(lr / lr_factor, min_lr)
    if kl < kl_threshold / kl_factor:
        return min(lr * lr_factor, max_lr)
    return lr
