"""Independent restatement of the exteroception noise (include/rover_step.h, rover_obs_noise; csrc/rover_noise.hip): the draws in numpy
uint32 / float64 on gauss_ref's Philox and on the head's pair formula, and the bound the tests hold the device to.

Definition (normative; the header's).  Columns [0, first) are copied.  For heightmap column c = col - first, global row g, call counter
t, column pair p = c // 2, seed split into key (lo, hi):
    w    = philox4x32_10((g, t & 0xffffffff, t >> 32, 0x60000000 | p), key)
    eps  = the head's pair from (w0, w1): u0 = ((w0 >> 8) + 1) 2^-24, u1 = (w1 >> 8) 2^-24, rad = sqrt(-2 ln u0),
           eps[2p] = rad cos(2 pi u1), eps[2p + 1] = rad sin(2 pi u1)
    u_c  = w2 >> 8 (even c), w3 >> 8 (odd c)
    wo   = philox4x32_10((g, e & 0xffffffff, e >> 32, 0x70000000), key),   e = the row's episode count (0 without one)
    eo   = the cos branch of the pair from (wo0, wo1)
    v    = (in + (sigma_offset s) eo) + (sigma_point s) eps_c;     out = drop_value where u_c < thr = rint(dropout 2^24), else v
A sigma of 0 switches its term off (+0.0, no draw), so all-off returns the input with -0.0 turned into +0.0.

Bound of the device's f32 result against this float64 one, u = 2^-24 (gauss_ref.U).  sigma_point, sigma_offset, s and `in` are f32
values and enter both sides exactly.  The device's eps_c and eo are within gauss_ref.noise_bound(rad) of the draws above (derived there:
16 u (1 + rad)), which moves v by at most
    s (sigma_point noise_bound(rad_c) + sigma_offset noise_bound(rad_o)).
The formula then writes four products and two sums, each rounded once (relative u):
    a_p = sigma_point s, t_p = a_p eps: |t_p| carries 2 u;  a_o, t_o likewise;  s1 = in + t_o: u |s1|;  v = s1 + t_p: u |v|
    rounding <= u (2 |t_p| + 2 |t_o| + |in + t_o| + |v|) (1 + 4 u)
(1 + 4 u covers the products of two relative errors; |t_p| and |t_o| are taken with |eps| + noise_bound, the device's own values at
most.)  TINY = 2^-120 is added for results in the subnormal range.  Nothing here is fitted to a measurement."""
import numpy as np

import gauss_ref as G

U = G.U
TINY = G.TINY
WORD3_POINT = 0x60000000
WORD3_OFFSET = 0x70000000
SEED_STAT = 0x0B5E55ED5EED         # the one seed of the host statistics (tests/test_obs_noise_host.py)


def threshold(dropout):
    """thr: the integer a 24-bit dropout word is compared with (llrint: round half to even, as np.rint)."""
    return int(np.rint(np.float64(dropout) * 16777216.0))


def _key(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed & 0xffffffff, seed >> 32


def _pair(w0, w1):
    """The head's Box-Muller pair (gauss_ref.noise's formula) from two word arrays -> (cos branch, sin branch, rad) float64."""
    u0 = ((w0 >> np.uint32(8)).astype(np.float64) + 1.0) * U
    u1 = (w1 >> np.uint32(8)).astype(np.float64) * U
    rad = np.sqrt(-2.0 * np.log(u0))
    return rad * np.cos(2.0 * np.pi * u1), rad * np.sin(2.0 * np.pi * u1), rad


def point_words(seed, t, rows, n_pairs):
    """-> four uint32 arrays [n, n_pairs]: Philox on (g, t lo, t hi, 0x60000000 | p) for global rows ``rows`` and pairs 0 .. n_pairs."""
    t = int(t) & (2 ** 64 - 1)
    g = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    p = np.arange(n_pairs, dtype=np.uint64).reshape(1, -1)
    shape = np.broadcast(g, p).shape
    return G.philox4x32_10((np.broadcast_to(g, shape), t & 0xffffffff, t >> 32, np.uint64(WORD3_POINT) | np.broadcast_to(p, shape)), _key(seed))


def point_draws(seed, t, rows, c):
    """-> (eps [n, c], rad [n, c] float64, u [n, c] uint32: the 24-bit dropout words) for heightmap columns 0 .. c."""
    n_pairs = (c + 1) // 2
    n = len(np.asarray(rows).reshape(-1))
    eps, rad, u = np.zeros((n, 2 * n_pairs)), np.zeros((n, 2 * n_pairs)), np.zeros((n, 2 * n_pairs), dtype=np.uint32)
    if n_pairs and n:
        w = point_words(seed, t, rows, n_pairs)
        eps[:, 0::2], eps[:, 1::2], r = _pair(w[0], w[1])
        rad[:, 0::2], rad[:, 1::2] = r, r
        u[:, 0::2], u[:, 1::2] = w[2] >> np.uint32(8), w[3] >> np.uint32(8)
    return eps[:, :c], rad[:, :c], u[:, :c]


def offset_words(seed, episode, rows):
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1)
    e = np.asarray(episode, dtype=np.int64).astype(np.uint64) * np.ones_like(rows)
    return G.philox4x32_10((rows, e & np.uint64(0xffffffff), e >> np.uint64(32), WORD3_OFFSET), _key(seed))


def offset_draws(seed, episode, rows):
    """-> (eo [n], rad_o [n]) float64: one draw per global row and episode count (``episode``: a scalar or an int64 array [n])."""
    w = offset_words(seed, episode, rows)
    eo, _, rad = _pair(w[0], w[1])
    return eo, rad


def reference(x, first, sigma_point=0.0, sigma_offset=0.0, dropout=0.0, drop_value=0.0, row_scale=None, episode=None, seed=0, t=0,
              row_offset=0):
    """x [M, F] float32 -> (want [M, F] float64, bound [M, F] float64, dropped [M, F] bool).  ``want`` holds drop_value where
    ``dropped``; the proprioceptive columns and the dropped elements have bound 0 (they are exact)."""
    x = np.asarray(x, dtype=np.float32)
    m, f = x.shape
    c = f - first
    sp, so, dv = float(np.float32(sigma_point)), float(np.float32(sigma_offset)), float(np.float32(drop_value))
    rows = np.arange(m, dtype=np.uint64) + np.uint64(row_offset)
    s = np.ones(m) if row_scale is None else np.asarray(row_scale, dtype=np.float32).astype(np.float64)
    want, bound, dropped = x.astype(np.float64), np.zeros((m, f)), np.zeros((m, f), dtype=bool)
    if c == 0 or m == 0:
        return want, bound, dropped
    eps, rad, u = point_draws(seed, t, rows, c)
    eo, rad_o = offset_draws(seed, 0 if episode is None else episode, rows)
    xin = want[:, first:]
    a_p, a_o = (sp * s)[:, None], (so * s)[:, None]
    t_p = a_p * eps if sp != 0.0 else np.zeros_like(eps)
    t_o = a_o * eo[:, None] if so != 0.0 else np.zeros((m, 1))
    v = (xin + t_o) + t_p
    nb_p = np.abs(a_p) * G.noise_bound(rad) if sp != 0.0 else 0.0
    nb_o = np.abs(a_o) * G.noise_bound(rad_o)[:, None] if so != 0.0 else 0.0
    tp_hi, to_hi = np.abs(t_p) + nb_p, np.abs(t_o) + nb_o
    rounding = U * (2.0 * tp_hi + 2.0 * to_hi + (np.abs(xin) + to_hi) + (np.abs(xin) + to_hi + tp_hi)) * (1.0 + 4.0 * U)
    b = nb_p + nb_o + rounding + TINY
    drop = u < np.uint32(threshold(dropout))
    want[:, first:] = np.where(drop, dv, v)
    bound[:, first:] = np.where(drop, 0.0, b)
    dropped[:, first:] = drop
    return want, bound, dropped


def evaluate_f32(x, first, sigma_point=0.0, sigma_offset=0.0, dropout=0.0, drop_value=0.0, row_scale=None, episode=None, seed=0, t=0,
                 row_offset=0):
    """The formula in numpy float32, one rounding per written operation, on the float64 draws rounded to f32 (a rounding of u |eps|,
    inside noise_bound): what a correct f32 kernel may return.  -> out [M, F] float32."""
    x = np.asarray(x, dtype=np.float32)
    m, f = x.shape
    c = f - first
    out = x.copy()
    if c == 0 or m == 0:
        return out
    rows = np.arange(m, dtype=np.uint64) + np.uint64(row_offset)
    s = np.ones(m, dtype=np.float32) if row_scale is None else np.asarray(row_scale, dtype=np.float32)
    eps, _, u = point_draws(seed, t, rows, c)
    eo, _ = offset_draws(seed, 0 if episode is None else episode, rows)
    sp, so = np.float32(sigma_point), np.float32(sigma_offset)
    t_o = ((so * s) * eo.astype(np.float32))[:, None] if so != 0 else np.zeros((m, 1), dtype=np.float32)
    t_p = (sp * s)[:, None] * eps.astype(np.float32) if sp != 0 else np.zeros((m, c), dtype=np.float32)
    v = (x[:, first:] + t_o) + t_p
    assert v.dtype == np.float32
    out[:, first:] = np.where(u < np.uint32(threshold(dropout)), np.float32(drop_value), v)
    return out
