"""Float64 reference and a derived per-element error bound for the optimiser step (csrc/rover_optim.hip, rover_optim_step of
include/rover_step.h): the total gradient norm, the clip coefficient, one Adam step.  Torch on the CPU, no project code.

Reference (step64).  All in float64 on the exact f32 inputs p, m, v, g (lists of tensors), t = the step count AFTER the increment:
    norm = sqrt(sum of g^2 over all tensors);  coef = clip > 0 ? min(1, clip / (norm + 1e-6)) : 1
    g' = g coef;  m' = m + (g' - m)(1 - beta1);  v' = beta2 v + (1 - beta2) g' g'
    bc1 = 1 - beta1^t;  bc2 = 1 - beta2^t;  p' = p - (lr / bc1) (m' / (sqrt(v') / sqrt(bc2) + eps))

Bound (bounds).  The implementation evaluates the same expressions in f32, one rounding per written operation, with the seven scalars
coef, 1 - beta1, beta2, 1 - beta2, lr / bc1, sqrt(bc2), eps rounded to f32 once (each then carries a relative error of at most u =
2^-24; their float64 evaluation — repeated squaring against pow, the order of the norm's sum — differs by some 2^-50, which the
second-order factor below swallows).  fl(x op y) = (x op y)(1 + d), |d| <= u, for +, -, *, / and sqrt (correctly rounded).  Every E_x
below bounds |computed x - exact x|; terms of second order in u are covered by one factor K = 1.01 at the end, which needs e_c u <<
1e-2 (asserted).  Writing G = |g| coef:

  coef  The norm the implementation uses has a relative error of at most e_norm u (e_norm_f64() for the kernels, whose norm is an f64
        sum of exact squares; e_norm_f32() for an implementation that sums in f32 in any order); x -> min(1, clip / (x + 1e-6)) does
        not amplify a relative error, the rounding to f32 adds u:  rel(coef) <= e_c u,  e_c = e_norm + 1.
        e_c = 0 where the coefficient is 1 whatever the norm's error does (clip <= 0, or clip / (norm (1 + 2 e_norm u) + 1e-6) >= 1).
  g'    E_g  = (e_c + 1) u G                                            coef's error, one product
  d = g' - m:   E_d = E_g + u (|d| + E_g)
  x = d (1 - beta1):   E_x = (1 - beta1) (E_d + 2 u (|d| + E_d))          the rounded scalar, one product
  m'    E_m  = E_x + u (|m'| + E_x)                                       (a fused multiply-add rounds once less: inside this)
  a = beta2 v:  E_a = 2 u beta2 |v|                                       the rounded scalar, one product
  b = ((1 - beta2) g') g':  E_b = (2 e_c + 5) u b                         the rounded scalar, g' twice (e_c + 1 each), two products
  v'    E_v  = E_a + E_b + u (v' + E_a + E_b)
  s = sqrt(v'):  |sqrt(x^) - sqrt(x)| = |x^ - x| / (sqrt(x^) + sqrt(x)) <= E_v / (sqrt(v') + sqrt(max(v' - E_v, 0)));
        E_s  = that + u (s + that)                                        (E_v > 0 only where v' > 0; 0 / 0 is taken as 0)
  q = s / sqrt(bc2):  E_q = (E_s + 3 u (s + E_s)) / sqrt(bc2)             the rounded scalar, one division, and one more u so that a
                                                                          multiplication by a rounded reciprocal is inside too
  den = q + eps:  E_den = E_q + u eps + u (den + E_q + u eps)
  r = m' / den:   E_r0 = (E_m + |r| E_den) / (den - E_den);  E_r = E_r0 + u (|r| + E_r0)          (den >= eps > E_den: asserted)
  y = (lr / bc1) r:  E_y = (lr / bc1) (E_r + 3 u (|r| + E_r))             the rounded scalar, one product, one u of slack as for q
  p'    E_p  = E_y + u (|p'| + E_y)

and B_m = K E_m + TINY, B_v = K E_v + TINY, B_p = K E_p + TINY.  Underflow is not modelled: the tests' data keeps every non-zero
intermediate a normal f32 number (a zero gradient on zero state stays exactly zero through every line, and E = 0 there)."""
import torch

U = 2.0 ** -24
TINY = 2.0 ** -120
K = 1.01


def e_norm_f64(n_elements):
    """rel(norm) / u of the kernels' norm: the squares of f32 numbers are exact in f64, their f64 sum in any order is within n 2^-53
    relative, the sqrt halves that and adds 2^-53; the + 1e-6 and the division add 2 more: (n + 4) 2^-53 / u covers it."""
    return (n_elements + 4.0) * 2.0 ** -53 / U


def e_norm_f32(n_elements, n_tensors):
    """rel(norm) / u of an implementation that squares and sums in f32 in ANY order, per tensor, and then takes the norm of the
    tensors' norms (torch's clip_grad_norm_): a sum of n rounded squares is within (n + 1) u, its sqrt halves that and adds u; the
    squares of the n_tensors norms carry twice that plus u, their sum n_tensors u more, its sqrt halves and adds u; + 1e-6 and the
    division add 2 u: (n + n_tensors) / 2 + 6 covers it."""
    return (n_elements + n_tensors) / 2.0 + 6.0


def total_norm64(g):
    return float(torch.sqrt(sum((x.double() ** 2).sum() for x in g)))


def coef64(norm, clip):
    return min(1.0, clip / (norm + 1e-6)) if clip > 0 else 1.0


def step64(p, m, v, g, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, clip=0.0):
    """-> (p', m', v') as lists of float64 tensors, norm, coef."""
    norm = total_norm64(g)
    c = coef64(norm, clip)
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    P, M, V = [], [], []
    for pi, mi, vi, gi in zip(p, m, v, g):
        gc = gi.double() * c
        m2 = mi.double() + (gc - mi.double()) * (1.0 - beta1)
        v2 = beta2 * vi.double() + (1.0 - beta2) * gc * gc
        P.append(pi.double() - (lr / bc1) * (m2 / (torch.sqrt(v2) / bc2 ** 0.5 + eps)))
        M.append(m2)
        V.append(v2)
    return P, M, V, norm, c


def bounds(p, m, v, g, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, clip=0.0, e_norm=None):
    """-> (B_p, B_m, B_v) as lists of float64 tensors: the bounds of the module docstring for one step from exact f32 inputs."""
    u = U
    if e_norm is None:
        e_norm = e_norm_f64(sum(x.numel() for x in g))
    norm = total_norm64(g)
    c = coef64(norm, clip)
    sure_one = clip <= 0 or clip / (norm * (1.0 + 2.0 * e_norm * u) + 1e-6) >= 1.0
    e_c = 0.0 if sure_one else e_norm + 1.0
    assert e_c * u < 1e-3
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    w1, w2, S, r2 = 1.0 - beta1, 1.0 - beta2, lr / bc1, bc2 ** 0.5
    BP, BM, BV = [], [], []
    for pi, mi, vi, gi in zip(p, m, v, g):
        pi, mi, vi, gi = pi.double(), mi.double(), vi.double(), gi.double()
        G = gi.abs() * c
        gc = gi * c
        E_g = (e_c + 1.0) * u * G
        d = gc - mi
        E_d = E_g + u * (d.abs() + E_g)
        E_x = w1 * (E_d + 2.0 * u * (d.abs() + E_d))
        m2 = mi + d * w1
        E_m = E_x + u * (m2.abs() + E_x)
        a, b = beta2 * vi, w2 * G * G
        E_a, E_b = 2.0 * u * a.abs(), (2.0 * e_c + 5.0) * u * b
        v2 = a + b
        E_v = E_a + E_b + u * (v2 + E_a + E_b)
        s = torch.sqrt(v2)
        den_s = s + torch.sqrt(torch.clamp(v2 - E_v, min=0.0))
        e_s0 = torch.where(den_s > 0, E_v / torch.where(den_s > 0, den_s, torch.ones_like(den_s)), torch.zeros_like(E_v))
        E_s = e_s0 + u * (s + e_s0)
        q = s / r2
        E_q = (E_s + 3.0 * u * (s + E_s)) / r2
        den = q + eps
        E_den = E_q + u * eps + u * (den + E_q + u * eps)
        assert bool((den > 2.0 * E_den).all()) or den.numel() == 0
        r = m2 / den
        E_r0 = (E_m + r.abs() * E_den) / (den - E_den)
        E_r = E_r0 + u * (r.abs() + E_r0)
        E_y = S * (E_r + 3.0 * u * (r.abs() + E_r))
        p2 = pi - S * r
        E_p = E_y + u * (p2.abs() + E_y)
        BP.append(K * E_p + TINY)
        BM.append(K * E_m + TINY)
        BV.append(K * E_v + TINY)
    return BP, BM, BV


# the parameter tensors of the two native-width nets in PPO's order (learning/model.py state_dict(): the actor's log_std_parameter, then
# per net both encoders and the MLP, weight then bias): 634 sparse + 1 112 dense + 4 proprioceptive inputs, 2 actions / 1 value
def native_numel():
    out = []
    for n_out, log_std in ((2, True), (1, False)):
        if log_std:
            out.append(n_out)
        for k, n in ((634, 80), (80, 60), (1112, 80), (80, 60), (124, 256), (256, 160), (160, 128), (128, n_out)):
            out += [n * k, n]
    return out
