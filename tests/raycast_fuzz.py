"""The one generator of ray-cast fuzz cases: tools/fuzz_shapes.py (kernel against kernel, any size) and
tests/test_raycast_plans_gpu.py (every kernel against the CPU oracle, bounded) both draw from it."""
import numpy as np
import torch

# (name, raycast_variant, options set after it) of the ways a step's rays can be cast; variant 1 has no as-shipped fp16 arithmetic
ROUTES = (("env-order kernel", 1, {}),
          ("binned", 2, {}),
          ("culled", 3, {}),
          ("staged, sorted, rocks on the culled kernel", 4, {"lane_env_order": 0, "lane_rocks": 0}),
          ("staged, sorted, rocks staged", 4, {"lane_env_order": 0, "lane_rocks": 1}),
          ("staged, env order", 4, {"lane_env_order": 1}))

# The oracle's measured throughput (8 host cores, K = 200: 0.83 M rays/s in f32, 0.19 M rays/s in its fp16 mode) as (ray, triangle)
# pairs per second, and the bound on envs x (26 + P) x K that keeps one oracle pass of a case near half a second on those cores
# (a case takes two: one per step)
ORACLE_PAIRS_PER_S = {0: 0.83e6 * 200, 2: 0.19e6 * 200}
ORACLE_PAIR_BOUND = {prec: int(0.5 * v) for prec, v in ORACLE_PAIRS_PER_S.items()}      # 83 M pairs (f32), 19 M pairs (as shipped)

ENVS = (1, 7, 63, 64, 65, 100, 128, 500, 1000, 1024, 2000, 4096, 5000, 8192, 20000, 33000)
POINTS = (1, 2, 5, 6, 7, 13, 37, 38, 39, 70, 102, 120, 230, 300)
CELLS = (24, 40, 64, 96)
# against the oracle a case's terrain hit rate has to lie in (0.3, 1]: a 2.4 m map is smaller than the rays' reach (2.5 m ahead of a rover in
# its middle), most of its rays leave it (hit rates 0.28 ... 0.49 in the oracle) — the bounded draw takes the other sizes
CELLS_BOUNDED = CELLS[1:]
KS = (8, 24, 64, 200)          # K8 <= 256: beyond it every variant runs as the env-order kernel by design (its own test)


def draw_case(rng, oracle_bound=True):
    """One case from ``rng`` (a numpy Generator): batch size — multiples of 64 and not —, number of heightmap points (any padding of
    the ray slots: the fused-histogram shapes R8 = 32 / 64 and the others) and their positions, the sparse / dense split, map size, K
    and precision (0: f32, 2: as shipped).  ``oracle_bound``: the batch is cut so that envs x (26 + P) x K <= ORACLE_PAIR_BOUND of the
    precision — the oracle then needs about half a second per step at the throughput ORACLE_PAIRS_PER_S assumes (it has twice the
    cores on the GPU machines)."""
    n = int(rng.choice(ENVS))
    p = int(rng.choice(POINTS))
    cells = int(rng.choice(CELLS_BOUNDED if oracle_bound else CELLS))
    k = int(rng.choice(KS))
    prec = int(rng.choice([0, 0, 2]))
    pts = np.stack([rng.uniform(0.1, 2.5, p).round(4), rng.uniform(-1.5, 1.5, p).round(4), np.full(p, -0.26878)], axis=1)
    ns = int(rng.integers(0, p + 1))
    if oracle_bound:
        n = max(1, min(n, ORACLE_PAIR_BOUND[prec] // ((26 + p) * k)))
    return dict(envs=n, points=p, cells=cells, k=k, precision=prec,
                distribution=(pts, np.arange(ns, dtype=np.int64), np.arange(ns, p, dtype=np.int64)))


def describe(case):
    return (f"envs {case['envs']}, {case['points']} + 26 rays (R8 = {(26 + case['points'] + 7) // 8 * 8}), {case['cells']} x {case['cells']} cells, "
            f"K = {case['k']}, precision {case['precision']}")


ADVERSARIAL_SHARE = 4          # the last n // 4 envs of a batch


def add_adversarial_poses(st, seed):
    """Overwrites the last n // ADVERSARIAL_SHARE envs of ``st`` (synth.make_states) with, in four equal parts: arbitrary unit
    quaternions; axis-aligned poses on the vertex lattice (rays in facet planes, through vertices); poses far outside the map; NaN
    positions.  -> the number of envs left as make_states placed them (the first ones)."""
    n = st["pos"].shape[0]
    n_adv = n // ADVERSARIAL_SHARE
    plain = n - n_adv
    g = torch.Generator().manual_seed(7000 + seed)
    part = [plain + (n_adv * i) // 4 for i in range(5)]
    a, b = part[0], part[1]
    if b > a:
        q = torch.randn(b - a, 4, generator=g)
        st["quat"][a:b] = q / q.norm(dim=1, keepdim=True)
    a, b = part[1], part[2]
    if b > a:
        axis = torch.tensor([[1.0, 0, 0, 0], [0.70710678, 0.70710678, 0, 0], [0.70710678, 0, 0.70710678, 0], [0, 1.0, 0, 0]])
        st["quat"][a:b] = axis[torch.randint(0, 4, (b - a,), generator=g)]
        st["pos"][a:b, 0:2] = torch.round(st["pos"][a:b, 0:2] * 20) / 20
    a, b = part[2], part[3]
    st["pos"][a:b] *= 1.0e4
    a, b = part[3], part[4]
    st["pos"][a:b] = float("nan")
    return plain
