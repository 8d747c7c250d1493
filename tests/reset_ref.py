"""Float64 restatement of the reset path (rover.py:533-564, 649-661) and seeded case builders for its tests.  numpy only, no GPU.

The restatement decides in float64 what the kernels of csrc/rover_reset.hip decide in float32, so a case is only usable where the two
cannot disagree: every builder rerolls an input whose decision margin |clearance - threshold| is below MARGIN.  MARGIN is 1e-3 m, a
thousand times the ~1e-6 m that one ulp of the device's cosf / sinf moves a goal at radius 8 (and far above the f32 rounding of the
clearance itself, ~1e-6 m at 10 m): after the reroll every compared decision is exact and no case has to be skipped."""
import ctypes as C

import numpy as np

MARGIN = 1e-3
F32 = np.float32
THR_SPAWN = float(F32(1.4))         # rover.py:660, as the kernel holds it
THR_GOAL = float(F32(1.0))          # rover.py:539
STEP_X = F32(0.05)                  # rover.py:660
TWO_PI_F32 = F32(2 * 3.14159265358979323846)
YAW_KEY = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
STONE_TILE = 1024                   # tile of clearance_tiles
CELL = 2.0                          # stone-grid cell, rover_set_stones
# first-clear indices the scheduled goal cases prescribe (those below max_draws), plus max_draws - 1 and "never" (= max_draws)
T_LIST = (0, 7, 8, 9, 15, 63, 64, 65, 127, 128)
# Found on the CPU with the host Philox (tests/test_reset_path_host.py pins it): among the first 255 of YAW_IDS + 5000 this seed draws
# both 0 and 360 degrees, so floor(u * 361) cannot pass for floor(u * 360).
YAW_SEED = 9
YAW_IDS = np.arange(2304, dtype=np.int64)[::-1][3:300].copy()      # 297 local ids, descending, without env 0
YAW_IDS.setflags(write=False)


def info7_of(x, y, r):
    """[S,7] float32 stone_info rows (terrain_utils.py:416-424) from centres and radii; the reset path reads columns 0, 1 and 6."""
    x = np.atleast_1d(np.asarray(x, np.float64))
    info = np.zeros((x.shape[0], 7), F32)
    info[:, 0], info[:, 1], info[:, 6] = x, y, r
    return info


# ---------------------------------------------------------------------------------------------------------------------------------
# clearance and the decisions made on it
# ---------------------------------------------------------------------------------------------------------------------------------
def stone_distances64(info7, xy):
    """-> (hypot [n,S], d = hypot - r [n,S]) in float64."""
    info = np.asarray(info7, F32).astype(np.float64).reshape(-1, 7)
    q = np.asarray(xy, F32).astype(np.float64).reshape(-1, 2)
    h = np.hypot(q[:, 0:1] - info[None, :, 0], q[:, 1:2] - info[None, :, 1])
    return h, h - info[None, :, 6]


def clearance64(info7, xy):
    """min_s(hypot - r) in float64; +inf without stones; NaN propagates as torch.min does (rover.py:538)."""
    _, d = stone_distances64(info7, xy)
    if d.shape[1] == 0:
        return np.full(d.shape[0], np.inf)
    with np.errstate(invalid="ignore"):
        return d.min(axis=1)                    # np.min propagates NaN


def collides64(info7, xy, thr):
    """-> (clearance <= thr, margin |clearance - thr|).  A NaN clearance collides with nothing and is decided (margin inf)."""
    c = clearance64(info7, xy)
    with np.errstate(invalid="ignore"):
        m = np.abs(c - float(thr))
        hit = c <= float(thr)
    m[np.isnan(m)] = np.inf
    return hit, m


def walk_spawn(info7, pos3, max_iter):
    """avoid_pos_rock_collision per spawn: x = f32(x + 0.05f) while clearance64 <= 1.4, at most max_iter times.
    -> (x [n] float32, steps [n] int64, the smallest margin among the decisions taken [n])."""
    p = np.asarray(pos3, F32).reshape(-1, 3)
    x, y = p[:, 0].copy(), p[:, 1].copy()
    n = x.shape[0]
    steps = np.zeros(n, np.int64)
    margin = np.full(n, np.inf)
    active = np.arange(n)
    it = 0
    while it < max_iter and active.size:
        hit, m = collides64(info7, np.stack((x[active], y[active]), axis=1), THR_SPAWN)
        margin[active] = np.minimum(margin[active], m)
        active = active[hit]
        x[active] = x[active] + STEP_X          # float32 + float32: the kernel's single rounding
        steps[active] += 1
        it += 1
    return x, steps, margin


# ---------------------------------------------------------------------------------------------------------------------------------
# goals: the sequential loop of oracle_generate_goals with its decisions in float64
# ---------------------------------------------------------------------------------------------------------------------------------
def goal_xy64(u, radius, spawn_xy):
    """random_goals rover.py:554-564: alpha is the kernel's one float32 product; the rest in float64."""
    alpha = (TWO_PI_F32 * np.asarray(u, F32)).astype(np.float64)
    s = np.asarray(spawn_xy, np.float64)
    return np.stack((float(radius) * np.cos(alpha) + s[..., 0], float(radius) * np.sin(alpha) + s[..., 1]), axis=-1)


def goals64(info7, env_ids, initial_pos3, draws, radius):
    """-> dict: target [E,2] float64 (NaN = never written), used (-1 = the draws ran out), t [n] (the iteration at which entry i was
    accepted; -1 for a zero-id entry, max_draws for one that never clears), tmax, lz (the last entry whose id is 0 when iteration
    max(tmax, 0) draws; -1 = none), margin (the smallest decision margin met), env0_trips (64-draw trips env 0's replay needs)."""
    ids = np.asarray(env_ids, np.int64).copy()
    init = np.asarray(initial_pos3, F32).astype(np.float64)
    u_all = np.asarray(draws, F32).reshape(-1, ids.shape[0])
    T, n = u_all.shape
    target = np.full((init.shape[0], 2), np.nan)
    t_acc = np.where(ids == 0, -1, T).astype(np.int64)
    last_zero = np.full(T, -1, np.int64)        # per iteration: the last zero-id entry while it draws
    margin, used, done = np.inf, 0, False
    while not done:
        if used >= T:
            used = -1
            break
        u = u_all[used]
        z = np.nonzero(ids == 0)[0]
        last_zero[used] = z[-1] if z.size else -1
        g = goal_xy64(u, radius, init[ids, 0:2])
        nz = ids != 0
        target[ids[nz]] = g[nz]                 # distinct ids
        if z.size:
            target[0] = g[z[-1]]                # a sequential index_put: the last writer wins
        hit, m = collides64(info7, target[ids], THR_GOAL)
        margin = min(margin, float(m.min()))
        t_acc[nz & ~hit] = used
        ids = np.where(hit, ids, 0)
        used += 1
        done = not hit.any()
    own = t_acc[(t_acc >= 0) & (t_acc < T)]
    tmax = int(own.max()) if own.size else -1
    lz = int(last_zero[max(tmax, 0)])
    trips = 0
    if used > 0 and lz >= 0:
        trips = (used - 1 - max(tmax, 0)) // 64 + 1
    return dict(target=target, used=int(used), t=t_acc, tmax=tmax, lz=lz, margin=margin, env0_trips=trips)


# ---------------------------------------------------------------------------------------------------------------------------------
# Philox on the host (rover_philox4x32: the round function the kernels run)
# ---------------------------------------------------------------------------------------------------------------------------------
def _philox_c0(key, c0, c1):
    from isaac_rover_amd import _lib
    return _lib.philox4x32((c0, c1, 0, 0), (key & 0xffffffff, (key >> 32) & 0xffffffff))[0]


def philox_uniform(seed, t, gid):
    """The goal uniform of (seed, draw t, global env id): counter {gid, t, 0, 0}, key {seed lo, seed hi} -> (c0 >> 8) / 2^24, float32."""
    return F32((_philox_c0(int(seed) & M64, int(gid), int(t)) >> 8) / 16777216.0)


def philox_draws(seed, max_draws, gids):
    """[max_draws, n] float32: what goals_draw_kernel draws for the listed global ids."""
    from isaac_rover_amd import _lib
    lib = _lib.load()
    seed = int(seed) & M64
    key = (C.c_uint32 * 2)(seed & 0xffffffff, seed >> 32)
    ctr, out = (C.c_uint32 * 4)(), (C.c_uint32 * 4)()
    u = np.zeros((max_draws, len(gids)), F32)
    for i, g in enumerate(gids):
        for t in range(max_draws):
            ctr[0], ctr[1], ctr[2], ctr[3] = int(g) & 0xffffffff, t, 0, 0
            assert lib.rover_philox4x32(ctr, key, out) == 0
            u[t, i] = (out[0] >> 8) / 16777216.0
    return u


def philox_yaw_deg(seed, gids):
    """reset_envs_kernel's yaw: key seed ^ 0x9E3779B97F4A7C15, counter {gid, 0, 0, 0}, deg = floor(f32(u) * f32(361)) in 0 .. 360."""
    u = np.array([philox_uniform((int(seed) & M64) ^ YAW_KEY, 0, g) for g in gids], F32)
    return np.floor(u * F32(361.0)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
# the stone grid of rover_set_stones, restated in float32 (only to know which cell list a query meets)
# ---------------------------------------------------------------------------------------------------------------------------------
REACH_F32 = F32(1.4) + F32(0.05)                # the grid's reach as the library adds it up: one ulp below f32(1.45)


def grid_origin(info7, reach=F32(1.45)):
    """(x0, y0) = min - (rmax + reach) in float32 over the finite stones; (0, 0) - reach without any."""
    info = np.asarray(info7, F32).reshape(-1, 7)
    ok = ~np.isnan(info[:, [0, 1, 6]]).any(axis=1)
    if not ok.any():
        return F32(0) - (F32(0) + F32(reach)), F32(0) - (F32(0) + F32(reach))
    rmax = max(F32(0), info[ok, 6].max())
    pad = F32(rmax + F32(reach))
    return F32(info[ok, 0].min() - pad), F32(info[ok, 1].min() - pad)


def stone_grid(info7):
    """-> dict x0, y0, nx, ny, lists {(cx, cy): [stone, ...]} as rover_set_stones builds them (stone order kept; all lists empty when a
    stone holds a NaN)."""
    info = np.asarray(info7, F32).reshape(-1, 7)
    nan = np.isnan(info[:, [0, 1, 6]]).any(axis=1)
    ok = ~nan
    x0, y0 = grid_origin(info, REACH_F32)
    if ok.any():
        rmax = max(F32(0), info[ok, 6].max())
        pad = F32(rmax + REACH_F32)
        x1, y1 = F32(info[ok, 0].max() + pad), F32(info[ok, 1].max() + pad)
    else:
        x1, y1 = F32(F32(1) + REACH_F32), F32(F32(1) + REACH_F32)
    cell = F32(CELL)
    nx, ny = max(int(F32(x1 - x0) / cell) + 1, 1), max(int(F32(y1 - y0) / cell) + 1, 1)
    lists = {}
    if not nan.any():
        for s in np.nonzero(ok)[0]:
            x, y, rr = info[s, 0], info[s, 1], F32(info[s, 6] + REACH_F32)
            cx0, cx1 = int(F32(F32(x - rr) - x0) / cell), int(F32(F32(x + rr) - x0) / cell)
            cy0, cy1 = int(F32(F32(y - rr) - y0) / cell), int(F32(F32(y + rr) - y0) / cell)
            for cx in range(max(cx0, 0), min(cx1, nx - 1) + 1):
                for cy in range(max(cy0, 0), min(cy1, ny - 1) + 1):
                    lists.setdefault((cx, cy), []).append(int(s))
    return dict(x0=x0, y0=y0, nx=nx, ny=ny, lists=lists)


def cell_of(grid, x, y):
    """The cell collides_grid looks up for (x, y), or None outside the grid."""
    fx, fy = F32(F32(x) - grid["x0"]) * F32(0.5), F32(F32(y) - grid["y0"]) * F32(0.5)
    if not (fx >= 0 and fy >= 0 and fx < grid["nx"] and fy < grid["ny"]):
        return None
    return int(fx), int(fy)


# ---------------------------------------------------------------------------------------------------------------------------------
# case builders (fixed seeds; everything they return is read-only)
# ---------------------------------------------------------------------------------------------------------------------------------
def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def reroll_points(info7, draw, n, thr, rng):
    """n points from draw(rng, k) -> [k,2] float32, each with |clearance64 - thr| >= MARGIN for every thr given."""
    xy = draw(rng, n).astype(F32)
    thrs = np.atleast_1d(thr)
    for _ in range(100):
        bad = np.zeros(n, bool)
        for t in thrs:
            bad |= collides64(info7, xy, t)[1] < MARGIN
        if not bad.any():
            return xy
        xy[bad] = draw(rng, int(bad.sum())).astype(F32)
    raise AssertionError("reroll_points: no decided sample found")


def lattice_stones(S, seed=0):
    """S stones on a jittered 4 m lattice (radius 0.1 .. 0.4): the stone next to a query close to a centre is known by construction."""
    rng = np.random.default_rng(1000 + seed + S)
    side = max(int(np.ceil(np.sqrt(max(S, 1)))), 1)
    k = rng.permutation(side * side)[:S]
    x = 4.0 * (k // side) + rng.uniform(-0.5, 0.5, S)
    y = 4.0 * (k % side) + rng.uniform(-0.5, 0.5, S)
    return info7_of(x, y, rng.uniform(0.1, 0.4, S))


def dedicated_stones(S):
    """Stones whose loss shows a dropped or shifted tile: 0, 1023, 1024, S - 1 and the last stone of each tile."""
    want = {0, STONE_TILE - 1, STONE_TILE, S - 1} | {min(s0 + STONE_TILE, S) - 1 for s0 in range(0, S, STONE_TILE)}
    return sorted(s for s in want if 0 <= s < S)


def clearance_case(S, seed=0):
    """Stones, 1000 queries (random ones, then one beside each dedicated stone: those are the LAST rows, in the last partial block of
    a launch over all of them), and the float64 answer with the derived float32 bound per query."""
    info = lattice_stones(S, seed)
    rng = np.random.default_rng(2000 + seed + S)
    ded = dedicated_stones(S)
    side = 4.0 * max(int(np.ceil(np.sqrt(max(S, 1)))), 1)
    xy = rng.uniform(-3.0, side, (1000 - len(ded), 2)).astype(F32)
    if ded:
        ang = rng.uniform(0, 2 * np.pi, len(ded))
        near = info[ded, 0:2].astype(np.float64) + 0.3 * np.stack((np.cos(ang), np.sin(ang)), axis=1)
        xy = np.concatenate((xy, near.astype(F32)))
    return _freeze(dict(info=info, xy=xy, dedicated=np.asarray(ded, np.int64), **clearance_answer(info, xy)))


def clearance_answer(info7, xy):
    """-> want (float64), tol = 8 * 2^-24 * (dist + |r|) of the nearest stone: two subtractions, two squares, a sum, a sqrt and the final
    subtraction, each rounded once (the build uses -ffp-contract=off), nearest (stone index), gap (runner-up - nearest)."""
    h, d = stone_distances64(info7, xy)
    n = d.shape[0]
    if d.shape[1] == 0:
        return dict(want=np.full(n, np.inf), tol=np.zeros(n), nearest=np.full(n, -1), gap=np.full(n, np.inf))
    k = d.argmin(axis=1)
    r = np.abs(np.asarray(info7, F32).astype(np.float64)[k, 6])
    tol = 8 * 2.0 ** -24 * (h[np.arange(n), k] + r)
    gap = np.partition(d, 1, axis=1)[:, 1] - d[np.arange(n), k] if d.shape[1] > 1 else np.full(n, np.inf)
    return dict(want=d[np.arange(n), k], tol=tol, nearest=k, gap=gap)


CLUSTER_LENGTHS = (1, 3, 4, 5, 8, 9)


def grid_stone_sets():
    """name -> info7 for the grid-decision tests."""
    rng = np.random.default_rng(31)
    sets = {}
    # isolated clusters, 40 m apart: L - 1 small stones (r = 0.05) and, listed last, one of r = 0.8, all within 0.05 m of one centre
    xs, ys, rs = [], [], []
    for j, L in enumerate(CLUSTER_LENGTHS):
        c = np.array([40.0 * j + 1.0, 3.0 + 7.0 * j])
        off = rng.uniform(-0.05, 0.05, (L, 2))
        xs += list(c[0] + off[:, 0]); ys += list(c[1] + off[:, 1]); rs += [0.05] * (L - 1) + [0.8]
    sets["clusters"] = info7_of(xs, ys, rs)
    sets["big"] = info7_of([3.0], [-2.0], [5.0])
    sets["negative"] = info7_of(rng.uniform(-60, -40, 30), rng.uniform(-35, -20, 30), rng.uniform(0.1, 0.45, 30))
    sets["one_point"] = info7_of([7.25] * 12, [-1.5] * 12, rng.uniform(0.1, 0.45, 12))
    sets["empty"] = np.zeros((0, 7), F32)
    nan = info7_of(rng.uniform(0, 12.8, 12), rng.uniform(0, 12.8, 12), rng.uniform(0.1, 0.45, 12))
    nan[5, 1] = np.nan
    sets["nan"] = nan
    for v in sets.values():
        v.setflags(write=False)
    return sets


def cluster_centres(info7):
    """(centre of the large stone, L) per cluster of the "clusters" set."""
    out, s = [], 0
    for L in CLUSTER_LENGTHS:
        out.append((np.asarray(info7, F32)[s + L - 1, 0:2].astype(np.float64), L, s + L - 1))
        s += L
    return out


def grid_queries(name, info7, thr=THR_SPAWN, n_random=160, seed=0):
    """Finite query points for a stone set, all decided against every threshold in thr: random ones (rerolled), the grid's cell corners
    x0 + 2k, y0 + 2k with their float32 neighbours (for the origin as f32(min - (rmax + 1.45)) and as the library sums it), and points
    0.01 m and 10 m outside each side.  -> [n,2] float32."""
    info = np.asarray(info7, F32)
    rng = np.random.default_rng(77 + seed)
    g = stone_grid(info)
    lo = np.array([g["x0"], g["y0"]], np.float64)
    hi = lo + CELL * np.array([g["nx"], g["ny"]])
    fin = info[~np.isnan(info[:, [0, 1, 6]]).any(axis=1)]
    thrs = np.atleast_1d(thr)

    def near_stones(r, k):          # around a random stone, within 3.5 m of its rim: both outcomes occur
        if fin.shape[0] == 0:
            return r.uniform(lo - 3, hi + 3, (k, 2))
        s = r.integers(0, fin.shape[0], k)
        a = r.uniform(0, 2 * np.pi, k)
        d = np.where(r.random(k) < 0.25, fin[s, 6] * r.random(k), fin[s, 6] + r.uniform(0.0, 3.5, k))     # a quarter inside the disc
        return fin[s, 0:2] + np.stack((d * np.cos(a), d * np.sin(a)), axis=1)

    pts = [reroll_points(info, near_stones, n_random, thrs, rng)]
    if name == "clusters":
        # in each cluster's own cell list only the last listed stone is within reach of these
        for c, _, _ in cluster_centres(info):
            def ring(r, k, c=c):
                a = np.round(r.uniform(0, 2 * np.pi, k) / (np.pi / 2)) * (np.pi / 2) + np.pi / 4 + r.uniform(-0.1, 0.1, k)   # near a diagonal
                d = r.uniform(1.65, 1.95, k)
                return c + np.stack((d * np.cos(a), d * np.sin(a)), axis=1)
            pts.append(reroll_points(info, ring, 8, thrs, rng))
    # cell corners: every lattice coordinate near the stones, for both readings of the origin, with float32 neighbours
    corners = []
    for reach in (F32(1.45), REACH_F32):
        x0, y0 = grid_origin(info, reach)
        kx = np.unique(np.clip(rng.integers(0, g["nx"] + 1, 12), 0, g["nx"]))
        ky = np.unique(np.clip(rng.integers(0, g["ny"] + 1, 12), 0, g["ny"]))
        for a in kx:
            for b in ky:
                x, y = F32(x0 + F32(2.0) * F32(a)), F32(y0 + F32(2.0) * F32(b))
                for ex in (np.nextafter(x, F32(-1e30)), x, np.nextafter(x, F32(1e30))):
                    for ey in (np.nextafter(y, F32(-1e30)), y, np.nextafter(y, F32(1e30))):
                        corners.append((ex, ey))
    # corners of the cells that hold stones too (the random k above may miss them on a large grid)
    for s in fin[:: max(fin.shape[0] // 6, 1)]:
        x0, y0 = g["x0"], g["y0"]
        a, b = np.floor((s[0] - x0) / 2), np.floor((s[1] - y0) / 2)
        for da in (0, 1):
            for db in (0, 1):
                x, y = F32(x0 + F32(2.0) * F32(a + da)), F32(y0 + F32(2.0) * F32(b + db))
                corners += [(x, y), (np.nextafter(x, F32(-1e30)), y), (x, np.nextafter(y, F32(-1e30)))]
    corners = np.unique(np.asarray(corners, F32), axis=0)
    keep = np.ones(len(corners), bool)
    for t in thrs:
        keep &= collides64(info, corners, t)[1] >= MARGIN           # fixed points cannot be rerolled: the decided ones are chosen
    pts.append(corners[keep])
    # outside the grid on each side
    out = []
    for d in (0.01, 10.0):
        for t in rng.uniform(0.05, 0.95, 3):
            out += [(lo[0] - d, lo[1] + t * (hi[1] - lo[1])), (hi[0] + d, lo[1] + t * (hi[1] - lo[1])),
                    (lo[0] + t * (hi[0] - lo[0]), lo[1] - d), (lo[0] + t * (hi[0] - lo[0]), hi[1] + d)]
    out = np.asarray(out, F32)
    for t in thrs:
        assert (collides64(info, out, t)[1] >= MARGIN).all()
    pts.append(out)
    xy = np.concatenate(pts).astype(F32)
    xy.setflags(write=False)
    return xy


NONFINITE_XY = np.array([[np.nan, 1.0], [1.0, np.nan], [np.nan, np.nan], [np.inf, 1.0], [-np.inf, 1.0], [1.0, np.inf], [1.0, -np.inf],
                         [np.inf, -np.inf]], F32)
NONFINITE_XY.setflags(write=False)


def walk_case(n, n_stones, seed=0):
    """Spawns whose walk along +x passes n_stones stones in sequence (3.2 m apart: a walk close to their line leaves one stone's 1.4 m zone inside the
    next one's), rerolled until every decision of every walk has margin >= MARGIN.  Rows differ in y and start."""
    rng = np.random.default_rng(500 + 10 * seed + n_stones)
    info = info7_of(4.0 + 3.2 * np.arange(n_stones), np.full(n_stones, 5.0), np.full(n_stones, 0.4))

    def draw(r, k):
        return np.stack((r.uniform(1.5, 4.0, k), r.uniform(3.6, 6.4, k), r.uniform(-1, 1, k)), axis=1).astype(F32)

    pos = draw(rng, n)
    for _ in range(200):
        bad = walk_spawn(info, pos, 100000)[2] < MARGIN
        if not bad.any():
            break
        pos[bad] = draw(rng, int(bad.sum()))
    else:
        raise AssertionError("walk_case: no decided walks found")
    x, steps, margin = walk_spawn(info, pos, 100000)
    return _freeze(dict(info=info, pos=pos, x=x, steps=steps, margin=margin))


def random_goal_case(n, env0, E=2304, T=64, radius=3.0, n_stones=25, seed=0):
    """Random stones on the 12.8 m scene, n listed ids with env 0 "first", "last" or "absent", uniforms rerolled until the goal of every
    (t, i) is decided both from entry i's own spawn and from env 0's (any column can become env 0's writer)."""
    rng = np.random.default_rng(9000 + 17 * n + seed + {"first": 1, "last": 2, "absent": 3}[env0])
    info = info7_of(rng.uniform(0, 12.8, n_stones), rng.uniform(0, 12.8, n_stones), rng.uniform(0.05, 0.45, n_stones))
    initial = np.zeros((E, 3), F32)
    initial[:, 0:2] = rng.uniform(1.0, 11.8, (E, 2))
    if env0 == "absent":
        ids = rng.permutation(np.arange(1, E))[:n]
    else:
        rest = rng.permutation(np.arange(1, E))[: n - 1]
        ids = np.concatenate(([0], rest)) if env0 == "first" else np.concatenate((rest, [0]))
    ids = ids.astype(np.int64)
    assert ids.shape[0] == n
    u = rng.random((T, n)).astype(F32)
    for _ in range(100):
        own = collides64(info, goal_xy64(u, radius, initial[ids, 0:2][None]).reshape(-1, 2), THR_GOAL)[1]
        at0 = collides64(info, goal_xy64(u, radius, initial[0, 0:2]).reshape(-1, 2), THR_GOAL)[1]
        bad = (np.minimum(own, at0) < MARGIN).reshape(T, n)
        if not bad.any():
            break
        u[bad] = rng.random(int(bad.sum())).astype(F32)
    else:
        raise AssertionError("random_goal_case: no decided uniforms found")
    return _freeze(dict(info=info, ids=ids, initial=initial, draws=u, radius=radius))


SCHED_SPAWN = (6.4, 6.4)
SCHED_RADIUS = 8.0


def scheduled_goal_case(T, t_own, env0, extra, E=2304, seed=0):
    """All spawns at one point, one stone (r = 0.5) at spawn + (radius, 0): a uniform within 0.02 of 0 (mod 1) collides, one in
    [0.08, 0.92] is clear.  ``t_own``: the prescribed first-clear index of each listed non-zero id (T = never); ``env0``: "first",
    "last" or "absent"; ``extra``: how many iterations after max(tmax, 0) env 0's own goal first clears (None: never).  The columns that
    do not decide an iteration hold the OPPOSITE of env 0's plan, so that reading a wrong column shows.  -> the case and its plan."""
    rng = np.random.default_rng(4000 + 131 * T + seed)
    t_own = [int(t) for t in t_own]
    k = len(t_own)
    rest = rng.permutation(np.arange(1, E))[:k].astype(np.int64)
    ids = rest if env0 == "absent" else np.concatenate(([0], rest)) if env0 == "first" else np.concatenate((rest, [0]))
    ids = ids.astype(np.int64)
    n = ids.shape[0]
    t = np.full(n, -1, np.int64)
    t[ids != 0] = t_own
    own = t[(t >= 0) & (t < T)]
    tmax = int(own.max()) if own.size else -1
    t0 = max(tmax, 0)
    zero_before = np.nonzero((t < 0) | (t < tmax))[0]
    lz = int(zero_before[-1]) if zero_before.size else -1
    never = bool((t >= T).any())
    clear_at = None if extra is None else t0 + int(extra)
    if never:
        used = -1
    elif lz < 0:
        used = t0 + 1
    elif clear_at is None or clear_at >= T:
        used = -1
    else:
        used = clear_at + 1

    def collide(shape):
        v = rng.uniform(0.0, 0.02, shape)
        return np.where(rng.random(shape) < 0.5, v, 1.0 - 0.02 + v * 0.999).astype(F32)

    def clear(shape):
        return rng.uniform(0.08, 0.92, shape).astype(F32)

    plan_clear = np.array([clear_at is not None and it >= clear_at for it in range(T)])
    u = np.where(plan_clear[:, None], collide((T, n)), clear((T, n)))            # decoys: the opposite of env 0's plan
    for i in range(n):
        if t[i] < 0:
            continue
        u[: min(t[i], T), i] = collide(min(t[i], T))
        if t[i] < T:
            u[t[i], i] = clear(())
    if lz >= 0:
        # env 0's plan is written even when an entry never clears: then that entry alone makes the draws run out
        assert t[lz] < T and t[n - 1] < T
        u[t0, lz] = clear(()) if plan_clear[t0] else collide(())
        for it in range(t0 + 1, T):
            u[it, n - 1] = clear(()) if plan_clear[it] else collide(())
    initial = np.zeros((E, 3), F32)
    initial[:, 0], initial[:, 1] = SCHED_SPAWN
    info = info7_of([SCHED_SPAWN[0] + SCHED_RADIUS], [SCHED_SPAWN[1]], [0.5])
    trips = (used - 1 - t0) // 64 + 1 if (used > 0 and lz >= 0) else 0
    plan = dict(t=t, tmax=tmax, lz=lz, used=used, env0_trips=trips)
    return _freeze(dict(info=info, ids=ids, initial=initial, draws=u, radius=SCHED_RADIUS, plan=plan))


def scheduled_cases(T):
    """name -> scheduled_goal_case for max_draws = T: prescribed first-clear indices from T_LIST (those that fit), T - 1 and never."""
    fit = [t for t in T_LIST if t < T]
    cases = {}
    # every index that fits, and T - 1; env 0 listed first, clears with the slowest entry's iteration
    cases["all_t"] = scheduled_goal_case(T, fit + [T - 1] + fit[::-1], "first", 0, seed=1)
    # env 0 absent: its writer at iteration tmax is the last entry accepted earlier, afterwards entry n - 1
    lo = sorted(set([t for t in fit if t <= T - 4] + ([0, (T - 1) // 2] if T >= 3 else [0])))
    cases["absent_later"] = scheduled_goal_case(T, lo + [lo[0]] + lo[::-1] + [lo[-1]], "absent", min(2, T - 1 - max(lo)), seed=2)
    # no zero-id entry yet at tmax (all entries accept in the same iteration): env 0 is not written
    cases["no_writer"] = scheduled_goal_case(T, [fit[len(fit) // 2]] * 5, "absent", 0, seed=3)
    # only the zero id: tmax = -1
    cases["only_zero"] = scheduled_goal_case(T, [], "first", min(3, T - 1), seed=4)
    # an entry that never clears
    cases["never"] = scheduled_goal_case(T, fit[:3] + [T] + fit[:2], "last", 0, seed=5)
    # env 0 runs out of draws in its own replay
    cases["env0_exhausts"] = scheduled_goal_case(T, lo[:4], "last", None, seed=6)
    if T >= 65:
        # env 0 clears only in the second 64-draw trip of its replay
        early = [t for t in fit if t + 65 < T] or [0]
        extra = min(64 + 1, T - 1 - max(early))
        cases["second_trip"] = scheduled_goal_case(T, early + early[::-1], "first", extra, seed=7)
        # the same with entry n - 1 no zero-id entry from the start (env 0 absent where two prescribed indices fit, else listed last)
        cases["second_trip_absent"] = scheduled_goal_case(T, early + [early[0]], "absent" if len(early) > 1 else "last",
                                                          min(64, T - 1 - max(early)), seed=8)
    return cases
