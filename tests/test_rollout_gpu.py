"""rover_gae / Engine.gae / RolloutMemory / compute_gae on the GPU against the float64 reference and its derived bound (tests/gae_ref.py):
every (T, E) of the list in all three normalize modes, contiguous / padded / [T, E, 1] layouts and five done patterns, inside trap-filled
buffers; the moments, the sharding identity, determinism, aliasing, graph replay, argument errors and one end-to-end rollout; env counts
past the scan's grid cap (its tile loop's second and third trip), non-finite columns, a one-element and an all-zero rollout."""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import gae_ref as G
from conftest import ROOT

pytestmark = pytest.mark.gpu

NAN = float("nan")
LAYOUTS = (("plain", 0), ("plain", 5), ("skrl", 0))          # (layout, pad): contiguous, padded time stride, skrl's [T, E, 1]


@pytest.fixture(scope="module")
def eng():
    from isaac_rover_amd import _lib
    e = _lib.Engine(64, device=0)
    yield e
    e.close()


class Case:
    """One rollout on the device: NaN-trapped inputs, CANARY-trapped outputs, the float64 reference."""

    def __init__(self, T, E, pattern="random", layout="plain", pad=0, seed=0, scale=1.0, data=None):
        dev = "cuda:0"
        self.T, self.E = T, E
        self.np_in = r, v, d, lv = G.make_case(T, E, pattern, scale=scale, seed=seed) if data is None else data
        mk = lambda data, dtype=torch.float32, fill=NAN: G.Guarded(T, E, dev, dtype, pad, layout, fill, data)
        self.rew, self.val, self.don = mk(r), mk(v), mk(d, torch.bool)
        lvb = torch.full((E + 64,), NAN, device=dev)
        lvb[:E] = torch.from_numpy(lv).to(dev)
        self.lv = lvb[:E]
        self.ret, self.adv = mk(None, fill=G.CANARY), mk(None, fill=G.CANARY)
        self.ref = G.reference(r, v, d, lv) if data is None else G.reference_nonfinite(r, v, d, lv)

    def run(self, eng, **kw):
        eng.gae(self.rew.t, self.val.t, self.don.t, self.lv, self.ret.t, self.adv.t, **kw)
        torch.cuda.synchronize()
        assert all(g.intact() for g in (self.rew, self.val, self.don, self.ret, self.adv)), "a guard row or pad column was written"
        return self.ret.t.reshape(self.T, self.E).clone(), self.adv.t.reshape(self.T, self.E).clone()


def _stats(dev="cuda:0"):
    return torch.full((3,), NAN, dtype=torch.float64, device=dev)


def _check_stats(stats, raw_dev, T, E, label):
    """stats_out against the float64 moments of the device's own raw A, within the stated f64 term."""
    got, want = stats.cpu().numpy(), G.moments(raw_dev.cpu().numpy())
    d_mean, d_m2 = G.moments_bound(raw_dev.cpu().numpy(), T, E)
    print(f"{label}: stats |d mean| / bound = {abs(got[1] - want[1]) / max(d_mean, G.TINY):.3f}, |d M2| / bound = {abs(got[2] - want[2]) / max(d_m2, G.TINY):.3f}")
    assert got[0] == T * E and abs(got[1] - want[1]) <= d_mean and abs(got[2] - want[2]) <= d_m2, (label, got, want, d_mean, d_m2)


def _all_modes(eng, c, label):
    """RAW + stats_out, NORMALIZE + stats_out, NORMALIZE_GIVEN with the moments of the first: each against the reference."""
    ref = c.ref
    s_raw = _stats()
    ret, raw = c.run(eng, normalize=False, stats_out=s_raw)
    G.check(ret, ref["returns"], ref["b_returns"], f"{label} RAW returns")
    G.check(raw, ref["A"], ref["bA"], f"{label} RAW A")
    _check_stats(s_raw, raw, c.T, c.E, f"{label} RAW")
    if c.T * c.E < 2:
        return
    out, b_norm = G.normalized(ref["A"], ref["bA"])
    s_own = _stats()
    ret_n, adv_n = c.run(eng, normalize=True, stats_out=s_own)
    assert torch.equal(ret_n, ret) and torch.equal(s_own, s_raw), f"{label}: returns / moments differ between RAW and NORMALIZE"
    G.check(adv_n, out, b_norm, f"{label} NORMALIZE advantages")
    ret_g, adv_g = c.run(eng, normalize=True, stats_in=s_raw)
    assert torch.equal(ret_g, ret)
    G.check(adv_g, out, b_norm, f"{label} NORMALIZE_GIVEN advantages")


SHAPES = [(T, E) for T in (1, 2, 59, 60, 61, 257) for E in (1, 63, 64, 65, 512, 4096, 65536) if E < 65536 or T <= 60]


@pytest.mark.parametrize("T,E", SHAPES)
def test_kernel_against_reference(eng, T, E):
    """Every layout x done pattern up to 4 096 envs (at 65 536: each layout and each pattern once), all three modes each."""
    combos = [(lay, pat) for lay in LAYOUTS for pat in G.DONE_PATTERNS]
    if E == 65536:
        combos = [(LAYOUTS[i % 3], pat) for i, pat in enumerate(G.DONE_PATTERNS)]
    for i, ((layout, pad), pattern) in enumerate(combos):
        c = Case(T, E, pattern, layout, pad, seed=1000 * T + E + i)
        _all_modes(eng, c, f"T={T} E={E} {layout}+{pad} {pattern}")


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_kernel_against_reference_scaled(eng, scale):
    _all_modes(eng, Case(60, 512, "random", seed=5, scale=scale), f"scale {scale}")


# GAE_BLOCK (csrc/rover_rollout.hip) and GAE_MAX_BLOCKS (csrc/rover_internal.h) as they stand in the source: the env counts below are
# placed round their product.  A change of either constant must move the sizes with it.
GAE_BLOCK, GAE_MAX_BLOCKS = 64, 2048
GAE_CAP_ENVS = GAE_BLOCK * GAE_MAX_BLOCKS                             # 131 072 envs: the most one trip of the scan's tile loop covers


@pytest.mark.parametrize("T", [1, 4, 5])                               # head only, one whole chunk only, head + chunk
@pytest.mark.parametrize("E", [GAE_CAP_ENVS, GAE_CAP_ENVS + 1, 2 * GAE_CAP_ENVS + 65])
def test_kernel_past_the_grid_cap(eng, T, E):
    """The scan's tile loop at its cap, one env past it (block 0 takes a second tile of one lane), and three trips with a ragged tail."""
    tiles = -(-E // GAE_BLOCK)
    blocks = min(tiles, GAE_MAX_BLOCKS)
    print(f"gae T={T} E={E}: {tiles} tiles on {blocks} blocks = {blocks} partials, {-(-tiles // blocks)} trip(s) of the tile loop, "
          f"{-(-blocks // 256)} trip(s) of the finishing kernel's partial loop")
    for layout, pad in LAYOUTS[:2]:
        _all_modes(eng, Case(T, E, "random", layout, pad, seed=7 * T + E + pad), f"T={T} E={E} {layout}+{pad} random")


def _ibits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("E", [130, GAE_CAP_ENVS + 1])
def test_nonfinite_columns_stay_in_their_columns(eng, E):
    """A +Inf reward under a done flag in one column and a NaN value in another: every other column's returns and raw A are the bits of
    a run on cleaned copies (the sharding identity rests on that); the two columns are +Inf / NaN exactly where the float64 recurrence
    says (0 * Inf = NaN at the next done); the moments are NaN with the full count."""
    T = 5
    data = G.nonfinite_case(T, E, seed=E)
    cols = data[4]
    bad, clean = Case(T, E, pad=3, data=data[:4]), Case(T, E, pad=3, data=G.cleaned(*data)[:4])
    s_bad, s_clean = _stats(), _stats()
    ret_b, raw_b = bad.run(eng, normalize=False, stats_out=s_bad)
    ret_c, raw_c = clean.run(eng, normalize=False, stats_out=s_clean)
    G.check(ret_c, clean.ref["returns"], clean.ref["b_returns"], f"E={E} cleaned returns")
    G.check(raw_c, clean.ref["A"], clean.ref["bA"], f"E={E} cleaned A")
    other = torch.ones(E, dtype=torch.bool, device="cuda:0")
    other[[cols["inf"], cols["nan"]]] = False
    assert torch.equal(_ibits(ret_b[:, other]), _ibits(ret_c[:, other])), "a non-finite column changed another column's returns"
    assert torch.equal(_ibits(raw_b[:, other]), _ibits(raw_c[:, other])), "a non-finite column changed another column's raw A"
    for name, got, want in (("returns", ret_b, bad.ref["returns"]), ("A", raw_b, bad.ref["A"])):
        pg, pw = G.nonfinite_pattern(got), G.nonfinite_pattern(want)
        print(f"E={E} {name}: column {cols['inf']} (+Inf reward, done) {pg[:, cols['inf']].tolist()}, column {cols['nan']} (NaN value) "
              f"{pg[:, cols['nan']].tolist()} (0 finite, 1 +Inf, 2 -Inf, 3 NaN; t = 0 .. {T - 1}); {int((pg != 0).sum())} non-finite of {pg.size}")
        assert np.array_equal(pg, pw), f"{name}: non-finite elements are not where the float64 recurrence has them"
    assert G.nonfinite_pattern(raw_b)[:, cols["inf"]].tolist() == [3, 3, 1, 1, 0] and G.nonfinite_pattern(raw_b)[:, cols["nan"]].tolist() == [3, 3, 3, 0, 0]
    sb, sc = s_bad.cpu().numpy(), s_clean.cpu().numpy()
    print(f"E={E}: stats_out {sb.tolist()}, cleaned {sc.tolist()}")
    assert sb[0] == T * E and np.isnan(sb[1]) and np.isnan(sb[2]) and np.isfinite(sc).all() and sc[0] == T * E


def test_one_element_rollout(eng):
    """T = E = 1: returns and the raw A are right, the moments are (1, A, 0).  The unbiased std of one element is 0 / 0: NORMALIZE refuses
    it (include/rover_step.h), and NORMALIZE_GIVEN with those moments — the one way to ask for it — gives NaN, as torch.std does."""
    from isaac_rover_amd._lib import RoverError
    c = Case(1, 1, "none", seed=2)
    s = _stats()
    ret, raw = c.run(eng, normalize=False, stats_out=s)
    G.check(ret, c.ref["returns"], c.ref["b_returns"], "T=E=1 returns")
    G.check(raw, c.ref["A"], c.ref["bA"], "T=E=1 A")
    assert s.tolist() == [1.0, float(raw), 0.0]
    with pytest.raises(RoverError, match=r"rover_gae failed \(-1\)"):
        c.run(eng, normalize=True)
    ret_g, adv_g = c.run(eng, normalize=True, stats_in=s)
    print(f"T=E=1: returns {float(ret_g)}, A {float(raw)}, advantage normalised with (1, A, 0): {float(adv_g)}")
    assert torch.equal(ret_g, ret) and bool(torch.isfinite(ret_g).all()) and bool(torch.isnan(adv_g).all())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                             # torch warns about the degrees of freedom, and returns NaN too
        assert bool(torch.isnan(torch.std(raw.reshape(-1).cpu())))


def test_all_zero_rollout_normalizes_to_zero(eng):
    """rewards = values = last_values = 0: the raw A is identically 0, std = 0, and (0 - 0) / (0 + 1e-8) is exactly 0, not NaN."""
    T, E = 5, 130
    _, _, d, _ = G.make_case(T, E, "random", seed=1, rate=0.2)
    z = np.zeros((T, E), dtype=np.float32)
    c = Case(T, E, pad=3, data=(z, z.copy(), d, np.zeros(E, dtype=np.float32)))
    s = _stats()
    ret, adv = c.run(eng, normalize=True, stats_out=s)
    assert s.tolist() == [float(T * E), 0.0, 0.0]
    assert bool((ret == 0).all()) and bool((adv == 0).all())
    ret_g, adv_g = c.run(eng, normalize=True, stats_in=s)
    assert bool((ret_g == 0).all()) and bool((adv_g == 0).all())
    print(f"all-zero rollout T={T} E={E}: {int((adv == 0).sum())} of {adv.numel()} advantages are 0 (NORMALIZE), {int((adv_g == 0).sum())} (NORMALIZE_GIVEN)")


@pytest.mark.parametrize("T,E", [(60, 512), (60, 130), (7, 65536)])
def test_sharding_identity(eng, T, E):
    """Two half-shards: returns and raw A bit-identical to the whole's; RAW + stats_out on each half, the moments combined (on the device
    and on the host) and fed back with NORMALIZE_GIVEN match the whole's NORMALIZE within the bound."""
    from isaac_rover_amd._lib import combine_moments
    c = Case(T, E, "random", "plain", 3, seed=E)
    s_whole = _stats()
    ret_w, raw_w = c.run(eng, normalize=False)
    _, adv_w = c.run(eng, normalize=True, stats_out=s_whole)
    h = E // 2 + 1                                                  # an odd cut: the halves' lanes do not line up with the whole's
    halves, stats = [], []
    for lo, hi in ((0, h), (h, E)):
        sl = lambda g: g.t[:, lo:hi]
        s = _stats()
        ret, adv = G.Guarded(T, hi - lo, "cuda:0", pad=2), G.Guarded(T, hi - lo, "cuda:0", pad=2)
        eng.gae(sl(c.rew), sl(c.val), sl(c.don), c.lv[lo:hi], ret.t, adv.t, normalize=False, stats_out=s)
        torch.cuda.synchronize()
        assert ret.intact() and adv.intact()
        assert torch.equal(ret.t, ret_w[:, lo:hi]) and torch.equal(adv.t, raw_w[:, lo:hi]), "a half-shard differs from the whole"
        halves.append((lo, hi, sl, ret, adv))
        stats.append(s)
    both = combine_moments(stats[0], stats[1])
    host = combine_moments(stats[0].cpu().numpy(), stats[1].cpu().numpy())
    np.testing.assert_array_equal(both.cpu().numpy(), host)         # the same IEEE operations in the same order: the same bits
    empty = torch.tensor([0.0, 5.0, 7.0], dtype=torch.float64, device="cuda:0")          # count 0, other words not zero
    assert torch.equal(combine_moments(empty, stats[0]), stats[0]) and torch.equal(combine_moments(stats[0], empty), stats[0])
    d_mean, d_m2 = G.moments_bound(raw_w.cpu().numpy(), T, E)
    sw = s_whole.cpu().numpy()
    assert host[0] == sw[0] and abs(host[1] - sw[1]) <= 2 * d_mean and abs(host[2] - sw[2]) <= 2 * d_m2
    out, b_norm = G.normalized(c.ref["A"], c.ref["bA"])
    for lo, hi, sl, ret, adv in halves:
        eng.gae(sl(c.rew), sl(c.val), sl(c.don), c.lv[lo:hi], ret.t, adv.t, normalize=True, stats_in=both)
        torch.cuda.synchronize()
        G.check(adv.t, out[:, lo:hi], b_norm[:, lo:hi], f"T={T} E={E} shard [{lo}, {hi}) NORMALIZE_GIVEN")
        G.check(adv_w[:, lo:hi], out[:, lo:hi], b_norm[:, lo:hi], f"T={T} E={E} whole NORMALIZE [{lo}, {hi})")
        # and against each other: both are within b_norm of the same float64 value
        G.check(adv.t, adv_w[:, lo:hi].double().cpu().numpy(), 2 * b_norm[:, lo:hi], f"T={T} E={E} shard [{lo}, {hi}) against the whole")


@pytest.mark.parametrize("T,E", [(60, 512), (60, 65536), (257, 65)])
def test_deterministic(eng, T, E):
    c = Case(T, E, "random", seed=9)
    s1, s2 = _stats(), _stats()
    a = c.run(eng, normalize=True, stats_out=s1)
    b = c.run(eng, normalize=True, stats_out=s2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(s1, s2)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("T,E", [(60, 512), (61, 65)])
def test_returns_may_alias_values(eng, T, E, normalize):
    c = Case(T, E, "random", "plain", 3, seed=4)
    ret, adv = c.run(eng, normalize=normalize)
    eng.gae(c.rew.t, c.val.t, c.don.t, c.lv, c.val.t, c.adv.t, normalize=normalize)          # returns = values, in place
    torch.cuda.synchronize()
    assert c.val.intact() and c.adv.intact()
    assert torch.equal(c.val.t, ret) and torch.equal(c.adv.t, adv)


def _filled_memory(eng, T, E, seed):
    from isaac_rover_amd.learning.rollout import RolloutMemory
    mem = RolloutMemory(T, E, device="cuda:0")
    for name, dtype in (("rewards", torch.float32), ("values", torch.float32), ("terminated", torch.bool)):
        mem.create_tensor(name, 1, dtype)
    r, v, d, lv = G.make_case(T, E, "random", seed=seed)
    for t in range(T):
        mem.add_samples(rewards=torch.from_numpy(r[t]).cuda(), values=torch.from_numpy(v[t]).cuda(), terminated=torch.from_numpy(d[t]).cuda())
    assert mem.filled
    return mem, torch.from_numpy(lv).cuda(), (r, v, d, lv)


def test_compute_gae_graph_replay_equals_eager(eng):
    """compute_gae captured after one warm-up and replayed on NEW contents of the same buffers equals an eager call bit for bit."""
    from isaac_rover_amd.learning.rollout import compute_gae
    T, E = 60, 512
    mem, lv, _ = _filled_memory(eng, T, E, seed=1)
    compute_gae(eng, mem, lv)                                        # warm-up: creates returns / advantages
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        compute_gae(eng, mem, lv)
    r, v, d, lv2 = G.make_case(T, E, "random", seed=2)
    mem.set_tensor_by_name("rewards", torch.from_numpy(r).cuda().unsqueeze(-1))
    mem.set_tensor_by_name("values", torch.from_numpy(v).cuda().unsqueeze(-1))
    mem.set_tensor_by_name("terminated", torch.from_numpy(d).cuda().unsqueeze(-1))
    lv.copy_(torch.from_numpy(lv2).cuda())
    for name in ("returns", "advantages"):
        mem.get_tensor_by_name(name).fill_(G.CANARY)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    replayed = [mem.get_tensor_by_name(n).clone() for n in ("returns", "advantages")]
    ret, adv = compute_gae(eng, mem, lv)
    torch.cuda.synchronize()
    assert torch.equal(replayed[0], ret) and torch.equal(replayed[1], adv)
    ref = G.reference(r, v, d, lv2)
    G.check(ret, ref["returns"], ref["b_returns"], "graph returns")
    G.check(adv, *G.normalized(ref["A"], ref["bA"]), "graph advantages")


def test_compute_gae_wants_a_filled_memory(eng):
    from isaac_rover_amd.learning.rollout import compute_gae
    mem, lv, _ = _filled_memory(eng, 4, 8, seed=3)
    mem.add_samples(rewards=torch.zeros(8, device="cuda:0"), values=torch.zeros(8, device="cuda:0"), terminated=torch.zeros(8, dtype=torch.bool, device="cuda:0"))
    with pytest.raises(ValueError):
        compute_gae(eng, mem, lv)                                    # wrapped: row 1 is next
    mem.reset()
    with pytest.raises(ValueError):
        compute_gae(eng, mem, lv)                                    # forgotten
    assert "returns" not in mem.tensors


def test_argument_errors(eng):
    """Every refused case returns ROVER_E_INVALID before any launch (canaried outputs untouched) and leaves a text; E = 0 is ROVER_OK."""
    from isaac_rover_amd import _lib
    T, E = 4, 8
    c = Case(T, E, "none", "plain", 2)
    st = E + 2

    def desc(**kw):
        f = dict(T=T, E=E, gamma=0.99, lam=0.95, rewards=c.rew.t.data_ptr(), rewards_stride=st, values=c.val.t.data_ptr(), values_stride=st,
                 dones=c.don.t.data_ptr(), dones_stride=st, last_values=c.lv.data_ptr(), returns=c.ret.t.data_ptr(), returns_stride=st,
                 advantages=c.adv.t.data_ptr(), advantages_stride=st, normalize=_lib.GAE_RAW, stats_out=None, stats_in=None)
        f.update(kw)
        return _lib.GaeDesc(**f)

    stream = _lib._stream(0)
    bad = [dict(**{k: None}) for k in ("rewards", "values", "dones", "last_values", "returns", "advantages")]
    bad += [dict(**{k + "_stride": E - 1}) for k in ("rewards", "values", "dones", "returns", "advantages")]
    bad += [dict(T=0), dict(T=4097), dict(E=-1), dict(T=4096, E=1 << 19), dict(normalize=3), dict(normalize=-1),
            dict(normalize=_lib.GAE_NORMALIZE_GIVEN), dict(T=1, E=1, normalize=_lib.GAE_NORMALIZE),
            dict(advantages=c.ret.t.data_ptr()), dict(returns=c.val.t.data_ptr() + 4), dict(advantages=c.rew.t.data_ptr()),
            dict(rewards_stride=(1 << 40) + 1), dict(stats_out=c.rew.t.data_ptr()), dict(stats_out=c.adv.t.data_ptr())]
    for kw in bad:
        rc = eng.lib.rover_gae(eng._h, C.byref(desc(**kw)), stream)
        assert rc == -1, (kw, rc)
        assert eng.lib.rover_last_error(eng._h).decode().startswith("gae:"), kw
    assert eng.lib.rover_gae(eng._h, None, stream) == -1
    torch.cuda.synchronize()
    assert c.ret.untouched() and c.adv.untouched() and c.ret.intact() and c.adv.intact()
    for mode in (_lib.GAE_RAW, _lib.GAE_NORMALIZE):
        assert eng.lib.rover_gae(eng._h, C.byref(desc(E=0, normalize=mode)), stream) == 0
    z = lambda dtype=torch.float32: torch.empty(T, 0, dtype=dtype, device="cuda:0")
    eng.gae(z(), z(), z(torch.bool), torch.empty(0, device="cuda:0"), z(), z())                  # E = 0 through the binding
    with pytest.raises(_lib.RoverError):
        eng.gae(c.rew.t, c.val.t, c.don.t, c.lv, c.ret.t.double(), c.adv.t)
    with pytest.raises(_lib.RoverError):
        eng.gae(c.rew.t, c.val.t[:, :4], c.don.t, c.lv, c.ret.t, c.adv.t)
    with pytest.raises(_lib.RoverError):
        eng.gae(c.rew.t.cpu(), c.val.t, c.don.t, c.lv, c.ret.t, c.adv.t)
    torch.cuda.synchronize()
    assert c.ret.untouched() and c.adv.untouched()


def test_end_to_end_rollout_into_memory():
    """RoverTask at 512 envs, actor + critic, 8 steps into a RolloutMemory: compute_gae equals the reference on the stored tensors, and
    log_prob re-evaluated with taken_actions from the memory equals the stored one bit for bit."""
    from isaac_rover_amd import synth
    from isaac_rover_amd.config import SimConfig
    from isaac_rover_amd.learning.model import DeterministicHeightmap, StochasticActorHeightmap
    from isaac_rover_amd.learning.rollout import RolloutMemory, compute_gae
    from isaac_rover_amd.tasks.rover import RoverTask
    from isaac_rover_amd.vec_env import VecEnv
    n, T = 512, 8
    scene = synth.make_scene(n_cells=128, k=16, n_stones=10)
    env = VecEnv(headless=True)
    g = torch.Generator().manual_seed(3)
    spawn = torch.zeros(n, 3)
    spawn[:, 0:2] = 4.0 + 4.8 * torch.rand(n, 2, generator=g)
    task = RoverTask("Rover", SimConfig(num_envs=n, device="cuda:0"), env, scene=scene, distribution=synth.ray_distribution("37"))
    env.set_task(task, sim_params={"dt": 0.05}, spawn_positions=spawn)
    obs = env.reset()
    actor, critic = StochasticActorHeightmap(task._engine, task), DeterministicHeightmap(task._engine, task, seed=1)
    mem = RolloutMemory(T, n, device=task.device)
    for name, size, dtype in (("states", obs.shape[1], torch.float32), ("actions", 2, torch.float32), ("log_prob", 1, torch.float32),
                              ("values", 1, torch.float32), ("rewards", 1, torch.float32), ("terminated", 1, torch.bool)):
        mem.create_tensor(name, size, dtype)
    for _ in range(T):
        actions, log_prob, _ = actor.act(obs)
        values, _, _ = critic.act(obs)
        states = obs.clone()
        obs, rew, done, info = env.step(actions)
        mem.add_samples(states=states, actions=actions, log_prob=log_prob, values=values, rewards=rew, terminated=done.bool())
    assert mem.filled and len(mem) == T * n
    last_values, _, _ = critic.act(obs)
    ret, adv = compute_gae(task._engine, mem, last_values)
    torch.cuda.synchronize()
    get = mem.get_tensor_by_name
    ref = G.reference(get("rewards"), get("values"), get("terminated"), last_values)
    G.check(ret, ref["returns"], ref["b_returns"], "end to end returns")
    G.check(adv, *G.normalized(ref["A"], ref["bA"]), "end to end advantages")
    assert ret.data_ptr() == get("returns").data_ptr() and adv.shape == (T, n, 1)
    for t in (0, T - 1):
        _, lp, _ = actor.act({"states": get("states")[t], "taken_actions": get("actions")[t]}, role="policy")
        assert torch.equal(lp, get("log_prob")[t]), f"log_prob of the stored actions differs at step {t}"
    env.close()


def test_rollout_example_with_rollouts():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "rollout.py"), "--policy", "actor", "--rollouts", "4", "--steps", "8",
                          "--envs", "512"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("rollout of 4 steps: mean return") == 2, out.stdout
