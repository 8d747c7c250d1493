"""GPU: rover_obs_noise (csrc/rover_noise.hip) against the float64 restatement (tests/obs_noise_ref.py) under its derived bound — the
dropout mask and the copied columns exactly —, the 8-byte and the scalar path on the same data, in place and strided, invariance to
sharding, call counter form and repetition, the offset draw's episodes, the all-off case, HeightmapNoise eagerly and captured in a
graph, the student acting on a noisy observation, and the two examples' new flags."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import obs_noise_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON = dict(sigma_point=0.05, sigma_offset=0.02, dropout=0.1, drop_value=-1.0)
P37 = {"proprioceptive": 4, "sparse": 37, "dense": 0, "actions": 2}           # the widths of the p37 fixtures: obs [E, 41]


@pytest.fixture(scope="module")
def eng():
    from isaac_rover_amd import _lib
    e = _lib.Engine(64, device=0)
    yield e
    e.close()


def rows_of(m, f, stride=None, seed=0, offset=0):
    """A seeded [m, f] float32 matrix on the GPU as a view of rows ``stride`` apart, starting ``offset`` floats into its buffer."""
    stride = f if stride is None else stride
    g = torch.Generator().manual_seed(seed)
    data = 3.0 * torch.randn(m, f, generator=g)
    buf = torch.full((m * stride + offset,), 99.0, device=DEV)
    view = buf[offset:].view(m, stride)[:, :f]
    view.copy_(data.to(DEV))
    return view


def check(got, x, first, label, **kw):
    """got against the restatement: untouched columns and dropped elements exactly, the rest inside the bound -> worst error / bound."""
    want, bound, dropped = R.reference(x.cpu().numpy(), first, **kw)
    g = got.cpu().numpy()
    assert np.array_equal(g[:, :first].view(np.uint32), x.cpu().numpy()[:, :first].view(np.uint32)), f"{label}: a copied column changed"
    assert np.array_equal(g[dropped], want[dropped].astype(np.float32)), f"{label}: a dropped element is not drop_value"
    live = ~dropped
    live[:, :first] = False
    if "dropout" in kw and kw["dropout"] > 0 and live.any():                    # the mask itself: nothing else reads drop_value
        assert not np.any(g[live] == np.float32(kw.get("drop_value", 0.0))), f"{label}: an element outside the mask was dropped"
    if not live.any():
        return 0.0
    ratio = float((np.abs(g.astype(np.float64) - want)[live] / bound[live]).max())
    print(f"{label}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0, f"{label}: error / bound = {ratio}"
    return ratio


SHAPES = [(41, 4, 41), (6, 4, 6), (5, 4, 5), (1750, 4, 1750), (40, 3, 40), (42, 4, 43), (41, 41, 41), (41, 0, 41)]


@pytest.mark.parametrize("m", [1, 63, 65, 333])
@pytest.mark.parametrize("f,first,stride", SHAPES)
def test_against_the_restatement(eng, m, f, first, stride):
    x = rows_of(m, f, stride, seed=m + f)
    g = torch.Generator().manual_seed(1)
    s = (2.0 * torch.rand(m, generator=g)).to(DEV)
    ep = torch.randint(0, 4, (m,), generator=g).to(DEV)
    kw = dict(ON, seed=0x1234567890ABCDEF, row_offset=1000)
    got = eng.obs_noise(x, first=first, row_scale=s, episode=ep, step=2 ** 32 + 5, **kw)
    check(got, x, first, f"M {m} F {f} first {first} stride {stride}", row_scale=s.cpu().numpy(), episode=ep.cpu().numpy(), t=2 ** 32 + 5, **kw)
    if first == f:
        assert torch.equal(got, x)


@pytest.mark.parametrize("f", [5, 6])
def test_more_row_groups_than_workgroups(eng, f):
    """Past 32 768 groups of 8 rows the workgroups walk the rows with a grid stride: every row is still written once, with its own draws."""
    m = 8 * 32768 + 13
    x = rows_of(m, f, seed=3)
    got = eng.obs_noise(x, first=4, seed=9, step=1, **ON)
    check(got, x, 4, f"M {m} F {f}", seed=9, t=1, **ON)


def test_paths_give_the_same_bits(eng):
    """The 8-byte path (even stride, aligned base) and the scalar path (odd stride; a base 4 bytes off) on the same logical matrix; in
    place and out of place; a [:, t] slice of a [B, T, F] window."""
    m, f = 333, 42
    kw = dict(ON, first=4, seed=5, step=17)
    a = rows_of(m, f, 42, seed=8)
    ref = eng.obs_noise(a, **kw)
    assert torch.equal(eng.obs_noise(rows_of(m, f, 43, seed=8), **kw), ref)
    b = rows_of(m, f, 42, seed=8, offset=1)
    assert b.data_ptr() % 8 == 4 and torch.equal(eng.obs_noise(b, **kw), ref)
    out43 = rows_of(m, f, 43, seed=0)
    assert torch.equal(eng.obs_noise(a, out43, **kw), ref)                      # aligned in, odd-stride out
    for stride, offset in ((42, 0), (43, 0), (42, 1)):
        c = rows_of(m, f, stride, seed=8, offset=offset)
        keep = c[:, :4].clone()
        r = eng.obs_noise(c, c, **kw)                                            # in place
        assert r.data_ptr() == c.data_ptr() and torch.equal(c, ref) and torch.equal(c[:, :4], keep)
    g = torch.Generator().manual_seed(2)
    win = torch.randn(5, 3, 41, generator=g).to(DEV)
    src = win.clone()
    flat = eng.obs_noise(src[:, 1].contiguous(), **kw)
    eng.obs_noise(win[:, 1], win[:, 1], **kw)
    assert torch.equal(win[:, 1], flat) and torch.equal(win[:, 0], src[:, 0]) and torch.equal(win[:, 2], src[:, 2])
    fresh = torch.zeros(5, 3, 41, device=DEV)
    eng.obs_noise(src[:, 1], fresh[:, 2], **kw)                                  # out of place between two windows' slices
    assert torch.equal(fresh[:, 2], flat) and not fresh[:, :2].any()


def test_invariance(eng):
    m, f = 1024, 41
    x = rows_of(m, f, seed=4)
    kw = dict(ON, first=4, seed=77)
    whole = eng.obs_noise(x, step=3, **kw)
    halves = torch.cat([eng.obs_noise(x[:512], step=3, row_offset=0, **kw), eng.obs_noise(x[512:], step=3, row_offset=512, **kw)])
    assert torch.equal(whole, halves)                                            # a shard reproduces its slice of the whole
    assert torch.equal(eng.obs_noise(x, step=3, **kw), whole)                    # two runs: the same bits
    top = eng.obs_noise(x, step=3, row_offset=2 ** 32 - m, **kw)                 # the last legal row_offset
    check(top, x, 4, "row_offset 2^32 - M", t=3, row_offset=2 ** 32 - m, seed=77, **ON)
    for a, b in ((5, 9), (2 ** 32 - 1, 1), (2 ** 64 - 1, 3)):                    # t = step + *step_dev mod 2^64
        dev_word = torch.tensor([b], dtype=torch.int64, device=DEV)
        assert torch.equal(eng.obs_noise(x, step=a, step_dev=dev_word, **kw), eng.obs_noise(x, step=(a + b) % 2 ** 64, **kw))
        assert int(dev_word) == b                                                # the library never writes it
    assert not torch.equal(eng.obs_noise(x, step=4, **kw), whole)


def test_offset_draw(eng):
    m, f, first, so = 96, 41, 4, 0.25
    x = rows_of(m, f, seed=6)
    ep = torch.zeros(m, dtype=torch.int64, device=DEV)
    kw = dict(first=first, sigma_offset=so, seed=21, episode=ep)
    d0 = (eng.obs_noise(x, step=0, **kw) - x)[:, first:]
    eo, _ = R.offset_draws(21, 0, np.arange(m))
    # the same offset in every column of a row (up to the rounding of x + t_o: compare through the restatement's bound) ...
    check(eng.obs_noise(x, step=0, **kw), x, first, "offset only", sigma_offset=so, seed=21, t=0)
    zero = torch.zeros(m, f, device=DEV)
    z0 = eng.obs_noise(zero, step=0, **kw)[:, first:]
    assert torch.equal(z0, z0[:, :1].expand_as(z0)) and not torch.equal(z0[0], z0[1])      # ... exactly so on a zero input
    np.testing.assert_allclose(z0[:, 0].cpu().numpy(), so * eo, rtol=1e-5, atol=1e-7)
    assert float((d0 - z0).abs().max()) < 1e-5
    z1 = eng.obs_noise(zero, step=1, **kw)[:, first:]
    assert torch.equal(z1, z0)                                                   # the next call: the same offset
    ep[::3] += 1
    z2 = eng.obs_noise(zero, step=2, **kw)[:, first:]
    changed = (z2[:, 0] != z0[:, 0]).cpu().numpy()
    assert np.array_equal(changed, np.arange(m) % 3 == 0)                        # exactly the rows whose episode changed
    # row_scale = 0 rows are untouched by both sigmas; a sweep scales the per-row deviation linearly
    from isaac_rover_amd.learning.noise import HeightmapNoise
    sweep = HeightmapNoise.noise_sweep(0.2, m, device=DEV)
    assert float(sweep[0]) == 0.0 and float(sweep[-1]) == 1.0
    got = eng.obs_noise(x, first=first, sigma_point=0.2, sigma_offset=0.2, row_scale=sweep, seed=21, step=5)
    assert torch.equal(got[0], x[0])
    eps, _, _ = R.point_draws(21, 5, np.arange(m), f - first)
    unit = np.abs(0.2 * eo[:, None] + 0.2 * eps)                                 # the deviation of a row at scale 1
    dev = (got - x)[:, first:].abs().cpu().numpy().astype(np.float64)
    s = sweep.cpu().numpy().astype(np.float64)[:, None]
    assert np.all(dev <= s * unit * (1 + 1e-5) + 1e-5) and np.all(dev >= s * unit * (1 - 1e-5) - 1e-5)


def test_all_off_returns_the_input(eng):
    x = rows_of(65, 41, seed=7)
    x[3, 10], x[4, 11], x[5, 2], x[6, 12], x[7, 13] = -0.0, 0.0, -0.0, float("inf"), 1e-42
    got = eng.obs_noise(x, first=4, seed=3, step=9)
    assert torch.equal(got, x)                                                   # by value: -0.0 == +0.0
    sign = torch.signbit(got)
    assert not bool(sign[3, 10]) and bool(torch.signbit(x[3, 10]))               # a heightmap -0.0 comes out as +0.0
    assert bool(sign[5, 2])                                                      # a copied column keeps its bits
    assert torch.equal(got[:, :4].view(torch.int32), x[:, :4].view(torch.int32))
    # row_scale = 0 with the sigmas on: the same
    got = eng.obs_noise(x, first=4, sigma_point=0.3, sigma_offset=0.3, row_scale=torch.zeros(65, device=DEV), seed=3, step=9)
    assert torch.equal(got, x)
    # dropout alone reads words 2 and 3 of the same Philox call: the mask of the full model
    both = eng.obs_noise(x, first=4, seed=3, step=9, **ON)
    drop = eng.obs_noise(x, first=4, dropout=0.1, drop_value=-1.0, seed=3, step=9)
    mask = drop[:, 4:] != x[:, 4:]
    assert 0.02 < float(mask.float().mean()) < 0.2 and torch.equal(both[:, 4:][mask], drop[:, 4:][mask]) and bool((drop[:, 4:][mask] == -1.0).all())
    assert not bool((both[:, 4:][~mask] == -1.0).any())
    assert bool((eng.obs_noise(x, first=4, dropout=1.0, drop_value=2.5)[:, 4:] == 2.5).all())


def test_refusals_with_a_ctx(eng):
    """The Python layer's checks, and one refusal of the C layer through a live ctx (the rest: tests/test_obs_noise_host.py)."""
    from isaac_rover_amd._lib import RoverError
    x = rows_of(8, 10)
    for bad in (dict(obs=x.double()), dict(obs=x.cpu()), dict(obs=x.t()), dict(obs=x, out=torch.empty(8, 11, device=DEV)),
                dict(obs=x, row_scale=torch.zeros(7, device=DEV)), dict(obs=x, episode=torch.zeros(8, device=DEV)),
                dict(obs=x, step_dev=torch.zeros(1, device=DEV)), dict(obs=x, sigma_point=-1.0), dict(obs=x, dropout=2.0), dict(obs=x, first=11)):
        kw = dict(first=4)
        kw.update(bad)
        with pytest.raises(RoverError):
            eng.obs_noise(kw.pop("obs"), **kw)
    big = torch.zeros(100, device=DEV)
    with pytest.raises(RoverError, match="overlaps in"):
        eng.obs_noise(big[:80].view(8, 10), big[4:84].view(8, 10), first=4)
    assert eng.obs_noise(torch.empty(0, 10, device=DEV), first=4).shape == (0, 10)


def test_heightmap_noise_eager_and_captured(eng):
    from isaac_rover_amd.learning.noise import HeightmapNoise
    e, f = 64, 41
    noise = HeightmapNoise(eng, P37, seed=31, **ON)
    obs = [rows_of(e, f, seed=40 + i) for i in range(5)]
    resets = [torch.zeros(e, dtype=torch.bool, device=DEV) for _ in range(5)]
    resets[1][::5] = True
    resets[2][1::7] = True
    first = noise.apply(obs[0], reset=resets[0])                                # the warm-up call
    check(first, obs[0], 4, "HeightmapNoise call 0", seed=31, t=0, **ON)
    assert int(noise.counter) == 1 and not bool(noise.episode.any())
    second = noise.apply(obs[0])
    assert not torch.equal(second[:, 4:], first[:, 4:]) and torch.equal(second[:, :4], first[:, :4])     # consecutive calls draw different noise
    start = noise.state_dict()
    want = []
    for t in range(1, 4):                                                        # three eager calls from `start`
        want.append(noise.apply(obs[t], reset=resets[t]).clone())
    end_counter, end_episode = int(noise.counter), noise.episode.clone()
    assert end_counter == int(start["counter"]) + 3
    assert torch.equal(end_episode, (resets[1].long() + resets[2].long() + resets[3].long()))            # only the flagged envs' episodes
    check(want[2], obs[3], 4, "HeightmapNoise call 4", seed=31, t=4, episode=(resets[1].long() + resets[2].long()).cpu().numpy(), **ON)
    # the same three calls as replays of one captured apply
    noise.load_state_dict(start)
    ptrs = (noise.counter.data_ptr(), noise.episode.data_ptr())
    static_obs, static_reset, static_out = obs[1].clone(), resets[1].clone(), torch.empty(e, f, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        noise.apply(static_obs, out=static_out, reset=static_reset)
    noise.load_state_dict(start)                                                 # capture runs nothing; be explicit about the start
    for t in range(1, 4):
        static_obs.copy_(obs[t])
        static_reset.copy_(resets[t])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, want[t - 1]), f"replay {t} differs from the eager call"
    assert (noise.counter.data_ptr(), noise.episode.data_ptr()) == ptrs
    assert int(noise.counter) == end_counter and torch.equal(noise.episode, end_episode)                # advanced by 3 on the device


def test_student_acts_on_a_noisy_observation(eng):
    from isaac_rover_amd.learning.noise import HeightmapNoise
    from isaac_rover_amd.learning.student import StudentPolicy
    e = 64
    obs = rows_of(e, 41, seed=12) / 3.0
    done = torch.zeros(e, dtype=torch.bool, device=DEV)
    done[::9] = True
    pol = StudentPolicy(eng, P37, device=DEV, seed=4)
    pol.init_hidden(e)
    clean = pol.act(obs, reset=done).clone()
    pol.init_hidden(e)
    noise = HeightmapNoise(eng, P37, sigma_point=0.1, sigma_offset=0.05, dropout=0.1, seed=6)
    noisy = pol.act(noise.apply(obs, reset=done), reset=done)
    assert noisy.shape == (e, 2) and bool(torch.isfinite(noisy).all()) and not torch.equal(noisy, clean)
    assert torch.equal(noise.episode, done.long())


def _example(name, *args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", name), *args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_distill_example_with_device_noise():
    out = _example("distill.py", "--envs", "64", "--window", "4", "--updates", "2", "--device-noise", "--obs-offset", "0.02", "--obs-dropout", "0.1")
    lines = [l for l in out.splitlines() if l.startswith("update ")]
    assert len(lines) == 2, out
    for l in lines:
        vals = [float(v) for v in l.replace(":", "").split()[3::2]]
        assert len(vals) == 3 and all(np.isfinite(vals)), l
    assert "rover_obs_noise" in out


def test_rollout_example_with_obs_noise():
    out = _example("rollout.py", "--policy", "student", "--envs", "64", "--steps", "8", "--obs-noise", "0.05")
    assert "8 steps x 64 envs" in out and "rover_obs_noise" in out
