"""GPU: rover_obs_occlusion (csrc/rover_occlusion.hip) against the float32 restatement (tests/occlusion_ref.py) bit for bit — out, the
mask and the measured points, no column left out —, the frame tied to the step's own hit points, the invariances (in place, window
slices, a noisy input, shards, repetition, graph replay, the two routes), the edges, and the composition with HeightmapNoise on a task."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import occlusion_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD_SEED = 0              # chosen on the CPU: every case below hides and shows at least 200 columns (asserted)
FILL = 12345.0              # what the optional outputs hold before a call: a column the call must not write keeps it
# The frame test's bound: ten times the largest |target3 - hit_pt| measured over seeds 0 .. 3, 1.431e-6 m (EXPERIMENTS.md §30; three ulp
# of a coordinate near 6 m), and never above 1e-3 m
FRAME_BOUND = min(10 * 1.431e-6, 1e-3)


@functools.lru_cache(maxsize=None)
def distribution(name):
    from isaac_rover_amd import synth
    from isaac_rover_amd.tasks.utils.heightmap_distribution import generate_native
    return generate_native() if name == "native" else synth.ray_distribution(name)


@functools.lru_cache(maxsize=None)
def field():
    return R.make_field(FIELD_SEED)


@functools.lru_cache(maxsize=None)
def case(name, envs, first, seed=0):
    """A seeded case and the restatement's answer, computed once per module run and never written to."""
    body = R.body_points(*distribution(name))
    c = R.make_case(field(), body, envs, seed=seed, first=first)
    c["ref"] = R.occlude(field(), body, c["pos"], c["quat"], c["clean"], first=first)
    for v in [v for k, v in c.items() if k != "ref"] + list(c["ref"].values()):
        v.setflags(write=False)
    return c


@pytest.fixture(scope="module")
def engines():
    from isaac_rover_amd import _lib
    made = {}
    for name in ("native", "37"):
        e = _lib.Engine(8, device=0)
        e.set_distribution(*distribution(name))
        e.set_heightfield(field().hm, float(field().hscale), 1.0, (0.0, 0.0))
        e.configure_occlusion()
        made[name] = e
    yield made
    for e in made.values():
        e.close()


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                    # a copy: the cases are read-only


def run(eng, c, first, in_=None, out=None, outputs=True, **kw):
    """-> (out, hidden, target) as numpy; the optional outputs start from FILL."""
    m, cols = c["clean"].shape[0], c["clean"].shape[1] - first
    hidden = torch.full((m, cols), 77, dtype=torch.uint8, device=DEV) if outputs else None
    target = torch.full((m, cols, 3), FILL, device=DEV) if outputs else None
    got = eng.obs_occlusion(dev(c["clean"]), in_, out, first=first, pos=dev(c["pos"]), quat=dev(c["quat"]), hidden=hidden, target=target, **kw)
    torch.cuda.synchronize()
    return got.cpu().numpy(), None if hidden is None else hidden.cpu().numpy(), None if target is None else target.cpu().numpy()


def same_as_ref(got, hidden, target, ref, label):
    assert np.array_equal(hidden, ref["hidden"]), f"{label}: {int((hidden != ref['hidden']).sum())} mask entries differ"
    assert np.array_equal(R.bits(got), R.bits(ref["out"])), f"{label}: out differs"
    has = ref["has_point"]
    assert np.array_equal(R.bits(target[has]), R.bits(ref["target"][has])), f"{label}: a measured point differs in its bits"
    assert (target[~has] == np.float32(FILL)).all(), f"{label}: a column without a point had its target written"


CASES = [("native", 1, 4), ("native", 65, 4), ("native", 333, 4), ("37", 333, 0), ("37", 333, 4)]       # F = 1750, 1750, 1750, 37 and 41 (both odd)


@pytest.mark.parametrize("name,envs,first", CASES)
def test_against_the_restatement(engines, name, envs, first):
    c = case(name, envs, first)
    ref = c["ref"]
    n_hidden, n_shown = int(ref["hidden"].sum()), int((ref["hidden"] == 0).sum())
    print(f"{name} E={envs}: the restatement hides {n_hidden} and shows {n_shown} columns ({int((~ref['has_point']).sum())} without a point)")
    assert n_hidden >= 200 and n_shown >= 200 and (~ref["has_point"]).any()                     # not vacuous
    for route in (1, 0):
        engines[name].set_option("occlusion_route", route)
        same_as_ref(*run(engines[name], c, first), ref, f"{name} E={envs} route {route}")
    engines[name].set_option("occlusion_route", 1)


def _step_with_hit_points(eng, st):
    """One rover_step with hit_pt requested -> (obs [E, 4 + C], hit_pt [E, P, 3]) on the device."""
    from hip_helpers import EXTRA_DT
    from isaac_rover_amd import _lib
    e = eng.num_envs
    d = {k: v.to(DEV).contiguous() for k, v in st.items()}
    sin = eng.make_in(d["pos"], d["quat"], d["joints"], d["target"], d["lin_hist"], d["ang_hist"], d["euler_pre"], d["progress"].clone())
    i64 = torch.int64
    obs, hit = torch.zeros(e, eng.num_observations, device=DEV), torch.zeros(e, eng.P, 3, device=DEV)
    sout = eng.make_out(obs, rew=torch.zeros(e, device=DEV), reset=torch.ones(e, dtype=i64, device=DEV), rock_collision=torch.zeros(e, dtype=i64, device=DEV),
                        reset_ids=torch.full((e,), -1, dtype=i64, device=DEV), n_reset=torch.zeros(1, dtype=torch.int32, device=DEV),
                        extras={k: torch.zeros(e, dtype=EXTRA_DT[k], device=DEV) for k in _lib.EXTRAS}, hit_pt=hit)
    eng.step(sin, sout, increment_progress=True, compact=True)
    torch.cuda.synchronize()
    return obs, hit


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_frame_agrees_with_the_steps_hit_points(seed):
    """target3 is rebuilt from (pose, body point, obs) by f32 quaternion rotation; the step's hit_pt comes from its Euler route and the
    ray cast.  They must name the same point: a few ulp at the coordinates' magnitude, where a swapped axis or a sign shows as decimetres."""
    from isaac_rover_amd import _lib, synth
    scene = synth.make_scene(n_cells=64, k=16, n_stones=16)
    pts, sp, de = synth.ray_distribution("37")
    e = 64
    st = synth.make_states(e, 6.4, seed=seed)
    eng = _lib.Engine(e, device=0)
    try:
        eng.set_scene(scene, (pts, sp, de))
        eng.configure_occlusion()
        obs, hit = _step_with_hit_points(eng, st)
        target = torch.full((e, len(sp) + len(de), 3), FILL, device=DEV)
        eng.obs_occlusion(obs, first=4, pos=st["pos"].to(DEV), quat=st["quat"].to(DEV), target=target)
        torch.cuda.synchronize()
        below = (obs[:, 4:].abs() < 5.0).cpu().numpy()
        cols = np.concatenate([sp, de])
        diff = np.abs(target.cpu().numpy().astype(np.float64) - hit.cpu().numpy().astype(np.float64)[:, cols])[below]
        print(f"seed {seed}: {int(below.sum())} of {below.size} columns below miss, largest |target3 - hit_pt| = {diff.max():.3e} m")
        assert below.sum() >= below.size // 2
        assert float(diff.max()) <= FRAME_BOUND
        assert (target.cpu().numpy()[~below] == np.float32(FILL)).all()
    finally:
        eng.close()


def test_invariances_bit_for_bit(engines):
    eng, first = engines["native"], 4
    c = case("native", 65, first)
    ref, m, f = c["ref"], 65, c["clean"].shape[1]
    clean, pos, quat = dev(c["clean"]), dev(c["pos"]), dev(c["quat"])
    kw = dict(first=first, pos=pos, quat=quat)
    want = dev(ref["out"])
    eq = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))                     # bits: the case holds NaNs
    assert eq(eng.obs_occlusion(clean, **kw), want) and eq(eng.obs_occlusion(clean, **kw), want)               # two runs
    # a noisy input, out of place and in place: visible columns carry its bits, hidden ones drop_value
    g = torch.Generator().manual_seed(5)
    noisy = clean + 0.1 * torch.randn(m, f, generator=g).to(DEV)
    hid = dev(ref["hidden"]).bool()
    want_noisy = noisy.clone()
    want_noisy[:, first:] = torch.where(hid, torch.full_like(noisy[:, first:], -2.5), noisy[:, first:])
    out = eng.obs_occlusion(clean, noisy, drop_value=-2.5, **kw)
    assert eq(out, want_noisy) and bool((out[:, first:][hid] == -2.5).all()) and eq(out[:, first:][~hid], noisy[:, first:][~hid])
    x = noisy.clone()
    assert eng.obs_occlusion(clean, x, x, drop_value=-2.5, **kw) is x and eq(x, want_noisy)                    # in place
    # a [B, T, F] window's row as out, guard rows untouched; and as in and out at once
    win = torch.full((m, 3, f), 99.0, device=DEV)
    eng.obs_occlusion(clean, noisy, win[:, 1], drop_value=-2.5, **kw)
    assert eq(win[:, 1], want_noisy) and bool((win[:, 0] == 99.0).all()) and bool((win[:, 2] == 99.0).all())
    win[:, 2] = noisy
    eng.obs_occlusion(clean, win[:, 2], win[:, 2], drop_value=-2.5, **kw)
    assert eq(win[:, 2], want_noisy) and eq(win[:, 1], want_noisy) and bool((win[:, 0] == 99.0).all())
    # two halves with their own pose slices against the whole
    h = 32
    halves = torch.cat([eng.obs_occlusion(clean[:h], first=first, pos=pos[:h], quat=quat[:h]),
                        eng.obs_occlusion(clean[h:], first=first, pos=pos[h:].contiguous(), quat=quat[h:].contiguous())])
    assert eq(halves, want)
    # graph replay against eager, both routes
    for route in (0, 1):
        eng.set_option("occlusion_route", route)
        s_clean, s_out, s_hidden = clean.clone(), torch.zeros(m, f, device=DEV), torch.zeros(m, f - first, dtype=torch.uint8, device=DEV)
        eng.obs_occlusion(s_clean, None, s_out, hidden=s_hidden, **kw)                                         # warm-up
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            eng.obs_occlusion(s_clean, None, s_out, hidden=s_hidden, **kw)
        s_out.zero_()
        s_hidden.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert eq(s_out, want) and torch.equal(s_hidden.bool(), hid), f"route {route}: the replay differs from the restatement"
    eng.set_option("occlusion_route", 1)


def test_edges(engines):
    from isaac_rover_amd._lib import RoverError
    eng = engines["37"]
    # E = 0
    z = lambda *s: torch.zeros(*s, device=DEV)
    assert eng.obs_occlusion(z(0, 41), first=4, pos=z(0, 3), quat=z(0, 4)).shape == (0, 41)
    # more envs than the grid cap (4 096 workgroups): rows beyond it are walked with the grid stride
    c = case("37", 4133, 4)
    for route in (1, 0):
        eng.set_option("occlusion_route", route)
        same_as_ref(*run(eng, c, 4), c["ref"], f"4133 envs, route {route}")
    eng.set_option("occlusion_route", 1)
    # every column at miss: nothing hidden, out equals in, no target written
    small = case("37", 333, 4)
    allmiss = dict(small, clean=np.where(np.arange(41)[None, :] >= 4, np.float32(5.0), small["clean"]))
    noisy = dev(small["clean"]) + 0.5
    got, hidden, target = run(eng, allmiss, 4, in_=noisy)
    assert not hidden.any() and np.array_equal(R.bits(got), R.bits(noisy.cpu().numpy())) and (target == np.float32(FILL)).all()
    # the camera far outside the map: every sample clamps to the border nodes
    far = dict(small, pos=small["pos"] + np.array([-60.0, 45.0, 0.0], dtype=np.float32))
    far["ref"] = R.occlude(field(), R.body_points(*distribution("37")), far["pos"], far["quat"], far["clean"], first=4)
    for route in (1, 0):
        eng.set_option("occlusion_route", route)
        same_as_ref(*run(eng, far, 4), far["ref"], f"camera outside the map, route {route}")
    eng.set_option("occlusion_route", 1)
    # the Python layer's checks and the state's
    clean, pos, quat = dev(small["clean"]), dev(small["pos"]), dev(small["quat"])
    for bad in (dict(first=5), dict(pos=pos[:, :2]), dict(quat=quat.double()), dict(hidden=torch.zeros(333, 37, device=DEV)),
                dict(target=torch.zeros(333, 37, device=DEV)), dict(out=clean), dict(in_=clean[:, :40])):
        kw = dict(first=4, pos=pos, quat=quat)
        kw.update(bad)
        with pytest.raises(RoverError):
            eng.obs_occlusion(clean, kw.pop("in_", None), kw.pop("out", None), **kw)


def test_tables_are_keyed_on_the_distribution_and_the_heightfield():
    from isaac_rover_amd import _lib
    c = case("37", 333, 4)
    eng = _lib.Engine(8, device=0)
    try:
        clean, pos, quat = dev(c["clean"]), dev(c["pos"]), dev(c["quat"])
        call = lambda: eng.obs_occlusion(clean, first=4, pos=pos, quat=quat)
        with pytest.raises(_lib.RoverError, match="rover_set_distribution"):
            call()
        eng.set_distribution(*distribution("37"))
        with pytest.raises(_lib.RoverError, match="rover_set_heightfield"):
            eng.configure_occlusion()
        eng.set_heightfield(field().hm, float(field().hscale), 1.0, (0.0, 0.0))
        with pytest.raises(_lib.RoverError, match="rover_set_occlusion first"):
            call()
        eng.configure_occlusion()
        want = dev(c["ref"]["out"])
        assert torch.equal(call().view(torch.int32), want.view(torch.int32))
        flat = np.full_like(field().hm, -1.0)                                               # below every target: nothing can hide
        eng.set_heightfield(flat, float(field().hscale), 1.0, (0.0, 0.0))
        with pytest.raises(_lib.RoverError, match=r"\(-2\).*heightfield was set again after rover_set_occlusion"):
            call()
        eng.configure_occlusion()                                                                   # the tile table is rebuilt from the new field
        assert torch.equal(call().view(torch.int32), clean.view(torch.int32)) and float(c["ref"]["target"][c["ref"]["has_point"]][:, 2].min()) > -0.9
        eng.set_heightfield(field().hm, float(field().hscale), 1.0, (0.0, 0.0))
        eng.configure_occlusion()
        assert torch.equal(call().view(torch.int32), want.view(torch.int32))
        eng.set_distribution(*distribution("37"))
        with pytest.raises(_lib.RoverError, match="distribution was set again after rover_set_occlusion"):
            call()
        eng.configure_occlusion()
        assert torch.equal(call().view(torch.int32), want.view(torch.int32))
        with pytest.raises(_lib.RoverError, match="Ns \\+ Nd"):
            eng.obs_occlusion(clean, first=3, pos=pos, quat=quat)
    finally:
        eng.close()


def test_composition_with_the_noise_on_a_task():
    """HeightmapNoise.apply, then HeightmapOcclusion.apply, on a task moved by the terrain-following motion model: hidden columns read
    drop_value exactly, the others hold the noise kernel's bits, the task's obs_buf stays as it was."""
    from isaac_rover_amd import config, synth, vec_env
    from isaac_rover_amd.learning.noise import HeightmapNoise, HeightmapOcclusion
    from isaac_rover_amd.tasks.rover import RoverTask
    e = 64
    scene = synth.make_scene(n_cells=64, k=16, n_stones=16)
    env = vec_env.VecEnv(headless=True, sim="terrain")
    g = torch.Generator().manual_seed(0)
    spawn = torch.zeros(e, 3)
    spawn[:, 0:2] = 0.15 * 6.4 + 0.7 * 6.4 * torch.rand(e, 2, generator=g)
    task = RoverTask("Rover", config.SimConfig(num_envs=e, device=DEV), env, scene=scene, distribution=synth.ray_distribution("37"))
    env.set_task(task, sim_params={"dt": 0.05}, spawn_positions=spawn)
    obs = env.reset()
    noise = HeightmapNoise(task._engine, task, sigma_point=0.05, sigma_offset=0.02, dropout=0.05, drop_value=-1.0, seed=3)
    occ = HeightmapOcclusion(task._engine, task, drop_value=-3.0)
    hidden = torch.zeros(e, occ.columns, dtype=torch.uint8, device=DEV)
    first, seen_hidden = obs.shape[1] - occ.columns, 0
    for step in range(3):
        before, task_before = obs.clone(), task.obs_buf.clone()                # (what the env hands out is the task's buffer clipped to +-5)
        x = noise.apply(obs)
        noise_bits = x.clone()
        assert occ.apply(obs, noisy=x, out=x, hidden=hidden) is x
        h = hidden.bool()
        assert bool((x[:, first:][h] == -3.0).all()) and torch.equal(x[:, first:][~h].view(torch.int32), noise_bits[:, first:][~h].view(torch.int32))
        assert torch.equal(x[:, :first], noise_bits[:, :first]) and torch.equal(obs, before) and torch.equal(task.obs_buf, task_before)
        pos, quat = task._rover.get_world_poses()
        assert torch.equal(occ.apply(obs, noisy=noise_bits, pos=pos.clone(), quat=quat.clone()).view(torch.int32), x.view(torch.int32))
        seen_hidden += int(h.sum())
        obs, _, _, _ = env.step(2 * torch.rand(e, 2, device=DEV) - 1)
    print(f"hidden columns over three steps: {seen_hidden} of {3 * e * occ.columns}")
    env.close()


def _example(name, *args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", name), *args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_examples_with_occlusion():
    out = _example("rollout.py", "--policy", "student", "--envs", "64", "--steps", "8", "--sim", "terrain", "--occlusion", "--obs-noise", "0.05")
    assert "8 steps x 64 envs" in out and "rover_obs_occlusion" in out and "% of the heightmap columns hidden at the last step" in out
    out = _example("distill.py", "--envs", "64", "--window", "4", "--updates", "2", "--occlusion", "--sight-step", "0.1")
    lines = [l for l in out.splitlines() if l.startswith("update ")]
    assert len(lines) == 2 and "rover_obs_occlusion" in out and "rover_obs_noise" in out, out
    for l in lines:
        assert all(np.isfinite([float(v) for v in l.replace(":", "").split()[3::2]])), l
