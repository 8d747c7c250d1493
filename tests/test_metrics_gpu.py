"""GPU (-m gpu): the per-environment decision kernels — metrics_done_kernel, the fused obs_metrics_kernel, compact_count_kernel /
compact_write_kernel, pre_physics_kernel / ackermann_kernel — against tests/metrics_ref.py, bit for bit.

Every operation of the decision code is one correctly rounded float32 operation, so reward and the float extras are compared as
int32 views and every integer output exactly.  The restatement is fed the DEVICE'S OWN heading difference and rock-ray distances of
the same step (the pose trigonometry and the ray cast have tests of their own), so the kernel's inputs are the restatement's inputs
bit for bit: no row of the threshold table is exempted, and there is no flip budget.  The table's coverage assertions run again here
on the device's heading and distances.  All outputs sit between canary-filled guard zones."""
import dataclasses
import time

import numpy as np
import pytest
import torch

import metrics_ref as M
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CANARY = {torch.float32: -7777.25, torch.int64: -77, torch.int32: -77, torch.uint8: 0xA5}


class Guarded:
    """A contiguous tensor of ``shape`` between two canary-filled guard zones (the pattern of test_ppo_gpu.py); the window starts out
    holding the canary too, so an element no kernel wrote still shows it."""

    def __init__(self, shape, dtype=torch.float32, pad=64):
        n = int(np.prod(shape))
        self.canary = CANARY[dtype]
        self.buf = torch.full((n + 2 * pad,), self.canary, dtype=dtype, device=DEV)
        self.t = self.buf[pad:pad + n].view(shape)
        self.pad, self.n = pad, n

    def intact(self):
        return bool((self.buf[:self.pad] == self.canary).all()) and bool((self.buf[self.pad + self.n:] == self.canary).all())

    def refill(self):
        self.t.fill_(self.canary)

    def np(self):
        return self.t.cpu().numpy()


def _engine(num_envs, level=2, **kw):
    from hip_helpers import make_engine
    scene, distn = M.table_scene()
    return make_engine(scene, distn, num_envs, variant=None, curriculum_level=level, **kw)


class Run:
    """One engine's buffers: inputs on the device, every output Guarded."""

    def __init__(self, eng, st):
        e, f, i64 = eng.num_envs, torch.float32, torch.int64
        self.eng, self.e = eng, e
        self.d = {k: v.to(DEV).contiguous() for k, v in st.items()}
        self.progress0 = self.d["progress"].clone()
        self.g = dict(progress=Guarded((e,), i64), rew=Guarded((e,)), reset=Guarded((e,), i64), rock_collision=Guarded((e,), i64),
                      reset_ids=Guarded((e,), i64), n_reset=Guarded((1,), torch.int32), heading_diff=Guarded((e,)),
                      wheel_dist=Guarded((e, 24)), body_dist=Guarded((e, 2)), done_u8=Guarded((e,), torch.uint8),
                      obs=Guarded((e, eng.num_observations)))
        self.ex = {k: Guarded((e,), i64 if k == "collision_penalty" else f) for k in M.EXTRAS}
        d = self.d
        self.sin = eng.make_in(d["pos"], d["quat"], d["joints"], d["target"], d["lin_hist"], d["ang_hist"], d["euler_pre"],
                               self.g["progress"].t)
        g = self.g
        self.sout = eng.make_out(g["obs"].t, rew=g["rew"].t, reset=g["reset"].t, rock_collision=g["rock_collision"].t,
                                 extras={k: v.t for k, v in self.ex.items()}, reset_ids=g["reset_ids"].t, n_reset=g["n_reset"].t,
                                 heading_diff=g["heading_diff"].t, wheel_dist=g["wheel_dist"].t, body_dist=g["body_dist"].t,
                                 done_u8=g["done_u8"].t)

    def prepare(self, rock_fill=None):
        for v in list(self.g.values()) + list(self.ex.values()):
            v.refill()
        self.g["progress"].t.copy_(self.progress0)
        if rock_fill is not None:
            self.g["rock_collision"].t.copy_(rock_fill)

    def fused(self, increment):
        self.eng.step(self.sin, self.sout, increment_progress=increment, compact=True)

    def split(self, increment, between=None):
        if increment:
            self.g["progress"].t.add_(1)                    # rl_task.py:250, the caller's in the reference's method split
        self.eng.get_observations(self.sin, self.sout)
        if between is not None:
            between()
        self.eng.calculate_metrics(self.sin, self.sout)
        self.eng.is_done(self.sin, self.sout)
        self.eng.compact_resets(self.g["reset"].t, self.g["reset_ids"].t, self.g["n_reset"].t)

    def read(self):
        torch.cuda.synchronize()
        out = {k: v.np() for k, v in self.g.items()}
        out.update({"extras_" + k: v.np() for k, v in self.ex.items()})
        for k, v in list(self.g.items()) + list(self.ex.items()):
            assert v.intact(), f"a write outside the output {k}"
        return out


def _check(got, st, cfg, label, rock_in=None, code_in=None, step_in=None, exact=True, cover=True):
    """The device's outputs of one step against the restatement on the device's own heading and distances."""
    want = M.restate(st, got["heading_diff"], got["wheel_dist"], got["body_dist"], cfg, rock_collision_in=rock_in,
                     eval_code_in=code_in, eval_step_in=step_in)
    M.compare_bits(got, want, label, int_keys=("rock_collision", "reset", "progress", "extras_collision_penalty"))
    np.testing.assert_array_equal(got["done_u8"], want["reset"].astype(np.uint8), err_msg=f"{label}: done_u8")
    ids = np.nonzero(want["reset"])[0]
    n = int(got["n_reset"][0])
    assert n == len(ids), f"{label}: n_reset {n}, {len(ids)} envs are done"
    np.testing.assert_array_equal(got["reset_ids"][:n], ids, err_msg=f"{label}: reset_ids")
    assert (got["reset_ids"][n:] == CANARY[torch.int64]).all(), f"{label}: reset_ids written beyond n_reset"
    if cover:
        counts = M.coverage(want, cfg, exact=exact)
        print(f"[{label}] coverage on the device's heading and distances: {counts}")
    return want


def _three_ways(eng, st, cfg, label, exact=True):
    """Fused with and without the increment, and the reference's method split: each against the restatement, each run twice."""
    run = Run(eng, st)
    wants = {}
    for mode in ("fused+inc", "fused", "split+inc"):
        inc = mode.endswith("+inc")
        go = (lambda: run.fused(inc)) if mode.startswith("fused") else (lambda: run.split(inc))
        run.prepare()
        go()
        got = run.read()
        c = dataclasses.replace(cfg, increment=inc)
        _check(got, st, c, f"{label} {mode}", exact=exact, cover=(mode == "fused+inc"))
        wants[mode] = got
        run.prepare()
        go()
        again = run.read()
        for k in got:
            assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), f"{label} {mode}: {k} differs on the second run"
    # the split path computes what the fused one does
    for k in wants["fused+inc"]:
        assert np.array_equal(wants["fused+inc"][k].view(np.uint8), wants["split+inc"][k].view(np.uint8)), f"{label}: fused and split differ in {k}"


CASES = {
    "level0": dict(cfg=M.Config(level=0)),
    "level1": dict(cfg=M.Config(level=1)),
    "level2": dict(cfg=M.Config(level=2)),
    "level3": dict(cfg=M.Config(level=3)),
    "level2_A": dict(cfg=M.Config(level=2, max_episode_length=7, num_envs_global=5 * M.TABLE_ENVS, rewards=M.REWARDS_A)),
    "level2_e333": dict(cfg=M.Config(level=2), num_envs=333),       # 256 + 64 + 13: a partial last block and a partial last wave
}


@pytest.mark.parametrize("label", sorted(CASES))
def test_decisions_bit_equal_on_threshold_table(label):
    case = CASES[label]
    cfg = case["cfg"]
    e = case.get("num_envs", M.TABLE_ENVS)
    st, _ = M.threshold_table(num_envs=e, max_episode_length=cfg.max_episode_length)
    t0 = time.time()
    eng = _engine(e, level=cfg.level, max_episode_length=cfg.max_episode_length, num_envs_global=cfg.num_envs_global,
                  rewards=cfg.rewards)
    _three_ways(eng, st, cfg, label)
    eng.close()
    print(f"[{label}] {time.time() - t0:.2f} s")


@pytest.mark.parametrize("level", [0, 1])
def test_low_levels_never_read_rock_collision(level):
    """rover.py:292,514,645: below level 2 check_collision is not called and neither calculate_metrics nor is_done reads
    rock_collison.  Here the collision stage (fused step, get_observations) reports 0 there; calculate_metrics / is_done on their
    own leave the caller's array alone and give the same reward, extras and resets whatever it holds."""
    cfg = M.Config(level=level)
    st, _ = M.threshold_table()
    e = M.TABLE_ENVS
    eng = _engine(e, level=level)
    run = Run(eng, st)
    pattern = (torch.arange(e, device=DEV) % 3 == 0).to(torch.int64)
    run.prepare(rock_fill=pattern)
    run.fused(True)
    fused = run.read()
    assert not fused["rock_collision"].any(), "the fused step's collision stage must report 0 below level 2"
    want = _check(fused, st, cfg, f"level {level} fused, rock_collision pre-filled", cover=False)
    assert not want["extras_collision_penalty"].any()

    run.prepare(rock_fill=pattern)
    seen = {}

    def between():          # get_observations ran its collision stage; the caller overwrites the array before the other two calls
        seen["after_obs"] = run.g["rock_collision"].t.clone()
        run.g["rock_collision"].t.copy_(pattern)
    run.split(True, between=between)
    split = run.read()
    assert not seen["after_obs"].any(), "get_observations' collision stage must report 0 below level 2"
    np.testing.assert_array_equal(split["rock_collision"], pattern.cpu().numpy(), err_msg="calculate_metrics / is_done wrote rock_collision")
    c = M.Config(level=level, increment=False, collision=False)
    stp = dict(st, progress=st["progress"] + 1)
    _check(split, stp, c, f"level {level} split, rock_collision pre-filled", rock_in=pattern.cpu().numpy(), cover=False)
    for k in M.FLOAT_OUTPUTS + ("reset", "done_u8", "extras_collision_penalty", "reset_ids", "n_reset"):
        assert np.array_equal(fused[k].view(np.uint8), split[k].view(np.uint8)), f"level {level}: fused and split differ in {k}"
    eng.close()


@pytest.mark.parametrize("fused", [True, False])
def test_evaluation_latch_on_threshold_table(fused):
    """Evaluation on (as test_eval_gpu.py turns it on): three consecutive steps on the table rotated by a different number of rows each
    time, so that from the second step on the prior codes are mixed — latched envs, which must keep code and step whatever now holds
    for them, and pending ones.  Codes, latch steps and summary8 against the restatement."""
    e = M.TABLE_ENVS
    cfg = M.Config(level=2, evaluation=True, increment=fused)
    base, _ = M.threshold_table()
    eng = _engine(e, level=2)
    eng.set_evaluation(True)
    code, step = np.zeros(e, np.int64), np.zeros(e, np.int64)
    res, stp, summ = Guarded((e,), torch.int64), Guarded((e,), torch.int64), Guarded((8,), torch.int64)
    for k, shift in enumerate((0, 97, 211)):
        st = {key: torch.roll(v, shift, 0).contiguous() for key, v in base.items()}
        run = Run(eng, st)
        run.prepare()
        run.fused(True) if fused else run.split(True)
        got = run.read()
        stc = st if fused else dict(st, progress=st["progress"] + 1)
        want = _check(got, stc, cfg, f"eval step {k}", code_in=code, step_in=step, cover=(k == 0))
        eng.eval_read(res.t, stp.t, summ.t)
        torch.cuda.synchronize()
        r, s, sm = res.np(), stp.np(), summ.np()
        np.testing.assert_array_equal(r, want["eval_code"], err_msg=f"step {k}: codes")
        np.testing.assert_array_equal(s, want["eval_step"], err_msg=f"step {k}: latch steps")
        np.testing.assert_array_equal(sm[0:4], np.bincount(want["eval_code"], minlength=4)[:4])
        np.testing.assert_array_equal(sm[4:8], [int(want["eval_step"][want["eval_code"] == c].sum()) for c in range(4)])
        assert res.intact() and stp.intact() and summ.intact()
        if k > 0:
            latched = code != 0
            assert latched.sum() >= 16 and (~latched).sum() >= 16, "the prior codes are not mixed"
            assert np.array_equal(r[latched], code[latched]) and np.array_equal(s[latched], step[latched])
            # the latch is seen to hold: some latched env would have taken another code from this step's state
            fresh = M.restate(stc, got["heading_diff"], got["wheel_dist"], got["body_dist"], cfg)["eval_code"]
            assert ((fresh != code) & latched & (fresh != 0)).sum() >= 4
        code, step = want["eval_code"], want["eval_step"]
    eng.close()


# ---- compaction on its own -------------------------------------------------------------------------------------------------
def _flag_patterns(n):
    rng = np.random.default_rng(n)
    pats = {"none": np.zeros(n, np.int64), "all": np.ones(n, np.int64)}
    pats["first"] = np.zeros(n, np.int64); pats["first"][0] = 1
    pats["last"] = np.zeros(n, np.int64); pats["last"][n - 1] = 1
    one = np.zeros(n, np.int64)
    for b in range((n + 255) // 256):                           # one flag per 256-env block, at a lane that moves with the block
        one[min(b * 256 + (b * 37) % 256, n - 1)] = 1
    pats["one_per_block"] = one
    for name, p in (("p01", 0.01), ("p50", 0.5), ("p99", 0.99)):
        pats[name] = (rng.random(n) < p).astype(np.int64) * rng.integers(1, 1 << 40, n)        # any non-zero value is a flag
    if n > 65536:
        late = np.zeros(n, np.int64)
        late[65536:] = (rng.random(n - 65536) < 0.5)
        pats["blocks_from_256"] = late                          # the prefix of these blocks takes the loop's second trip
    return pats


@pytest.mark.parametrize("n,offset", [(255, 0), (256, 0), (257, 5000), (65536 + 300, 0), (65536 + 300, 123456789)])
def test_compact_resets(n, offset):
    """nonzero(reset) + env_offset, ascending; ids beyond n_reset untouched.  65 836 envs are 258 blocks: blocks 256 and 257 sum the
    counts before them in two trips of the 256-wide prefix loop."""
    from isaac_rover_amd import _lib
    t0 = time.time()
    eng = _lib.Engine(n, device=0, env_offset=offset)
    for name, flags in _flag_patterns(n).items():
        reset = Guarded((n,), torch.int64)
        reset.t.copy_(torch.from_numpy(flags))
        ids, cnt = Guarded((n,), torch.int64), Guarded((1,), torch.int32)
        for attempt in range(2):
            ids.refill(), cnt.refill()
            eng.compact_resets(reset.t, ids.t, cnt.t)
            torch.cuda.synchronize()
            want = np.nonzero(flags)[0] + offset
            got, k = ids.np(), int(cnt.np()[0])
            assert k == len(want), f"n={n} {name}: n_reset {k}, want {len(want)}"
            np.testing.assert_array_equal(got[:k], want, err_msg=f"n={n} {name}")
            assert (got[k:] == CANARY[torch.int64]).all(), f"n={n} {name}: ids written beyond n_reset"
            assert ids.intact() and cnt.intact() and reset.intact()
            np.testing.assert_array_equal(reset.np(), flags)
    eng.close()
    print(f"[compact n={n}] {time.time() - t0:.2f} s")


# ---- Ackermann and pre-physics -----------------------------------------------------------------------------------------------
# Largest error observed on the MI355X over ackermann_table() against the float64 run (EXPERIMENTS.md §17), in float32 ulp — steer in ulp
# of the unwrapped angle; vel's 40 ulp is float32 rounding of Px amplified where Px - 0.447 cancels, the same figure the float32
# restatement has, to which vel is bit-equal.  The bound is twice the observed figure.
STEER_ULP_MEASURED, VEL_ULP_MEASURED = 1.987, 40.180


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_ackermann_and_pre_physics():
    from isaac_rover_amd import _lib
    lin, ang = M.ackermann_table()
    n = len(lin)
    eng = _lib.Engine(n, device=0)
    steer_g, vel_g = eng.ackermann(torch.from_numpy(lin).to(DEV), torch.from_numpy(ang).to(DEV))
    # the second entry point: pre_physics_step scatters the same values into the 13-joint layout (rover.py:400-414)
    g = load_golden("pre_physics_step")
    pos_idx, vel_idx = g["out_pos_joint_indices"], g["out_vel_joint_indices"]
    rng = np.random.default_rng(3)
    lin_h, ang_h = rng.uniform(-1, 1, (n, 3)).astype(np.float32), rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    nn = rng.uniform(-1, 1, (n, 2, 3)).astype(np.float32)
    quat = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    lh, ah, an = Guarded((n, 3)), Guarded((n, 3)), Guarded((n, 2, 3))
    lh.t.copy_(torch.from_numpy(lin_h)), ah.t.copy_(torch.from_numpy(ang_h)), an.t.copy_(torch.from_numpy(nn))
    pt, vt, ep = Guarded((n, 13)), Guarded((n, 13)), Guarded((n, 3))
    actions = torch.from_numpy(np.stack((lin, ang), axis=1)).to(DEV).contiguous()
    eng.pre_physics_step(actions, torch.from_numpy(quat).to(DEV), lh.t, ah.t, euler_pre=ep.t, pos_targets13=pt.t, vel_targets13=vt.t,
                         actions_nn=an.t)
    torch.cuda.synchronize()
    steer, vel = steer_g.cpu().numpy(), vel_g.cpu().numpy()
    for x in (lh, ah, an, pt, vt, ep):
        assert x.intact()
    # exact: the two entry points agree, the joints no wheel maps to are untouched, the histories shift
    p13, v13 = pt.np(), vt.np()
    assert np.array_equal(_bits(p13[:, pos_idx]), _bits(steer[:, [1, 5, 0, 4]])), "pre_physics_step and ackermann: steering differs"
    assert np.array_equal(_bits(v13[:, vel_idx]), _bits(vel[:, [1, 3, 5, 0, 2, 4]])), "pre_physics_step and ackermann: velocities differ"
    assert (np.delete(p13, pos_idx, axis=1) == CANARY[torch.float32]).all() and (np.delete(v13, vel_idx, axis=1) == CANARY[torch.float32]).all()
    assert np.array_equal(_bits(lh.np()), _bits(np.stack((lin, lin_h[:, 0], lin_h[:, 1]), axis=1)))
    assert np.array_equal(_bits(ah.np()), _bits(np.stack((ang, ang_h[:, 0], ang_h[:, 1]), axis=1)))
    want_nn = np.concatenate((np.stack((lin, ang), axis=1)[:, :, None], nn), axis=2)[:, :, 0:3]        # rover.py:389
    assert np.array_equal(_bits(an.np()), _bits(want_nn))
    assert np.array_equal(ep.np(), np.zeros((n, 3), np.float32))           # identity orientation

    # branch choices: the float32 restatement's.  vel is IEEE operations only (divide, square root, multiply): bit-equal to it
    s32, v32, br = M.ackermann(lin, ang)
    s64, v64, _ = M.ackermann(lin, ang, np.float64, br)
    unwrapped = np.arctan2(np.broadcast_to(M.WHEELS[None, :, 1].astype(np.float64), s64.shape),
                           M.WHEELS[None, :, 0].astype(np.float64) - br["px"].astype(np.float64)[:, None])
    near_wrap = (np.abs(unwrapped.astype(np.float32) - M.WRAP_LO) <= np.spacing(M.WRAP_HI)) | \
                (np.abs(unwrapped.astype(np.float32) - M.WRAP_HI) <= np.spacing(M.WRAP_HI))
    print(f"rows within 1 ulp of a wrap threshold: {int(near_wrap.sum())}")
    assert near_wrap.sum() <= 4
    assert np.array_equal(_bits(vel), _bits(v32)), "vel: a branch (Px zeroed, dist > 1000) or an IEEE operation differs from the restatement"
    s_err = M.steer_ulp(steer, s64, unwrapped)
    s_err = np.where(near_wrap & (np.abs(np.abs(steer.astype(np.float64) - s64) - np.pi) < 1e-5), 0.0, s_err)
    assert float(s_err.max()) < 64, f"steer: a wrap taken differently from the restatement (row {int(s_err.max(axis=1).argmax())})"
    v_err = M.ulp_diff(vel, v64)
    print(f"ackermann on the device vs the float64 run: steer {float(s_err.max()):.3f} ulp (of the unwrapped angle), "
          f"vel {float(v_err.max()):.3f} ulp; steer bits differing from numpy's float32 arctan2: {int((_bits(steer) != _bits(s32)).sum())} of {steer.size}")
    assert float(s_err.max()) <= 2 * STEER_ULP_MEASURED
    assert float(v_err.max()) <= 2 * VEL_ULP_MEASURED
    eng.close()
