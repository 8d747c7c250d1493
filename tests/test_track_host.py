"""CPU: the episode statistics as DEFINED (tests/track_ref.py; include/rover_step.h, rover_episode_track) on a hand-written sequence whose
ring and record are written out here, the refusals of rover_episode_track that need no device (the C layer validates the descriptor
before it looks at the ctx), rover_track_sizes, and the read-out of learning/tracking.py (absent tags, combine).  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import track_ref as R


def test_symbols_declared_and_layouts():
    from isaac_rover_amd import _lib
    lib = _lib.load()
    for name in ("rover_episode_track", "rover_track_sizes"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert C.sizeof(_lib.TrackRecord) == 240
    assert [f for f, _ in _lib.TrackRecord._fields_] == ["calls", "inst_sum", "ep_count", "ep_ret_sum", "ep_ret_sumsq", "ep_len_sum", "win_calls",
                                                         "win_ret_mean_sum", "win_len_mean_sum", "comp_sum", "inst_min", "inst_max", "ep_ret_min",
                                                         "ep_ret_max", "ep_len_min", "ep_len_max", "win_ret_min", "win_ret_max", "win_len_min",
                                                         "win_len_max"]
    assert (_lib.TRACK_MAX_COMPONENTS, _lib.TRACK_MAX_WINDOW) == (R.MAX_COMPONENTS, R.MAX_WINDOW) == (16, 1024)
    fresh, want = _lib.track_fresh_record(), R.fresh_record()
    for k in R.INT_FIELDS + R.F64_FIELDS + R.F32_FIELDS:
        assert getattr(fresh, k) == want[k], k
    assert list(fresh.comp_sum) == want["comp_sum"]


@pytest.mark.parametrize("e, parts", [(0, 0), (1, 1), (256, 1), (257, 2), (65793, 258)])
def test_track_sizes(e, parts):
    """The update kernel's workgroup is 256 envs: ceil(E / 256) partials, and a scratch of the partials plus one (return, length) pair
    of 8 bytes per workgroup slot."""
    from isaac_rover_amd import _lib
    s = _lib.track_sizes(e, 100, 8)
    assert s["workgroup"] == R.WORKGROUP == 256 and s["n_partials"] == parts == R.n_partials(e)
    assert s["partial_bytes"] > 0 and s["partial_bytes"] % 8 == 0
    assert s["finished_slots"] == parts * 256
    assert s["scratch_bytes"] == parts * s["partial_bytes"] + 8 * s["finished_slots"]


def test_track_sizes_refusals():
    from isaac_rover_amd import _lib
    lib = _lib.load()
    out = _lib.TrackSizes()
    assert lib.rover_track_sizes(4, 100, 0, None) == -1 and b"track_sizes" in lib.rover_last_error(None)
    for e, w, k in ((-1, 100, 0), (4, 0, 0), (4, 1025, 0), (4, 100, -1), (4, 100, 17)):
        assert lib.rover_track_sizes(e, w, k, C.byref(out)) == -1, (e, w, k)
        with pytest.raises(_lib.RoverError):
            _lib.track_sizes(e, w, k)
    for e, w, k in ((0, 1, 0), (4, 1024, 16), (2 ** 31 - 1, 100, 8)):
        assert lib.rover_track_sizes(e, w, k, C.byref(out)) == 0, (e, w, k)
    assert out.n_partials == 2 ** 23 and out.scratch_bytes == 2 ** 23 * (out.partial_bytes + 2048)


def _valid(**over):
    from isaac_rover_amd import _lib
    kw = dict(e=300, w=100, comps=((_lib._FAKE, _lib.TRACK_F32), (_lib._FAKE, _lib.TRACK_I64)))
    kw.update(over)
    return _lib.track_desc(**kw)


INVALID = {
    "E negative": dict(e=-1),
    "W zero": dict(w=0),
    "W above 1024": dict(w=1025),
    "K negative": dict(k=-1),
    "K above 16": dict(k=17),
    "done_size 4": dict(done_size=4),
    "done_size 0": dict(done_size=0),
    "component kind 2": dict(comps=((16, 0), (16, 2))),
    "component kind -1": dict(comps=((16, -1),)),
    "NULL rewards": dict(rewards=None),
    "NULL done": dict(done=None),
    "NULL cum_reward": dict(cum_reward=None),
    "NULL cum_steps": dict(cum_steps=None),
    "NULL ring_ret": dict(ring_ret=None),
    "NULL ring_len": dict(ring_len=None),
    "NULL ring_count": dict(ring_count=None),
    "NULL record": dict(record=None),
    "NULL scratch": dict(scratch=None),
    "NULL component below K": dict(comps=((16, 0), (None, 1))),
    "NULL component below K (k given)": dict(comps=((16, 0),), k=2),
    "scratch too small": dict(scratch_bytes=8),
    "scratch not aligned": dict(scratch=20),
    "NULL ring with E = 0": dict(e=0, ring_ret=None),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_every_refusal_is_reached_with_a_null_ctx(case):
    """rover_episode_track(NULL, desc, NULL) names the descriptor's fault: the descriptor is judged before the ctx."""
    from isaac_rover_amd import _lib
    lib = _lib.load()
    rc = lib.rover_episode_track(None, C.byref(_valid(**INVALID[case])), None)
    msg = lib.rover_last_error(None)
    assert rc == -1 and b"episode_track" in msg and b"null ctx" not in msg, (case, msg)


def test_a_valid_descriptor_gets_as_far_as_the_ctx():
    from isaac_rover_amd import _lib
    lib = _lib.load()
    for d in (_valid(), _valid(done_size=8), _valid(comps=()), _valid(w=1), _valid(w=1024),
              _valid(e=0, rewards=None, done=None, cum_reward=None, cum_steps=None, scratch=None, comps=((None, 0),)),
              _valid(comps=tuple((16, i % 2) for i in range(16))), _valid(comps=((16, 0), (None, 7)), k=1)):
        assert lib.rover_episode_track(None, C.byref(d), None) == -1 and b"episode_track: null ctx" in lib.rover_last_error(None)
    assert lib.rover_episode_track(None, None, None) == -1 and b"null descriptor" in lib.rover_last_error(None)


F = np.float32
REWARDS = [[1.0, 0.5, -0.25], [0.5, 0.5, 0.25], [2.0, -1.0, 0.75], [-0.5, 0.25, 0.25], [1.0, 1.0, 1.0]]
DONE = [[0, 0, 0], [1, 0, 0], [0, 1, 1], [0, 0, 0], [1, 1, 1]]


def _hand_sequence():
    t = R.Tracker(3, window=2, n_components=2)
    out = []
    for r, d in zip(REWARDS, DONE):
        r = np.array(r, dtype=F)
        out.append(t.call(r, np.array(d, dtype=np.int64), (r * F(2), np.array([1, 2, 3], dtype=np.int64))))
    return t, out


def test_hand_written_sequence():
    """Three envs, five steps, a window of two; every figure below was worked out by hand (all values are binary fractions, so every
    sum is exact).  Episodes, in the order they finish: env 0 (1.5, 2 steps) at step 2; env 1 (0.0, 3) and env 2 (0.75, 3) at step 3;
    envs 0, 1, 2 (2.5, 3), (1.25, 2), (1.25, 2) at step 5, of which the window of two keeps the last two."""
    t, out = _hand_sequence()
    st, rec, _ = out[0]
    assert st["ring_count"] == 0 and len(st["ring_ret"]) == 0 and rec["win_calls"] == 0 and rec["ep_count"] == 0
    assert rec["win_ret_min"] == np.inf and rec["win_len_max"] == -2 ** 31 and rec["ep_len_min"] == 2 ** 31 - 1
    st, rec, _ = out[1]
    assert st["cum_reward"].tolist() == [0.0, 1.0, 0.0] and st["cum_steps"].tolist() == [0, 2, 2]
    assert st["ring_ret"].tolist() == [1.5] and st["ring_len"].tolist() == [2] and st["ring_count"] == 1
    st, rec, _ = out[2]
    assert st["cum_reward"].tolist() == [2.0, 0.0, 0.0] and st["cum_steps"].tolist() == [1, 0, 0]
    assert st["ring_ret"].tolist() == [0.75, 0.0] and st["ring_len"].tolist() == [3, 3] and st["ring_count"] == 3     # slots 1, then 0
    st, rec, _ = out[3]
    assert st["cum_reward"].tolist() == [1.5, 0.25, 0.25] and st["cum_steps"].tolist() == [2, 1, 1] and st["ring_count"] == 3
    st, rec, bounds = out[4]
    assert st["cum_reward"].tolist() == [0.0, 0.0, 0.0] and st["cum_steps"].tolist() == [0, 0, 0]
    assert st["ring_ret"].tolist() == [1.25, 1.25] and st["ring_len"].tolist() == [2, 2] and st["ring_count"] == 6
    assert st["cum_reward"].dtype == np.float32 and st["ring_ret"].dtype == np.float32
    want = dict(calls=5, inst_min=F(-1.0), inst_max=F(2.0), inst_sum=7.25, ep_count=6, ep_ret_sum=7.25, ep_ret_sumsq=12.1875, ep_ret_min=F(0.0),
                ep_ret_max=F(2.5), ep_len_sum=15, ep_len_min=2, ep_len_max=3, win_calls=4, win_ret_mean_sum=3.5, win_ret_min=F(0.0),
                win_ret_max=F(1.5), win_len_mean_sum=10.0, win_len_min=2, win_len_max=3)
    for k, v in want.items():
        assert rec[k] == v and type(rec[k]) is type(v), (k, rec[k], v)
    assert rec["comp_sum"] == [14.5, 30.0] + [0.0] * 14
    assert all(b >= 0.0 for k in R.F64_FIELDS for b in [bounds[k]]) and bounds["inst_sum"] == 15 * R.U * 10.75


def test_minimum_orders_negative_zero_below_zero():
    assert np.signbit(R.omin([0.0, -0.0], np.inf)) and np.signbit(R.omin([-0.0, 0.0], np.inf)) and not np.signbit(R.omin([0.0], np.inf))
    assert not np.signbit(R.omax([0.0, -0.0], -np.inf)) and not np.signbit(R.omax([-0.0, 0.0], -np.inf)) and np.signbit(R.omax([-0.0], -np.inf))
    assert R.omin([], np.inf) == np.inf and R.omin([3.0], F(2.0)) == 2.0


def test_readout_tags_of_the_hand_written_sequence():
    from isaac_rover_amd.learning import tracking as T
    t, _ = _hand_sequence()
    out = T.tags_of(t.raw(("twice", "count")))
    assert out["Reward / Instantaneous reward (max)"] == 2.0 and out["Reward / Instantaneous reward (min)"] == -1.0
    assert out["Reward / Instantaneous reward (mean)"] == 7.25 / 15
    assert out["Reward / Total reward (mean)"] == 0.875 and out["Reward / Total reward (max)"] == 1.5 and out["Reward / Total reward (min)"] == 0.0
    assert out["Episode / Total timesteps (mean)"] == 2.5 and out["Episode / Total timesteps (max)"] == 3 and out["Episode / Total timesteps (min)"] == 2
    assert out["Episodes / finished"] == 6 and out["Episodes / return (mean)"] == 7.25 / 6
    assert out["Episodes / return (std)"] == math.sqrt(12.1875 / 6 - (7.25 / 6) ** 2)
    assert out["Episodes / return (min)"] == 0.0 and out["Episodes / return (max)"] == 2.5
    assert out["Episodes / length (mean)"] == 2.5 and out["Episodes / length (min)"] == 2 and out["Episodes / length (max)"] == 3
    assert out["Info / twice (mean)"] == 14.5 / 15 and out["Info / count (mean)"] == 2.0
    assert set(T.SKRL_TAGS) <= set(out) and len(T.SKRL_TAGS) == 9
    assert "Reward / Total reward (mean)" in out.line() and "\n" not in out.line()


def test_readout_omits_what_has_nothing_to_report():
    """No call: only the count of finished episodes.  Calls without a finished episode: the instantaneous tags and the components, no
    window and no episode figures.  Nothing is ever NaN."""
    from isaac_rover_amd.learning import tracking as T
    t = R.Tracker(4, window=3, n_components=1)
    out = T.tags_of(t.raw(("a",)))
    assert dict(out) == {"Episodes / finished": 0}
    t.call(np.ones(4, dtype=F), np.zeros(4, dtype=bool), (np.full(4, 0.5, dtype=F),))
    out = T.tags_of(t.raw(("a",)))
    assert set(out) == {"Reward / Instantaneous reward (max)", "Reward / Instantaneous reward (min)", "Reward / Instantaneous reward (mean)",
                        "Episodes / finished", "Info / a (mean)"}
    assert out["Info / a (mean)"] == 0.5 and not any(isinstance(v, float) and math.isnan(v) for v in out.values())
    t.call(np.ones(4, dtype=F), np.array([0, 1, 0, 0]), (np.full(4, 0.5, dtype=F),))
    out = T.tags_of(t.raw(("a",)))
    assert set(T.SKRL_TAGS) <= set(out) and out["Episodes / finished"] == 1 and out["Episodes / return (std)"] == 0.0
    # zero envs: calls are counted, nothing is averaged
    z = R.Tracker(0, window=3)
    z.call(np.zeros(0, dtype=F), np.zeros(0, dtype=bool))
    assert z.record["calls"] == 1 and dict(T.tags_of(z.raw())) == {"Episodes / finished": 0}


def test_combine_of_two_halves_equals_the_whole():
    """The restatement on 10 envs against EpisodeTracker.combine of the restatements on envs 0..4 and 5..9: integers and float32
    extrema are equal, the f64 sums agree within the whole's any-order bound (fsum(a) + fsum(b) is one such order, up to the two inner
    roundings, which the bound's n >= 3 covers), the window tags are absent."""
    from isaac_rover_amd.learning import tracking as T
    rng = np.random.default_rng(5)
    names = ("x", "n")
    whole, a, b = R.Tracker(10, 4, 2), R.Tracker(5, 4, 2), R.Tracker(5, 4, 2)
    for _ in range(30):
        r = rng.uniform(-1, 1, 10).astype(F)
        d = rng.random(10) < 0.2
        x, n = rng.uniform(0, 3, 10).astype(F), rng.integers(0, 5, 10).astype(np.int64)
        whole.call(r, d, (x, n))
        a.call(r[:5], d[:5], (x[:5], n[:5]))
        b.call(r[5:], d[5:], (x[5:], n[5:]))
    got = T.EpisodeTracker.combine(T.tags_of(a.raw(names)), T.tags_of(b.raw(names)))
    want = T.tags_of(whole.raw(names))
    _, _, bounds = whole.snapshot()
    assert got.raw["num_envs"] == 10 and got.raw["calls"] == 30 and got.raw["inst_count"] == 300
    for k in ("ep_count", "ep_len_sum", "ep_len_min", "ep_len_max", "inst_min", "inst_max", "ep_ret_min", "ep_ret_max"):
        assert got.raw[k] == want.raw[k], k
    for k in ("inst_sum", "ep_ret_sum", "ep_ret_sumsq"):
        assert abs(got.raw[k] - want.raw[k]) <= bounds[k], k
    for i in range(2):
        assert abs(got.raw["comp_sum"][i] - want.raw["comp_sum"][i]) <= bounds["comp_sum"][i]
    window_tags = {t for t in T.SKRL_TAGS if "Instantaneous" not in t}
    assert set(got) == set(want) - window_tags and window_tags <= set(want)
    for k in got:
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12), k
    with pytest.raises(ValueError):
        T.EpisodeTracker.combine(T.tags_of(a.raw(names)), T.tags_of(R.Tracker(5, 4, 2).raw(names)))
