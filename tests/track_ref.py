"""The episode statistics as DEFINED (include/rover_step.h, rover_episode_track), restated in numpy: float32 with one rounding per
operation for cum_reward, Python ints for every count, and ``math.fsum`` — the correctly rounded sum — over the exact addends (float32
values, integers, the exact float64 squares of float32 values) for every f64 sum.  What the device may differ by is an f64 sum's order:
``bounds`` holds, per f64 field, the bound n * 2^-53 * sum|x| of ANY summation order of its n addends (Higham, Accuracy and Stability,
eq. 4.4: |error| <= gamma_(n-1) sum|x|, and gamma_(n-1) <= n u while n u < 1).  For the two window means the addends are themselves
quotients: a call's mean return is fl(S' / m) on the device, with S' any-order sum of the m valid slots, against fl(fsum / m) here;
|S' - S| <= m u sum|x| gives |S'/m - S/m| <= u sum|x|, and the two divisions round by at most u |mean| each, so the call adds
u (sum|x| + 2 |mean|) to the bound; the lengths' sum is an exact integer on both sides, so their means are the same float64."""
import math

import numpy as np

U = 2.0 ** -53
MAX_COMPONENTS, MAX_WINDOW, WORKGROUP = 16, 1024, 256
F64_FIELDS = ("inst_sum", "ep_ret_sum", "ep_ret_sumsq", "win_ret_mean_sum", "win_len_mean_sum")
INT_FIELDS = ("calls", "ep_count", "ep_len_sum", "win_calls", "ep_len_min", "ep_len_max", "win_len_min", "win_len_max")
F32_FIELDS = ("inst_min", "inst_max", "ep_ret_min", "ep_ret_max", "win_ret_min", "win_ret_max")
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def fresh_record():
    r = {k: 0 for k in ("calls", "ep_count", "ep_len_sum", "win_calls")}
    r.update({k: 0.0 for k in F64_FIELDS})
    r["comp_sum"] = [0.0] * MAX_COMPONENTS
    for k in ("inst", "ep_ret", "win_ret"):
        r[k + "_min"], r[k + "_max"] = np.float32(np.inf), np.float32(-np.inf)
    for k in ("ep_len", "win_len"):
        r[k + "_min"], r[k + "_max"] = I32_MAX, I32_MIN
    return r


def omin(values, start):
    """The float32 minimum of ``start`` and ``values`` with -0 below +0."""
    v = np.concatenate((np.asarray(values, dtype=np.float32).ravel(), np.array([start], dtype=np.float32)))
    m = v.min()
    if m == 0 and np.any((v == 0) & np.signbit(v)):
        m = np.float32(-0.0)
    return np.float32(m)


def omax(values, start):
    v = np.concatenate((np.asarray(values, dtype=np.float32).ravel(), np.array([start], dtype=np.float32)))
    m = v.max()
    if m == 0 and np.any((v == 0) & ~np.signbit(v)):
        m = np.float32(0.0)
    return np.float32(m)


def n_partials(e):
    """The update kernel's workgroups for ``e`` envs: the documented workgroup size is 256."""
    return (e + WORKGROUP - 1) // WORKGROUP


class _Sum:
    """The exact addends of one f64 field: its value is their fsum; its bound n u sum|x| plus what the addends themselves may differ by."""

    def __init__(self):
        self.addends, self.magnitudes, self.slack = [], [], 0.0

    def add(self, values, slack=0.0):
        v = np.asarray(values, dtype=np.float64)
        self.addends.extend(v.tolist())
        self.magnitudes.extend(np.abs(v).tolist())
        self.slack += slack

    @property
    def value(self):
        return math.fsum(self.addends)

    @property
    def bound(self):
        return len(self.addends) * U * math.fsum(self.magnitudes) + self.slack


class Tracker:
    def __init__(self, num_envs, window=100, n_components=0):
        assert num_envs >= 0 and 1 <= window <= MAX_WINDOW and 0 <= n_components <= MAX_COMPONENTS
        self.E, self.W, self.K = num_envs, window, n_components
        self.cum_reward = np.zeros(num_envs, dtype=np.float32)
        self.cum_steps = np.zeros(num_envs, dtype=np.int64)
        self.ring_ret = np.zeros(window, dtype=np.float32)
        self.ring_len = np.zeros(window, dtype=np.int64)
        self.ring_count = 0
        self.reset_record()

    def reset_record(self):
        self.record = fresh_record()
        self._sums = {k: _Sum() for k in F64_FIELDS}
        self._comp = [_Sum() for _ in range(self.K)]

    @property
    def valid(self):
        return min(self.ring_count, self.W)

    def call(self, rewards, done, comps=()):
        """One env step -> (state, record, bounds) as ``snapshot`` returns them."""
        rewards = np.asarray(rewards, dtype=np.float32)
        done = np.asarray(done) != 0
        assert rewards.shape == (self.E,) and done.shape == (self.E,) and len(comps) == self.K
        r = self.record
        # 1. per env
        c = self.cum_reward + rewards                                    # float32 + float32: one rounding
        assert c.dtype == np.float32
        n = self.cum_steps + 1
        fin_ret, fin_len = c[done], n[done]                              # ascending env order
        self.cum_reward = np.where(done, np.float32(0), c).astype(np.float32)
        self.cum_steps = np.where(done, 0, n)
        # 2. ring
        for j in range(max(0, len(fin_ret) - self.W), len(fin_ret)):
            slot = (self.ring_count + j) % self.W
            self.ring_ret[slot], self.ring_len[slot] = fin_ret[j], fin_len[j]
        self.ring_count += len(fin_ret)
        # 3. record
        r["calls"] += 1
        if self.E:
            r["inst_min"], r["inst_max"] = omin(rewards, r["inst_min"]), omax(rewards, r["inst_max"])
            self._sums["inst_sum"].add(rewards.astype(np.float64))
        if len(fin_ret):
            f64 = fin_ret.astype(np.float64)
            r["ep_count"] += len(fin_ret)
            self._sums["ep_ret_sum"].add(f64)
            self._sums["ep_ret_sumsq"].add(f64 * f64)                   # exact: 48 significant bits
            r["ep_ret_min"], r["ep_ret_max"] = omin(fin_ret, r["ep_ret_min"]), omax(fin_ret, r["ep_ret_max"])
            r["ep_len_sum"] += int(fin_len.sum())
            r["ep_len_min"], r["ep_len_max"] = min(r["ep_len_min"], int(fin_len.min())), max(r["ep_len_max"], int(fin_len.max()))
        for k, col in enumerate(comps):
            col = np.asarray(col)
            assert col.shape == (self.E,) and col.dtype in (np.float32, np.int64)
            self._comp[k].add(col.astype(np.float64))
        m = self.valid
        if m > 0:
            ret, ln = self.ring_ret[:m], self.ring_len[:m]
            r["win_calls"] += 1
            mean = math.fsum(ret.astype(np.float64)) / m
            self._sums["win_ret_mean_sum"].add([mean], slack=U * (math.fsum(np.abs(ret.astype(np.float64))) + 2.0 * abs(mean)))
            self._sums["win_len_mean_sum"].add([int(ln.sum()) / m])
            r["win_ret_min"], r["win_ret_max"] = omin(ret, r["win_ret_min"]), omax(ret, r["win_ret_max"])
            r["win_len_min"], r["win_len_max"] = min(r["win_len_min"], int(ln.min())), max(r["win_len_max"], int(ln.max()))
        return self.snapshot()

    def snapshot(self):
        rec = dict(self.record)
        bounds = {}
        for k, s in self._sums.items():
            rec[k], bounds[k] = s.value, s.bound
        rec["comp_sum"] = [s.value for s in self._comp] + [0.0] * (MAX_COMPONENTS - self.K)
        bounds["comp_sum"] = [s.bound for s in self._comp]
        state = {"cum_reward": self.cum_reward.copy(), "cum_steps": self.cum_steps.copy(), "ring_ret": self.ring_ret[:self.valid].copy(),
                 "ring_len": self.ring_len[:self.valid].copy(), "ring_count": self.ring_count}
        return state, rec, bounds

    def raw(self, components=()):
        """The record in the form learning/tracking.py:tags_of takes."""
        _, rec, _ = self.snapshot()
        raw = {k: (float(v) if isinstance(v, np.floating) else v) for k, v in rec.items()}
        raw["comp_sum"] = rec["comp_sum"][:self.K]
        raw["components"], raw["num_envs"], raw["inst_count"] = tuple(components), self.E, rec["calls"] * self.E
        return raw
