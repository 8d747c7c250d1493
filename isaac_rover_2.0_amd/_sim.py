"""The entry points of rover_capi_sim.cpp: observation noise, line-of-sight occlusion, the running scalers, the motion model and the
episode statistics."""
import ctypes as C
import math

import numpy as np
import torch

from ._abi import (_FAKE, DRIVES, SUSPENSIONS, TRACK_F32, TRACK_I64, TRACK_MAX_COMPONENTS, TRACK_MAX_WINDOW, BogieParams, DriveParams, EngineBase, MotionDesc,
                   ObsNoiseDesc, ObsOcclusionDesc, OcclusionCfg, RoverError, ScalerApplyDesc, ScalerPlanDesc, ScalerUpdateDesc, TrackDesc,
                   TrackRecord, TrackSizes, _host, _rows, as_dict, host_call)


def obs_noise_desc(m, f, first, in_=_FAKE, out=_FAKE, in_stride=None, out_stride=None, sigma_point=0.0, sigma_offset=0.0, dropout=0.0,
                   drop_value=0.0, row_scale=None, episode=None, seed=0, step=0, step_dev=None, row_offset=0):
    """A rover_obs_noise_desc from plain values (pointers as integers; the strides default to ``f``)."""
    f = int(f)
    return ObsNoiseDesc(in_, f if in_stride is None else int(in_stride), out, f if out_stride is None else int(out_stride), int(m), f, int(first),
                        float(sigma_point), float(sigma_offset), float(dropout), float(drop_value), row_scale, episode, int(seed) & (2 ** 64 - 1),
                        int(step) & (2 ** 64 - 1), step_dev, int(row_offset))


def obs_noise_threshold(dropout):
    """rover_obs_noise_threshold: the integer rover_obs_noise compares a column's 24-bit dropout word with, llrint(dropout 2^24).  Host only."""
    out = C.c_uint32()
    host_call("rover_obs_noise_threshold", float(dropout), C.byref(out))
    return int(out.value)


def occlusion_cfg(camera=(0.0, 0.0, 0.7), step=0.05, clearance=0.03, max_steps=256, miss=5.0):
    """A rover_occlusion_cfg from plain values (the defaults are HeightmapOcclusion's)."""
    cam = tuple(float(v) for v in camera)
    if len(cam) != 3:
        raise RoverError("occlusion_cfg: camera must have three components (forward, left, up)")
    return OcclusionCfg((C.c_float * 3)(*cam), float(step), float(clearance), int(max_steps), float(miss))


def obs_occlusion_desc(m, f, first, pos3=_FAKE, quat4=_FAKE, clean=_FAKE, in_=_FAKE + (1 << 44), out=_FAKE + (2 << 44), clean_stride=None,
                       in_stride=None, out_stride=None, drop_value=0.0, hidden_u8=None, hidden_stride=None, target3=None):
    """A rover_obs_occlusion_desc from plain values (pointers as integers; the strides default to ``f``, hidden's to ``f - first``)."""
    f, first = int(f), int(first)
    return ObsOcclusionDesc(pos3, quat4, clean, f if clean_stride is None else int(clean_stride), in_, f if in_stride is None else int(in_stride),
                            out, f if out_stride is None else int(out_stride), int(m), f, first, float(drop_value), hidden_u8,
                            f - first if hidden_stride is None else int(hidden_stride), target3)


def occlusion_order(points, sparse_idx, dense_idx, camera=(0.0, 0.0, 0.7)):
    """rover_occlusion_order: the heightmap columns far first by the horizontal distance of their body point from ``camera``, ties in
    column order -> int32 numpy array [Ns + Nd], the permutation the occlusion kernel's route 1 walks.  Host only."""
    pts, sp, de = _host(points, np.float64), _host(sparse_idx, np.int64).reshape(-1), _host(dense_idx, np.int64).reshape(-1)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise RoverError("occlusion_order: points must be [P,3]")
    cam = np.ascontiguousarray(camera, dtype=np.float32).reshape(-1)
    if cam.shape != (3,):
        raise RoverError("occlusion_order: camera must have three components")
    out = np.empty(len(sp) + len(de), dtype=np.int32)
    host_call("rover_occlusion_order", pts.ctypes.data, pts.shape[0], sp.ctypes.data if len(sp) else None, len(sp),
              de.ctypes.data if len(de) else None, len(de), cam.ctypes.data, out.ctypes.data)
    return out


def scaler_plan(m, n):
    """rover_scaler_plan: how rover_scaler_update splits ``m`` rows of ``n`` columns, as a dict (route, rows_per_chunk, n_chunks,
    scratch_bytes).  Host only, a pure function of (m, n)."""
    out = ScalerPlanDesc()
    host_call("rover_scaler_plan", int(m), int(n), C.byref(out))
    return as_dict(out)


def scaler_update_desc(m, n, x=1 << 36, x_stride=None, mean=_FAKE, var=_FAKE + (1 << 15), count=_FAKE + (1 << 16), scratch=1 << 20,
                       scratch_bytes=None, skip_if=None):
    """A rover_scaler_update_desc from plain values (pointers as integers; the stride defaults to ``n``, ``scratch_bytes`` to the plan's;
    the default addresses are never read and disjoint for every legal shape)."""
    if scratch_bytes is None:
        scratch_bytes = scaler_plan(m, n)["scratch_bytes"]
    return ScalerUpdateDesc(x, int(n) if x_stride is None else int(x_stride), int(m), int(n), mean, var, count, scratch, int(scratch_bytes), skip_if)


def scaler_apply_desc(m, n, x=1 << 36, y=1 << 36, x_stride=None, y_stride=None, mean=_FAKE, var=_FAKE + (1 << 15), epsilon=1e-8, clip=5.0, inverse=False):
    """A rover_scaler_apply_desc from plain values (pointers as integers; the strides default to ``n``)."""
    return ScalerApplyDesc(x, int(n) if x_stride is None else int(x_stride), y, int(n) if y_stride is None else int(y_stride), int(m), int(n),
                           mean, var, float(epsilon), float(clip), int(bool(inverse)))


def motion_desc(e, pos3=_FAKE, quat4=_FAKE, lin=_FAKE, ang=_FAKE, cmd_stride=3, substeps=1, dt=0.05, max_lin=1.0, max_ang=1.0, ride_height=0.3,
                joint_pos_targets13=None, joint_vel_targets13=None, joint_pos13=None, joint_vel13=None):
    """A rover_motion_desc from plain values (pointers as integers)."""
    return MotionDesc(pos3, quat4, lin, ang, int(cmd_stride), int(e), int(substeps), float(dt), float(max_lin), float(max_ang), float(ride_height),
                      joint_pos_targets13, joint_vel_targets13, joint_pos13, joint_vel13)


def motion_plane_fit():
    """rover_motion_plane_fit: the constant C [3, 6] of the motion model's plane fit, (z_c, p, q) = C z over the six wheel contacts
    (FL, FR, ML, MR, RL, RR) -> a float32 array.  Host only."""
    out = np.empty((3, 6), dtype=np.float32)
    host_call("rover_motion_plane_fit", out.ctypes.data)
    return out


def motion_bogie_fit():
    """rover_motion_bogie_fit: the constant D [6, 6] of the rocker-bogie posture solve, the inverse of the Jacobian at rest of the six
    wheel-origin heights by (z_c, roll, pitch, j0, j1, j2) -> a float32 array.  Host only."""
    out = np.empty((6, 6), dtype=np.float32)
    host_call("rover_motion_bogie_fit", out.ctypes.data)
    return out


def motion_drive_fit():
    """rover_motion_drive_fit: the constant P [3, 12] of the wheel-level drive mode, (vx, vy, w) = P t over the six wheels' velocity
    vectors (FL, FR, ML, MR, RL, RR; column 2i is wheel i's body-x component, 2i + 1 its body-y) -> a float32 array.  Host only."""
    out = np.empty((3, 12), dtype=np.float32)
    host_call("rover_motion_drive_fit", out.ctypes.data)
    return out


def track_sizes(e, w=100, k=0):
    """rover_track_sizes: what rover_episode_track needs for ``e`` envs as a dict (workgroup, n_partials, partial_bytes, finished_slots,
    scratch_bytes).  Host only."""
    out = TrackSizes()
    host_call("rover_track_sizes", int(e), int(w), int(k), C.byref(out))
    return as_dict(out)


def track_desc(e, w=100, comps=(), rewards=_FAKE, done=_FAKE, done_size=1, cum_reward=_FAKE, cum_steps=_FAKE, ring_ret=_FAKE, ring_len=_FAKE,
               ring_count=_FAKE, record=_FAKE, scratch=_FAKE, scratch_bytes=None, k=None):
    """A rover_track_desc from plain values (pointers as integers).  ``comps``: (pointer, kind) pairs; ``k`` overrides their number;
    ``scratch_bytes`` defaults to what rover_track_sizes reports for ``e``."""
    d = TrackDesc()
    d.rewards, d.done, d.done_size, d.E, d.W = rewards, done, int(done_size), int(e), int(w)
    d.K = len(comps) if k is None else int(k)
    for i, (ptr, kind) in enumerate(comps):
        d.comp[i], d.comp_kind[i] = ptr, int(kind)
    d.cum_reward, d.cum_steps, d.ring_ret, d.ring_len, d.ring_count, d.record, d.scratch = cum_reward, cum_steps, ring_ret, ring_len, ring_count, record, scratch
    if scratch_bytes is None:
        scratch_bytes = track_sizes(e, 1, 0)["scratch_bytes"] if e >= 0 else 0
    d.scratch_bytes = int(scratch_bytes)
    return d


def track_fresh_record():
    """The interval record before its first call: zeros, minima at +inf / INT32_MAX, maxima at -inf / INT32_MIN."""
    r = TrackRecord()
    r.inst_min = r.ep_ret_min = r.win_ret_min = float("inf")
    r.inst_max = r.ep_ret_max = r.win_ret_max = float("-inf")
    r.ep_len_min = r.win_len_min = 2 ** 31 - 1
    r.ep_len_max = r.win_len_max = -2 ** 31
    return r


class SimEngine(EngineBase):
    def obs_noise(self, obs, out=None, *, first, sigma_point=0.0, sigma_offset=0.0, dropout=0.0, drop_value=0.0, row_scale=None, episode=None,
                  seed=0, step=0, step_dev=None, row_offset=0):
        """The exteroception noise on ``obs`` [m, f] (rover_obs_noise, one launch): columns [0, first) copied, every later column
        ``(obs + (sigma_offset s) eo) + (sigma_point s) eps``, or ``drop_value`` with probability ``dropout``; counter-based, keyed by
        (seed, step + *step_dev, row_offset + row, column) and, for the offset draw eo, by ``episode`` [m] int64.  ``row_scale`` [m]
        float32 is s (default 1).  ``out`` None: a new tensor; ``out is obs`` (or a view of the same memory): in place.  Strides come from
        the tensors: ``out = x[:, t]`` of a [B, T, F] window works."""
        what = "obs_noise"
        self._f32_rows(obs, "obs", what)
        m, f = obs.shape
        if out is None:
            out = torch.empty(m, f, device=obs.device)
        self._f32_rows(out, "out", what, (m, f))
        if obs.device != self.device or out.device != self.device:
            raise RoverError(f"{what}: obs and out must be on {self.device}")
        if row_scale is not None:
            self._chk(row_scale, (m,), torch.float32, "row_scale")
        if episode is not None:
            self._chk(episode, (m,), torch.int64, "episode")
        if step_dev is not None and (not step_dev.is_cuda or step_dev.dtype != torch.int64 or step_dev.numel() != 1):
            raise RoverError(f"{what}: step_dev must be one int64 word on the GPU (read as uint64)")
        dp = lambda t: None if t is None else t.data_ptr()
        (ip, is_), (op, os_) = _rows(obs, f, m), _rows(out, f, m)
        desc = obs_noise_desc(m, f, first, ip, op, is_, os_, sigma_point, sigma_offset, dropout, drop_value, dp(row_scale), dp(episode), seed, step,
                              dp(step_dev), row_offset)
        self._call("rover_obs_noise", C.byref(desc))
        return out

    def configure_occlusion(self, camera=(0.0, 0.0, 0.7), step=0.05, clearance=0.03, max_steps=256, miss=5.0):
        """The line-of-sight stage's configuration (rover_set_occlusion): needs set_distribution and set_heightfield, derives the column
        order and the tile-max table of the heightfield, and has to be called again after either of the two is set again."""
        self._call("rover_set_occlusion", C.byref(occlusion_cfg(camera, step, clearance, max_steps, miss)))

    def obs_occlusion(self, clean, in_=None, out=None, *, first, pos, quat, drop_value=0.0, hidden=None, target=None):
        """Which heightmap columns of ``clean`` [m, f] a mast camera at the poses ``pos`` [m, 3] / ``quat`` [m, 4] (w, x, y, z) cannot see
        (rover_obs_occlusion, one launch): out = ``drop_value`` where hidden, ``in_`` elsewhere (``in_`` None: ``clean``; it may be the
        output of obs_noise on ``clean``); columns [0, first) copied.  ``out`` None: a new tensor; ``out is in_`` (or a view of the same
        memory): in place — but never ``clean`` itself.  ``hidden``: optional uint8 [m, f - first], 1 = hidden.  ``target``: optional
        float32 [m, f - first, 3], the measured points (unwritten where ``|clean| >= miss``).  Strides come from the tensors."""
        what = "obs_occlusion"
        self._f32_rows(clean, "clean", what)
        m, f = clean.shape
        if in_ is None:
            in_ = clean
        self._f32_rows(in_, "in_", what, (m, f))
        if out is None:
            out = torch.empty(m, f, device=clean.device)
        self._f32_rows(out, "out", what, (m, f))
        if clean.device != self.device or in_.device != self.device or out.device != self.device:
            raise RoverError(f"{what}: clean, in_ and out must be on {self.device}")
        self._chk(pos, (m, 3), torch.float32, "pos")
        self._chk(quat, (m, 4), torch.float32, "quat")
        if pos is None or quat is None:
            raise RoverError(f"{what}: pos [m, 3] and quat [m, 4] must be given")
        c = f - int(first)
        if hidden is not None and (not hidden.is_cuda or hidden.device != self.device or hidden.dtype != torch.uint8 or hidden.dim() != 2
                                   or tuple(hidden.shape) != (m, c) or (c > 0 and hidden.stride(1) != 1)):
            raise RoverError(f"{what}: hidden must be a uint8 GPU matrix [{m},{c}] with unit column stride")
        self._chk(target, (m, c, 3), torch.float32, "target")
        (cp, cs), (ip, is_), (op, os_), (hp, hs) = _rows(clean, f, m), _rows(in_, f, m), _rows(out, f, m), _rows(hidden, c, m)
        desc = obs_occlusion_desc(m, f, first, pos.data_ptr(), quat.data_ptr(), cp, ip, op, cs, is_, os_, drop_value, hp, hs,
                                  None if target is None else target.data_ptr())
        self._call("rover_obs_occlusion", C.byref(desc))
        return out

    scaler_plan = staticmethod(scaler_plan)

    def _scaler_state(self, what, n, mean, var, count=None):
        self._chk(mean, (n,), torch.float64, "mean")
        self._chk(var, (n,), torch.float64, "var")
        self._chk(count, (1,), torch.float64, "count")
        if mean is None or var is None:
            raise RoverError(f"{what}: mean and var must be given")

    def scaler_update(self, x, mean, var, count, scratch, skip_if=None):
        """A train call of skrl's RunningStandardScaler on ``x`` [m, n] (rover_scaler_update, two launches, no host read, capturable):
        the batch's column means and unbiased variances are folded into ``mean`` / ``var`` [n] and ``count`` [1], float64 on the device.
        ``scratch``: uint8, at least ``scaler_plan(m, n)["scratch_bytes"]``.  ``skip_if``: one int32 on the device; nonzero when the
        kernels run leaves the state bit-unchanged."""
        what = "scaler_update"
        self._f32_rows(x, "x", what)
        m, n = x.shape
        self._scaler_state(what, n, mean, var, count)
        if count is None or scratch is None or not scratch.is_cuda or scratch.dtype != torch.uint8 or scratch.dim() != 1:
            raise RoverError(f"{what}: count and a uint8 scratch vector on the GPU must be given")
        if skip_if is not None and (not skip_if.is_cuda or skip_if.dtype != torch.int32 or skip_if.numel() != 1):
            raise RoverError(f"{what}: skip_if must be one int32 word on the GPU")
        desc = ScalerUpdateDesc(*_rows(x, n, m), m, n, mean.data_ptr(), var.data_ptr(), count.data_ptr(), scratch.data_ptr(),
                                scratch.numel(), None if skip_if is None else skip_if.data_ptr())
        self._call("rover_scaler_update", C.byref(desc))

    def scaler_apply(self, x, mean, var, out=None, *, epsilon=1e-8, clip=5.0, inverse=False):
        """``clamp((x - mean) / (sqrt(var) + epsilon), -clip, clip)``, or with ``inverse`` ``sqrt(var) * clamp(x, -clip, clip) + mean``, on
        ``x`` [m, n] in f32 (rover_scaler_apply, one launch); the float64 statistics are read on the device when the kernel runs.
        ``out`` None: a new tensor; ``out is x`` (or a view of the same memory): in place."""
        what = "scaler_apply"
        self._f32_rows(x, "x", what)
        m, n = x.shape
        if out is None:
            out = torch.empty(m, n, device=x.device)
        self._f32_rows(out, "out", what, (m, n))
        if x.device != self.device or out.device != self.device:
            raise RoverError(f"{what}: x and out must be on {self.device}")
        self._scaler_state(what, n, mean, var)
        (xp, xs), (yp, ys) = _rows(x, n, m), _rows(out, n, m)
        desc = scaler_apply_desc(m, n, xp, yp, xs, ys, mean.data_ptr(), var.data_ptr(), epsilon, clip, inverse)
        self._call("rover_scaler_apply", C.byref(desc))
        return out

    def motion_step(self, pos, quat, lin, ang, *, dt, substeps=1, max_lin=1.0, max_ang=1.0, ride_height=0.3, joints=None,
                    suspension="plane", iters=4, max_bogie=0.6, drive="command", wheel_radius=0.2, steer_rate=math.inf, wheel_accel=math.inf,
                    slip=None):
        """``substeps`` sub-steps of length ``dt`` of the terrain-following motion model on ``pos`` [e, 3] and ``quat`` [e, 4] (w, x, y, z),
        IN PLACE (rover_motion_step, one launch; needs set_heightfield): the commands ``lin`` / ``ang`` [e] scaled by ``max_lin`` /
        ``max_ang`` move the body, the six wheel contacts' terrain heights give z, roll and pitch.  ``lin`` and ``ang`` may be one column
        of a wider matrix (``tracker[:, 0]``): their common stride is passed on.  ``joints``: None, or (joint_pos_targets, joint_vel_targets,
        joint_pos, joint_vel), each [e, 13] — after the last sub-step the state becomes the targets.
        ``suspension="bogie"`` (rover_motion_step_bogie) solves the rocker-bogie posture instead of fitting a plane: ``iters`` chord
        iterations put all six wheels on the ground, and the three passive joint angles, clamped to +-``max_bogie`` rad, go to columns
        0-2 of joint_pos.  ``iters`` and ``max_bogie`` are not read with ``suspension="plane"``.
        ``drive="wheels"`` (rover_motion_step_drive; either suspension) moves the body by its wheels instead of by the command: the
        steering angles and wheel speeds of joint_pos / joint_vel follow their targets by at most ``steer_rate`` rad/s and ``wheel_accel``
        rad/s^2 (``inf``, the default: at once), and the body takes the rigid motion that fits the six wheel velocity vectors, rolling on
        ``wheel_radius`` m, best.  ``joints`` must be given; ``lin``, ``ang``, ``max_lin`` and ``max_ang`` are not read and ``lin`` / ``ang``
        may be None.  ``slip``: None, or a float32 vector [e] that receives the last sub-step's wheel slip in m/s.  ``wheel_radius`` = 0.2
        is the length the reference's Ackermann divides by, so a forward command covers the distance it covers with ``drive="command"``;
        0.1 is the asset's physical radius and halves every speed, as the reference's rover in PhysX does.  ``drive="command"``, the
        default, is the behaviour without these arguments, which it does not read."""
        what = "motion_step"
        if suspension not in SUSPENSIONS:
            raise RoverError(f"{what}: suspension must be one of {SUSPENSIONS}, not {suspension!r}")
        if drive not in DRIVES:
            raise RoverError(f"{what}: drive must be one of {DRIVES}, not {drive!r}")
        wheels = drive == "wheels"
        e = pos.shape[0] if pos is not None and pos.dim() == 2 else -1
        self._chk(pos, (e, 3), torch.float32, "pos")
        self._chk(quat, (e, 4), torch.float32, "quat")
        if pos is None or quat is None or e < 0:
            raise RoverError(f"{what}: pos [e, 3] and quat [e, 4] must be given")
        stride = 1
        if not wheels:
            for t, name in ((lin, "lin"), (ang, "ang")):
                if t is None or not t.is_cuda or t.device != self.device or t.dtype != torch.float32 or tuple(t.shape) != (e,):
                    raise RoverError(f"{what}: {name} must be a float32 vector [{e}] on {self.device}")
            stride = 1 if e <= 1 else lin.stride(0)
            if e > 1 and (stride < 1 or ang.stride(0) != stride):
                raise RoverError(f"{what}: lin and ang must have the same positive stride (got {lin.stride(0)} and {ang.stride(0)})")
        jp = [None] * 4
        if joints is not None:
            if len(joints) != 4:
                raise RoverError(f"{what}: joints = (joint_pos_targets, joint_vel_targets, joint_pos, joint_vel)")
            for t, name in zip(joints, ("joint_pos_targets", "joint_vel_targets", "joint_pos", "joint_vel")):
                if t is None:
                    raise RoverError(f"{what}: {name} is missing")
                self._chk(t, (e, 13), torch.float32, name)
            jp = [t.data_ptr() for t in joints]
        bogie = BogieParams(int(iters), float(max_bogie)) if suspension == "bogie" else None
        if wheels:
            if joints is None:
                raise RoverError(f"{what}: drive='wheels' needs joints: the joint state is what it drives")
            if slip is not None:
                self._chk(slip, (e,), torch.float32, "slip")
            desc = motion_desc(e, pos.data_ptr(), quat.data_ptr(), None, None, 0, substeps, dt, 0.0, 0.0, ride_height, *jp)
            params = DriveParams(float(wheel_radius), float(steer_rate), float(wheel_accel), None if slip is None else slip.data_ptr())
            self._call("rover_motion_step_drive", C.byref(desc), C.byref(params), None if bogie is None else C.byref(bogie))
            return
        desc = motion_desc(e, pos.data_ptr(), quat.data_ptr(), lin.data_ptr(), ang.data_ptr(), stride, substeps, dt, max_lin, max_ang, ride_height, *jp)
        if suspension == "bogie":
            self._call("rover_motion_step_bogie", C.byref(desc), C.byref(BogieParams(int(iters), float(max_bogie))))
        else:
            self._call("rover_motion_step", C.byref(desc))

    def episode_track(self, rewards, done, *, cum_reward, cum_steps, ring_ret, ring_len, ring_count, record, scratch, components=(), desc=None):
        """One env step of the episode statistics (rover_episode_track: two launches, no host read, capturable): ``rewards`` [e] float32
        and ``done`` [e] (bool, uint8 or int64) are folded into the per-env state ``cum_reward`` [e] float32 / ``cum_steps`` [e] int32, the
        window ``ring_ret`` [w] float32 / ``ring_len`` [w] int32 / ``ring_count`` [1] int64 and the interval ``record`` (uint8
        [sizeof(TrackRecord)], a _lib.track_fresh_record() before its first call); ``components``: up to 16 float32 or int64 vectors [e]
        whose sums the record keeps; ``scratch``: uint8, at least track_sizes(e)["scratch_bytes"].  Returns the descriptor; passed back as
        ``desc`` with the same tensors it skips the checks (the tensors must then be the ones it was built from)."""
        what = "episode_track"
        if desc is None:
            if rewards is None or rewards.dim() != 1:
                raise RoverError(f"{what}: rewards must be a float32 vector")
            e, w = rewards.shape[0], (ring_ret.shape[0] if ring_ret is not None and ring_ret.dim() == 1 else -1)
            self._chk(rewards, (e,), torch.float32, "rewards")
            if done is None or done.dtype not in (torch.bool, torch.uint8, torch.int64):
                raise RoverError(f"{what}: done must be a bool, uint8 or int64 vector [{e}]")
            self._chk(done, (e,), done.dtype, "done")
            if not 1 <= w <= TRACK_MAX_WINDOW:
                raise RoverError(f"{what}: ring_ret must be a float32 vector of 1 .. {TRACK_MAX_WINDOW} slots")
            if len(components) > TRACK_MAX_COMPONENTS:
                raise RoverError(f"{what}: {len(components)} components, at most {TRACK_MAX_COMPONENTS}")
            for t, shape, dtype, name in ((cum_reward, (e,), torch.float32, "cum_reward"), (cum_steps, (e,), torch.int32, "cum_steps"),
                                          (ring_ret, (w,), torch.float32, "ring_ret"), (ring_len, (w,), torch.int32, "ring_len"),
                                          (ring_count, (1,), torch.int64, "ring_count"), (record, (C.sizeof(TrackRecord),), torch.uint8, "record")):
                if t is None:
                    raise RoverError(f"{what}: {name} is missing")
                self._chk(t, shape, dtype, name)
            comps = []
            for i, t in enumerate(components):
                if t is None or t.dtype not in (torch.float32, torch.int64):
                    raise RoverError(f"{what}: component {i} must be a float32 or int64 vector [{e}]")
                self._chk(t, (e,), t.dtype, f"component {i}")
                comps.append((t.data_ptr(), TRACK_I64 if t.dtype == torch.int64 else TRACK_F32))
            need = track_sizes(e, w, len(comps))["scratch_bytes"]
            if scratch is None or scratch.dim() != 1 or scratch.numel() < need:
                raise RoverError(f"{what}: scratch must be a uint8 vector of at least {need} bytes")
            self._chk(scratch, (scratch.numel(),), torch.uint8, "scratch")
            desc = track_desc(e, w, comps, rewards.data_ptr(), done.data_ptr(), done.element_size(), cum_reward.data_ptr(), cum_steps.data_ptr(),
                              ring_ret.data_ptr(), ring_len.data_ptr(), ring_count.data_ptr(), record.data_ptr(), scratch.data_ptr(), scratch.numel())
        self._call("rover_episode_track", C.byref(desc))
        return desc
