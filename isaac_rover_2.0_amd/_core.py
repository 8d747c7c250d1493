"""The entry points of rover_capi.cpp: the ctx lifecycle, the tables, the step, the rays, the reset path, evaluation, options and profiling."""
import ctypes as C

import numpy as np
import torch

from ._abi import (EXTRAS, MAP_ROCKS, MAP_TERRAIN, STEP_COMPACT, STEP_INCREMENT_PROGRESS, Cfg, CullInfo, EngineBase, Info, PlanQuery, Profile,
                   RaycastPlan, ResetIO, RoverError, StepIn, StepOut, _host, _ptr, _stream, as_dict, host_call, load)


def plan_raycast(num_envs, maps, P=0, have_dist=None, ray_precision=0, raycast_variant=0, raycast_run=0, lane_env_order=-1, lane_rocks=-1,
                 bin_low_bits=0, cull_lazy=-1, cull_queue_mb=1536):
    """rover_plan_raycast: the plan a ctx with these inputs reports (Engine.raycast_plan()), from shapes and options alone — no ctx, no
    device, no environment variable.  ``maps``: (terrain, rocks), each None (not set) or a dict X, Y, K8, cells_with_far_bound,
    has_cull_tables, has_staged_tables = (f32 proof, fp16 proof).  ``have_dist`` defaults to P > 0."""
    q = PlanQuery(num_envs=int(num_envs), P=int(P), have_dist=int(P > 0 if have_dist is None else have_dist), ray_precision=int(ray_precision),
                  raycast_variant=int(raycast_variant), raycast_run=int(raycast_run), lane_env_order=int(lane_env_order), lane_rocks=int(lane_rocks),
                  bin_low_bits=int(bin_low_bits), cull_lazy=int(cull_lazy), cull_queue_mb=int(cull_queue_mb))
    for w, m in enumerate(maps):
        if m is None:
            continue
        q.map_present[w], q.X[w], q.Y[w], q.K8[w] = 1, int(m["X"]), int(m["Y"]), int(m["K8"])
        q.cells_with_far_bound[w], q.has_cull_tables[w] = int(m["cells_with_far_bound"]), int(m["has_cull_tables"])
        for k in range(2):
            q.has_staged_tables[w][k] = int(m["has_staged_tables"][k])
    out = RaycastPlan()
    host_call("rover_plan_raycast", C.byref(q), C.byref(out))
    return as_dict(out)


class CoreEngine(EngineBase):
    def __init__(self, num_envs, device=0, num_envs_global=0, env_offset=0, curriculum_level=2,
                 max_episode_length=3000, rewards=None):
        self.lib = load()
        rw = dict(pos_reward=1.0, heading_contraint_reward=0.05, motion_contraint_reward=-0.01,
                  goal_angle_reward=0.3, boogie_contraint_reward=0.5)
        rw.update({k: v for k, v in (rewards or {}).items() if k in rw})
        if isinstance(device, torch.device):
            device = device.index or 0
        self.num_envs = int(num_envs)
        self.device = torch.device("cuda", int(device))
        self._dev_index = int(device)
        self.cfg = Cfg(self.num_envs, int(num_envs_global), int(env_offset), int(device), int(curriculum_level),
                       int(max_episode_length), rw["pos_reward"], rw["heading_contraint_reward"],
                       rw["motion_contraint_reward"], rw["goal_angle_reward"], rw["boogie_contraint_reward"])
        h = C.c_void_p()
        host_call("rover_create", C.byref(self.cfg), C.byref(h))
        self._h = h
        self.P = self.Ns = self.Nd = 0
        self.generation = 0         # bumped by every method that changes what a launch bakes in: cached launch state is keyed on it

    def close(self):
        if getattr(self, "_h", None):
            self.lib.rover_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- tables -------------------------------------------------------------------------------
    def set_knn_map(self, which, map_indices, triangles, vertices, cell_size=0.1, shift=(0.0, 0.0)):
        self.generation += 1
        idx = _host(map_indices, np.int32)
        tris = _host(triangles, np.int32)
        v = vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices)
        verts = np.ascontiguousarray(v.astype(np.float16)).view(np.uint16)
        if idx.ndim != 3 or tris.ndim != 2 or tris.shape[1] != 3 or verts.ndim != 2 or verts.shape[1] != 3:
            raise RoverError("set_knn_map: expected map_indices [X,Y,K], triangles [T,3], vertices [V,3]")
        x, y, k = idx.shape
        self._call("rover_set_knn_map", which, idx.ctypes.data, x, y, k, tris.ctypes.data, tris.shape[0], verts.ctypes.data, verts.shape[0],
                   cell_size, float(shift[0]), float(shift[1]))

    def set_distribution(self, points, sparse_idx, dense_idx):
        self.generation += 1
        pts = _host(points, np.float64)
        sp = _host(sparse_idx, np.int64)
        de = _host(dense_idx, np.int64)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise RoverError("set_distribution: points must be [P,3]")
        self._call("rover_set_distribution", pts.ctypes.data, pts.shape[0], sp.ctypes.data, len(sp), de.ctypes.data, len(de))
        self.P, self.Ns, self.Nd = pts.shape[0], len(sp), len(de)

    def set_heightfield(self, heightmap, horizontal_scale=0.025, vertical_scale=1.0, shift=(0.0, 0.0)):
        self.generation += 1
        hm = _host(heightmap, np.float32)
        self._call("rover_set_heightfield", hm.ctypes.data, hm.shape[0], hm.shape[1], horizontal_scale, vertical_scale, float(shift[0]), float(shift[1]))

    def set_stones(self, info7):
        self.generation += 1
        info = _host(info7, np.float32)
        if info.ndim != 2 or info.shape[1] != 7:
            raise RoverError("set_stones: expected [S,7] (read_stone_info output)")
        self._call("rover_set_stones", info.ctypes.data, info.shape[0])

    def set_curriculum_level(self, level):
        self.generation += 1
        self._call("rover_set_curriculum_level", int(level))

    def set_scene(self, scene, distribution):
        """Convenience: load a synth.Scene + (points, sparse_idx, dense_idx)."""
        from . import synth
        sh = scene.shift[0:2]
        self.set_knn_map(MAP_TERRAIN, scene.terrain.map_indices, scene.terrain.triangles, scene.terrain.vertices,
                         scene.terrain.cell_size, sh)
        self.set_knn_map(MAP_ROCKS, scene.rocks.map_indices, scene.rocks.triangles, scene.rocks.vertices,
                         scene.rocks.cell_size, sh)
        self.set_distribution(*distribution)
        self.set_heightfield(scene.heightmap, scene.horizontal_scale, scene.vertical_scale, sh)
        self.set_stones(synth.read_stone_info_array(scene.stone_info_raw))

    @property
    def num_observations(self):
        return 4 + self.Ns + self.Nd

    def info(self):
        i = Info()
        self._call("rover_get_info", C.byref(i))
        return i

    def raycast_plan(self):
        """The ray-cast plan in force and the other host-side values that select a step's code path (rover_get_raycast_plan) as a
        plain dict of ints; host only, no launch, no synchronisation."""
        p = RaycastPlan()
        self._call("rover_get_raycast_plan", C.byref(p))
        return as_dict(p)

    def cull_info(self):
        """Diagnostics of the culled ray cast (rover_get_cull_info) as a dict; synchronises the device."""
        i = CullInfo()
        self._call("rover_get_cull_info", C.byref(i))
        d = {k: (list(getattr(i, k)) if k in ("triangles", "always_candidate_triangles", "cells_without_cone", "cells_with_far_bound") else int(getattr(i, k)))
             for k, _ in CullInfo._fields_}
        d["pairs_per_ray"] = d["candidate_pairs"] / d["rays"] if d["rays"] else 0.0
        return d

    # ---- step ---------------------------------------------------------------------------------
    def make_in(self, pos, quat, joints, target, lin_hist, ang_hist, euler_pre, progress):
        e, f = self.num_envs, torch.float32
        for t, s, n in ((pos, (e, 3), "pos"), (quat, (e, 4), "quat"), (joints, (e, 13), "joints"),
                        (target, (e, 3), "target"), (lin_hist, (e, 3), "lin_hist"), (ang_hist, (e, 3), "ang_hist"),
                        (euler_pre, (e, 3), "euler_pre")):
            self._chk(t, s, f, n)
        self._chk(progress, (e,), torch.int64, "progress")
        tensors = (pos, quat, joints, target, lin_hist, ang_hist, euler_pre, progress)
        sin = StepIn(*[_ptr(t) for t in tensors])
        sin._keep = tensors          # the struct holds raw device pointers: keep the tensors alive as long as it lives
        return sin

    def make_out(self, obs, rew=None, reset=None, rock_collision=None, extras=None, reset_ids=None, n_reset=None,
                 euler=None, heading_diff=None, ray_dist=None, wheel_dist=None, body_dist=None, stone_collision=None,
                 stone_margin=0.0, done_u8=None, ray_src=None, hit_pt=None):
        e, f, i64 = self.num_envs, torch.float32, torch.int64
        stride = 0
        if obs is not None:
            if obs.dim() != 2 or obs.shape[0] != e or obs.shape[1] != self.num_observations or obs.stride(1) != 1:
                raise RoverError(f"obs: expected [{e},{self.num_observations}] float32 rows, got {tuple(obs.shape)}")
            if obs.dtype != f or not obs.is_cuda:
                raise RoverError("obs: expected float32 on the GPU")
            stride = obs.stride(0)
        for t, sh, dt, n in ((rew, (e,), f, "rew"), (reset, (e,), i64, "reset"), (rock_collision, (e,), i64, "rock_collision"),
                             (reset_ids, (e,), i64, "reset_ids"), (n_reset, (1,), torch.int32, "n_reset"), (euler, (e, 3), f, "euler"),
                             (heading_diff, (e,), f, "heading_diff"), (ray_dist, (e, self.P), f, "ray_dist"), (wheel_dist, (e, 24), f, "wheel_dist"),
                             (body_dist, (e, 2), f, "body_dist"), (stone_collision, (e,), i64, "stone_collision"),
                             (done_u8, (e,), torch.uint8, "done_u8"), (ray_src, (e, self.P, 3), f, "ray_src"), (hit_pt, (e, self.P, 3), f, "hit_pt")):
            self._chk(t, sh, dt, n)
        ex = extras or {}
        for k in EXTRAS:
            self._chk(ex.get(k), (e,), i64 if k == "collision_penalty" else f, "extras." + k)
        sout = StepOut(_ptr(obs), stride, _ptr(rew), _ptr(reset), _ptr(rock_collision),
                       *[_ptr(ex.get(k)) for k in EXTRAS], _ptr(reset_ids), _ptr(n_reset), _ptr(euler),
                       _ptr(heading_diff), _ptr(ray_dist), _ptr(wheel_dist), _ptr(body_dist), _ptr(stone_collision),
                       float(stone_margin), _ptr(done_u8), _ptr(ray_src), _ptr(hit_pt))
        sout._keep = (obs, rew, reset, rock_collision, dict(ex), reset_ids, n_reset, euler, heading_diff, ray_dist, wheel_dist,
                      body_dist, stone_collision, done_u8, ray_src, hit_pt)
        return sout

    def step(self, sin: StepIn, sout: StepOut, increment_progress=True, compact=False):
        # the per-step hot path, like the two bind_* closures below: the function object and the stream accessor directly, not _call
        flags = (STEP_INCREMENT_PROGRESS if increment_progress else 0) | (STEP_COMPACT if compact else 0)
        self._check(self.lib.rover_step(self._h, C.byref(sin), C.byref(sout), flags, _stream(self._dev_index)), "rover_step")

    def get_observations(self, sin, sout):
        self._call("rover_get_observations", C.byref(sin), C.byref(sout))

    def calculate_metrics(self, sin, sout):
        self._call("rover_calculate_metrics", C.byref(sin), C.byref(sout))

    def is_done(self, sin, sout):
        self._call("rover_is_done", C.byref(sin), C.byref(sout))

    def get_depths(self, positions, rotations):
        """Camera.get_depths (camera.py:60-145): positions [E,3], rotations [E,3] euler angles -> (distances [E,P], points [E,P,3],
        sources [E,P,3])."""
        e, f = self.num_envs, torch.float32
        self._chk(positions, (e, 3), f, "positions")
        self._chk(rotations, (e, 3), f, "rotations")
        dist = torch.empty(e, self.P, device=positions.device)
        pts = torch.empty(e, self.P, 3, device=positions.device)
        src = torch.empty(e, self.P, 3, device=positions.device)
        self._call("rover_get_depths", _ptr(positions), _ptr(rotations), _ptr(dist), _ptr(pts), _ptr(src))
        return dist, pts, src

    def get_collisions(self, positions, rotations, joints=None):
        """Rock_Detection.get_collisions (rock_detect.py:52-149): positions [E,3], rotations [E,3] euler angles, joints [E,13] (None =
        zero) -> (wheel_dist [E,24], body_dist [E,2])."""
        e, f = self.num_envs, torch.float32
        self._chk(positions, (e, 3), f, "positions")
        self._chk(rotations, (e, 3), f, "rotations")
        if joints is not None:
            self._chk(joints, (e, 13), f, "joints")
        wheel = torch.empty(e, 24, device=positions.device)
        body = torch.empty(e, 2, device=positions.device)
        self._call("rover_get_collisions", _ptr(positions), _ptr(rotations), _ptr(joints), _ptr(wheel), _ptr(body))
        return wheel, body

    def export_rays(self):
        """The rays of the last cast in slot order (24 wheel, 2 body, P heightmap rays per env): (src [E,R,3], dir [E,R,3] — the ray
        record's direction -normalize(direction) —, cell [E,R] int32, dist [E,R]), R = 26 + P."""
        e, r = self.num_envs, 26 + self.P
        src = torch.empty(e, r, 3, device=self.device)
        dirs = torch.empty(e, r, 3, device=self.device)
        cell = torch.empty(e, r, dtype=torch.int32, device=self.device)
        dist = torch.empty(e, r, device=self.device)
        self._call("rover_export_rays", _ptr(src), _ptr(dirs), _ptr(cell), _ptr(dist))
        return src, dirs, cell, dist

    def cast_rays(self, src, dirs):
        """Casts caller-supplied rays (layout of export_rays: origins, record directions) through the sort + ray-cast kernels."""
        e, r, f = self.num_envs, 26 + self.P, torch.float32
        self._chk(src, (e, r, 3), f, "src")
        self._chk(dirs, (e, r, 3), f, "dir")
        dist = torch.empty(e, r, device=self.device)
        self._call("rover_cast_rays", _ptr(src), _ptr(dirs), _ptr(dist))
        return dist

    def compact_resets(self, reset, reset_ids, n_reset):
        self._chk(reset, (self.num_envs,), torch.int64, "reset")
        self._chk(reset_ids, (self.num_envs,), torch.int64, "reset_ids")
        self._chk(n_reset, (1,), torch.int32, "n_reset")
        self._call("rover_compact_resets", _ptr(reset), _ptr(reset_ids), _ptr(n_reset))

    def quat_to_euler(self, quat, out=None):
        n = quat.shape[0]
        self._chk(quat, (n, 4), torch.float32, "quat")
        out = torch.empty(n, 3, device=self.device) if out is None else out
        self._chk(out, (n, 3), torch.float32, "euler")
        self._call("rover_quat_to_euler", _ptr(quat), _ptr(out), n)
        return out

    # ---- evaluation mode (rover.py:122-137, 620-641, 670-672) -------------------------------------
    def set_evaluation(self, enable=True):
        """Turns the per-env outcome latch on (fresh zeroed codes and steps, synchronises) or off (frees them)."""
        self.generation += 1
        self._call("rover_set_evaluation", 1 if enable else 0)

    def eval_clear(self, env_ids=None):
        """Re-arms the given LOCAL env ids (int64 device tensor), or every env: code 0, step 0.  With ids the call synchronises."""
        self.generation += 1
        n = 0
        if env_ids is not None:
            n = env_ids.shape[0]
            self._chk(env_ids, (n,), torch.int64, "env_ids")
        self._call("rover_eval_clear", _ptr(env_ids), n)

    def eval_read(self, eval_res=None, eval_step=None, summary8=None):
        """Enqueues copies of the codes [E], the latch steps [E] and / or the summary [8] (counts of codes 0..3, sums of the steps
        over codes 0..3) into the given int64 device tensors; no host sync."""
        e = self.num_envs
        self._chk(eval_res, (e,), torch.int64, "eval_res")
        self._chk(eval_step, (e,), torch.int64, "eval_step")
        self._chk(summary8, (8,), torch.int64, "summary8")
        self._call("rover_eval_read", _ptr(eval_res), _ptr(eval_step), _ptr(summary8))

    def set_option(self, name, value):
        self.generation += 1
        self._call("rover_set_option", name.encode(), int(value))

    def set_profiling(self, enable=True, every=1):
        """Bracket the ray-cast launch of every `every`-th step with hipEvents (get_profile() sums them)."""
        self.generation += 1
        self._call("rover_set_profiling", max(1, int(every)) if enable else 0)

    def get_profile(self):
        p = Profile()
        self._call("rover_get_profile", C.byref(p))
        return p

    def replay_raycast(self, stream=None):
        self._call("rover_replay_raycast", stream=stream)

    # ---- reset path ----------------------------------------------------------------------------
    def clearance(self, xy):
        n = xy.shape[0]
        self._chk(xy, (n, 2), torch.float32, "xy")
        out = torch.empty(n, device=self.device)
        self._call("rover_clearance", _ptr(xy), n, _ptr(out))
        return out

    def shift_spawns(self, pos3, max_iter=100000):
        n = pos3.shape[0]
        self._chk(pos3, (n, 3), torch.float32, "pos3")
        self._call("rover_shift_spawns", _ptr(pos3), n, int(max_iter))
        return pos3

    def sample_height(self, xy):
        n = xy.shape[0]
        self._chk(xy, (n, 2), torch.float32, "xy")
        out = torch.empty(n, device=self.device)
        self._call("rover_sample_height", _ptr(xy), n, _ptr(out))
        return out

    def generate_goals(self, env_ids, initial_pos3, target3, radius=8.0, draws=None, max_draws=64, seed=0,
                       n_draws_used=None):
        n = env_ids.shape[0]
        self._chk(env_ids, (n,), torch.int64, "env_ids")
        self._chk(initial_pos3, (self.num_envs, 3), torch.float32, "initial_pos3")
        self._chk(target3, (self.num_envs, 3), torch.float32, "target3")
        if draws is not None:
            self._chk(draws, (draws.shape[0], n), torch.float32, "draws")
            max_draws = draws.shape[0]
        self._chk(n_draws_used, (1,), torch.int32, "n_draws_used")
        self._call("rover_generate_goals", _ptr(env_ids), n, _ptr(initial_pos3), _ptr(target3), float(radius), _ptr(draws), int(max_draws),
                   int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(n_draws_used))

    def _reset_io(self, reset_ids, initial_pos3, pos3, quat4, reset, progress, n_reset_dev=None, n_reset_host=0,
                  joint_pos13=None, joint_vel13=None, base_pos3=None, yaw_deg=None, target3=None, radius=8.0, draws=None,
                  max_draws=256, seed=0, n_draws_used=None, seed_dev=None):
        """Validates the arguments of rover_reset_envs and packs them (the struct keeps its tensors alive)."""
        e, f, i64 = self.num_envs, torch.float32, torch.int64
        self._chk(seed_dev, (1,), i64, "seed_dev")
        self._chk(reset_ids, (e,), i64, "reset_ids")
        for t, sh, n in ((initial_pos3, (e, 3), "initial_pos3"), (pos3, (e, 3), "pos3"), (quat4, (e, 4), "quat4"),
                         (joint_pos13, (e, 13), "joint_pos13"), (joint_vel13, (e, 13), "joint_vel13"),
                         (base_pos3, (e, 3), "base_pos3"), (target3, (e, 3), "target3")):
            self._chk(t, sh, f, n)
        self._chk(reset, (e,), i64, "reset")
        self._chk(progress, (e,), i64, "progress")
        self._chk(n_reset_dev, (1,), torch.int32, "n_reset_dev")
        self._chk(n_draws_used, (1,), torch.int32, "n_draws_used")
        if yaw_deg is not None:
            self._chk(yaw_deg, (yaw_deg.shape[0],), torch.int32, "yaw_deg")
            need = e if n_reset_dev is not None else int(n_reset_host)      # entry i belongs to reset_ids[i]; with the count on
            if yaw_deg.shape[0] < need:                                     # the device any i < num_envs may be read
                raise RoverError(f"yaw_deg: {yaw_deg.shape[0]} entries, but up to {need} may be read")
        if draws is not None:
            self._chk(draws, (draws.shape[0], int(n_reset_host)), f, "draws")
            max_draws = draws.shape[0]
        io = ResetIO(_ptr(reset_ids), _ptr(n_reset_dev), int(n_reset_host), _ptr(initial_pos3), _ptr(pos3), _ptr(quat4),
                     _ptr(joint_pos13), _ptr(joint_vel13), _ptr(base_pos3), _ptr(reset), _ptr(progress), _ptr(yaw_deg),
                     _ptr(target3), float(radius), _ptr(draws), int(max_draws), int(seed) & 0xFFFFFFFFFFFFFFFF,
                     _ptr(n_draws_used), 0 if yaw_deg is None else int(yaw_deg.shape[0]), _ptr(seed_dev))
        io._keep = (reset_ids, initial_pos3, pos3, quat4, reset, progress, n_reset_dev, joint_pos13, joint_vel13, base_pos3, yaw_deg,
                    target3, draws, n_draws_used, seed_dev)
        return io

    def reset_envs(self, *args, **kw):
        """rover_reset_envs (reset_idx + set_targets for the compacted ids, rover.py:416-453,566-584); arguments: `_reset_io`."""
        self._call("rover_reset_envs", C.byref(self._reset_io(*args, **kw)))

    def bind_reset_envs(self, *args, **kw):
        """reset_envs with everything but the seed validated and packed ONCE: returns call(seed) (for a task whose buffers persist)."""
        io = self._reset_io(*args, **kw)
        fn, check, idx, h = self.lib.rover_reset_envs, self._check, self._dev_index, self._h

        def call(seed):
            io.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
            check(fn(h, C.byref(io), _stream(idx)), "rover_reset_envs")
        return call

    def bind_pre_physics(self, quat, lin_hist, ang_hist, euler_pre=None, pos_targets13=None, vel_targets13=None, actions_nn=None):
        """Validates the persistent tensors ONCE and returns call(actions), which enqueues rover_pre_physics_step on them (for a task whose
        buffers are persistent: the per-call checks are a sizeable part of a small batch's host cost).  Only the actions tensor — usually a
        fresh policy output every step — is checked per call.  The callable keeps the bound tensors alive."""
        e, f = self.num_envs, torch.float32
        for t, sh, n in ((quat, (e, 4), "quat"), (lin_hist, (e, 3), "lin_hist"),
                         (ang_hist, (e, 3), "ang_hist"), (euler_pre, (e, 3), "euler_pre"), (pos_targets13, (e, 13), "pos_targets13"),
                         (vel_targets13, (e, 13), "vel_targets13"), (actions_nn, (e, 2, 3), "actions_nn")):
            self._chk(t, sh, f, n)
        keep = (quat, lin_hist, ang_hist, euler_pre, pos_targets13, vel_targets13, actions_nn)
        rest = [_ptr(t) for t in keep]
        fn, check, idx, h, chk = self.lib.rover_pre_physics_step, self._check, self._dev_index, self._h, self._chk

        def call(actions, _keep=keep):
            chk(actions, (e, 2), f, "actions")
            check(fn(h, C.c_void_p(actions.data_ptr()), *rest, _stream(idx)), "rover_pre_physics_step")
        return call

    def pre_physics_step(self, actions, *args, **kw):
        """rover_pre_physics_step on the given tensors; arguments after ``actions``: `bind_pre_physics`."""
        self.bind_pre_physics(*args, **kw)(actions)

    def ackermann(self, lin, ang):
        n = lin.shape[0]
        self._chk(lin, (n,), torch.float32, "lin")
        self._chk(ang, (n,), torch.float32, "ang")
        steer = torch.empty(n, 6, device=self.device)
        vel = torch.empty(n, 6, device=self.device)
        self._call("rover_ackermann", _ptr(lin), _ptr(ang), n, _ptr(steer), _ptr(vel))
        return steer, vel
