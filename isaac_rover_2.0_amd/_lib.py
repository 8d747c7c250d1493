"""ctypes binding of librover_step.so (C ABI in include/rover_step.h).

There is NO CPU fallback: if the HIP library is missing or a call fails, this module raises.
Tensors are PyTorch-ROCm tensors; only their ``data_ptr()`` crosses the boundary, and work is
enqueued on ``torch.cuda.current_stream()``.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import torch

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(_CSRC, "librover_step.so")

MAP_TERRAIN, MAP_ROCKS = 0, 1
STEP_INCREMENT_PROGRESS, STEP_COMPACT = 1, 2

EXTRAS = ("pos_reward", "collision_penalty", "uprightness_penalty", "heading_contraint_penalty",
          "motion_contraint_penalty", "goal_angle_penalty", "torque_penalty_driving", "torque_penalty_steering")


class RoverError(RuntimeError):
    pass


class Cfg(C.Structure):
    _fields_ = [("num_envs", C.c_int32), ("num_envs_global", C.c_int32), ("env_offset", C.c_int32),
                ("device", C.c_int32), ("curriculum_level", C.c_int32), ("max_episode_length", C.c_int32),
                ("pos_reward", C.c_float), ("heading_contraint_reward", C.c_float),
                ("motion_contraint_reward", C.c_float), ("goal_angle_reward", C.c_float),
                ("boogie_contraint_reward", C.c_float)]


class StepIn(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("pos", "quat", "joints", "target", "lin_hist", "ang_hist", "euler_pre",
                                          "progress")]


class StepOut(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("obs_stride", C.c_int64), ("rew", C.c_void_p), ("reset", C.c_void_p),
                ("rock_collision", C.c_void_p), ("ex_pos_reward", C.c_void_p), ("ex_collision_penalty", C.c_void_p),
                ("ex_uprightness_penalty", C.c_void_p), ("ex_heading_contraint_penalty", C.c_void_p),
                ("ex_motion_contraint_penalty", C.c_void_p), ("ex_goal_angle_penalty", C.c_void_p),
                ("ex_torque_penalty_driving", C.c_void_p), ("ex_torque_penalty_steering", C.c_void_p),
                ("reset_ids", C.c_void_p), ("n_reset", C.c_void_p), ("euler", C.c_void_p),
                ("heading_diff", C.c_void_p), ("ray_dist", C.c_void_p), ("wheel_dist", C.c_void_p),
                ("body_dist", C.c_void_p), ("stone_collision", C.c_void_p), ("stone_margin", C.c_float),
                ("done_u8", C.c_void_p), ("ray_src", C.c_void_p), ("hit_pt", C.c_void_p)]


class Info(C.Structure):
    _fields_ = [("P", C.c_int32), ("Ns", C.c_int32), ("Nd", C.c_int32), ("rays_per_env_padded", C.c_int32),
                ("K", C.c_int32 * 2), ("K8", C.c_int32 * 2), ("X", C.c_int32 * 2), ("Y", C.c_int32 * 2),
                ("table_bytes", C.c_uint64 * 2), ("workspace_bytes", C.c_uint64), ("raycast_variant", C.c_int32),
                ("cell_index_mode", C.c_int32), ("ray_precision", C.c_int32), ("raycast_sorted", C.c_int32),
                ("raycast_rocks_staged", C.c_int32), ("lane_box", C.c_int32 * 2), ("lane_pair_rows", C.c_int32 * 2)]


class CullInfo(C.Structure):
    _fields_ = [("triangles", C.c_int64 * 2), ("always_candidate_triangles", C.c_int64 * 2), ("cells_without_cone", C.c_int64 * 2),
                ("rays", C.c_uint64), ("candidate_pairs", C.c_uint64), ("rays_both_tests", C.c_uint64), ("bins", C.c_uint64),
                ("max_pairs_per_run", C.c_uint64), ("queue_bytes", C.c_uint64), ("launches_per_step", C.c_uint64), ("rays_far_skipped", C.c_uint64),
                ("cells_with_far_bound", C.c_int64 * 2), ("far_records_on_demand", C.c_uint64), ("rays_not_scanned", C.c_uint64),
                ("lane_items", C.c_uint64), ("lane_flushes", C.c_uint64)]


class RaycastPlan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("variant", "proof", "sorted", "env_order", "rocks_staged", "run", "env_run", "lazy_far",
                                         "skip_clear", "cull_launches", "low_bits", "sort_entry_dwords", "hist_fused")]


class PlanQuery(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_envs", "P", "have_dist", "ray_precision", "raycast_variant", "raycast_run", "lane_env_order",
                                         "lane_rocks", "bin_low_bits", "cull_lazy")]
    _fields_ += [("cull_queue_mb", C.c_int64), ("map_present", C.c_int32 * 2), ("X", C.c_int32 * 2), ("Y", C.c_int32 * 2), ("K8", C.c_int32 * 2),
                 ("cells_with_far_bound", C.c_int64 * 2), ("has_cull_tables", C.c_int32 * 2), ("has_staged_tables", (C.c_int32 * 2) * 2)]


class ChainDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_stride", C.c_int64), ("K0", C.c_int32), ("n_layers", C.c_int32), ("weights", C.c_void_p),
                ("biases", C.c_void_p), ("widths", C.c_void_p), ("activations", C.c_void_p), ("y", C.c_void_p), ("y_stride", C.c_int64)]


class GaussHead(C.Structure):
    _fields_ = [("log_std", C.c_void_p), ("A", C.c_int32), ("clip_log_std", C.c_int32), ("min_log_std", C.c_float), ("max_log_std", C.c_float),
                ("clip_actions", C.c_int32), ("low", C.c_float), ("high", C.c_float), ("reduction", C.c_int32), ("deterministic", C.c_int32),
                ("seed", C.c_uint64), ("step", C.c_uint64), ("step_dev", C.c_void_p), ("row_offset", C.c_int64),
                ("taken_actions", C.c_void_p), ("taken_stride", C.c_int64), ("actions", C.c_void_p), ("actions_stride", C.c_int64),
                ("log_prob", C.c_void_p), ("log_prob_stride", C.c_int64), ("mean", C.c_void_p), ("mean_stride", C.c_int64)]


class GaeDesc(C.Structure):
    _fields_ = [("T", C.c_int32), ("E", C.c_int32), ("gamma", C.c_float), ("lam", C.c_float), ("rewards", C.c_void_p), ("rewards_stride", C.c_int64),
                ("values", C.c_void_p), ("values_stride", C.c_int64), ("dones", C.c_void_p), ("dones_stride", C.c_int64), ("last_values", C.c_void_p),
                ("returns", C.c_void_p), ("returns_stride", C.c_int64), ("advantages", C.c_void_p), ("advantages_stride", C.c_int64),
                ("normalize", C.c_int32), ("stats_out", C.c_void_p), ("stats_in", C.c_void_p)]


GAE_RAW, GAE_NORMALIZE, GAE_NORMALIZE_GIVEN = 0, 1, 2


class PpoLossDesc(C.Structure):
    _fields_ = [("M", C.c_int32), ("A", C.c_int32), ("mean", C.c_void_p), ("mean_stride", C.c_int64), ("log_std", C.c_void_p),
                ("actions", C.c_void_p), ("actions_stride", C.c_int64), ("old_log_prob", C.c_void_p), ("advantages", C.c_void_p),
                ("value", C.c_void_p), ("old_values", C.c_void_p), ("returns", C.c_void_p), ("clip_log_std", C.c_int32),
                ("min_log_std", C.c_float), ("max_log_std", C.c_float), ("reduction", C.c_int32), ("ratio_clip", C.c_float),
                ("value_clip", C.c_float), ("clip_predicted_values", C.c_int32), ("entropy_loss_scale", C.c_float),
                ("value_loss_scale", C.c_float), ("d_mean", C.c_void_p), ("d_mean_stride", C.c_int64), ("d_value", C.c_void_p),
                ("d_log_std", C.c_void_p), ("stats", C.c_void_p)]


class OptimChunk(C.Structure):
    _fields_ = [("tensor", C.c_int32), ("first", C.c_int32), ("length", C.c_int32)]


class OptimDesc(C.Structure):
    _fields_ = [("n_tensors", C.c_int32), ("params", C.c_void_p), ("grads", C.c_void_p), ("numel", C.c_void_p), ("exp_avg", C.c_void_p),
                ("exp_avg_sq", C.c_void_p), ("step", C.c_void_p), ("stopped", C.c_void_p)]


class OptimStepDesc(C.Structure):
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("grad_norm_clip", C.c_double),
                ("gate", C.c_void_p), ("gate_threshold", C.c_double), ("norm_out", C.c_void_p)]


class ObsNoiseDesc(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("in_stride", C.c_int64), ("out", C.c_void_p), ("out_stride", C.c_int64), ("M", C.c_int32), ("F", C.c_int32),
                ("first", C.c_int32), ("sigma_point", C.c_float), ("sigma_offset", C.c_float), ("dropout", C.c_double), ("drop_value", C.c_float),
                ("row_scale", C.c_void_p), ("episode", C.c_void_p), ("seed", C.c_uint64), ("step", C.c_uint64), ("step_dev", C.c_void_p),
                ("row_offset", C.c_int64)]


class OcclusionCfg(C.Structure):
    _fields_ = [("camera", C.c_float * 3), ("step", C.c_float), ("clearance", C.c_float), ("max_steps", C.c_int32), ("miss", C.c_float)]


class ObsOcclusionDesc(C.Structure):
    _fields_ = [("pos3", C.c_void_p), ("quat4", C.c_void_p), ("clean", C.c_void_p), ("clean_stride", C.c_int64), ("in_", C.c_void_p),
                ("in_stride", C.c_int64), ("out", C.c_void_p), ("out_stride", C.c_int64), ("M", C.c_int32), ("F", C.c_int32), ("first", C.c_int32),
                ("drop_value", C.c_float), ("hidden_u8", C.c_void_p), ("hidden_stride", C.c_int64), ("target3", C.c_void_p)]


class ScalerPlanDesc(C.Structure):
    _fields_ = [("route", C.c_int32), ("rows_per_chunk", C.c_int32), ("n_chunks", C.c_int32), ("scratch_bytes", C.c_int64)]


SCALER_WIDE, SCALER_NARROW = 0, 1


class ScalerUpdateDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_stride", C.c_int64), ("M", C.c_int32), ("N", C.c_int32), ("mean", C.c_void_p), ("var", C.c_void_p),
                ("count", C.c_void_p), ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64), ("skip_if", C.c_void_p)]


class ScalerApplyDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_stride", C.c_int64), ("y", C.c_void_p), ("y_stride", C.c_int64), ("M", C.c_int32), ("N", C.c_int32),
                ("mean", C.c_void_p), ("var", C.c_void_p), ("epsilon", C.c_double), ("clip", C.c_double), ("inverse", C.c_int32)]


class MotionDesc(C.Structure):
    _fields_ = [("pos3", C.c_void_p), ("quat4", C.c_void_p), ("lin", C.c_void_p), ("ang", C.c_void_p), ("cmd_stride", C.c_int32), ("E", C.c_int32),
                ("substeps", C.c_int32), ("dt", C.c_float), ("max_lin", C.c_float), ("max_ang", C.c_float), ("ride_height", C.c_float),
                ("joint_pos_targets13", C.c_void_p), ("joint_vel_targets13", C.c_void_p), ("joint_pos13", C.c_void_p), ("joint_vel13", C.c_void_p)]


class BogieParams(C.Structure):
    _fields_ = [("iters", C.c_int32), ("max_bogie", C.c_float)]


SUSPENSIONS = ("plane", "bogie")
MARS_MAX_SIDE, MARS_MAX_CLASSES, MARS_MAX_TABLE, MARS_TILE = 131072, 16, 129, 16


class MarsDesc(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("n_hills", C.c_int32), ("hill_window", C.c_void_p), ("hill_amp", C.c_void_p),
                ("g", C.c_void_p), ("g_len", C.c_int32), ("n_classes", C.c_int32), ("class_side", C.c_void_p), ("class_tables", C.c_void_p),
                ("n_stamps", C.c_int32), ("stamp_row", C.c_void_p), ("stamp_col", C.c_void_p), ("stamp_class", C.c_void_p),
                ("stamp_factor", C.c_void_p), ("stamp_kept", C.c_void_p)]


TRACK_MAX_COMPONENTS, TRACK_MAX_WINDOW = 16, 1024
TRACK_F32, TRACK_I64 = 0, 1


class TrackRecord(C.Structure):
    """rover_track_record: the interval record of rover_episode_track (240 bytes, fixed layout)."""
    _fields_ = [("calls", C.c_int64), ("inst_sum", C.c_double), ("ep_count", C.c_int64), ("ep_ret_sum", C.c_double), ("ep_ret_sumsq", C.c_double),
                ("ep_len_sum", C.c_int64), ("win_calls", C.c_int64), ("win_ret_mean_sum", C.c_double), ("win_len_mean_sum", C.c_double),
                ("comp_sum", C.c_double * TRACK_MAX_COMPONENTS), ("inst_min", C.c_float), ("inst_max", C.c_float), ("ep_ret_min", C.c_float),
                ("ep_ret_max", C.c_float), ("ep_len_min", C.c_int32), ("ep_len_max", C.c_int32), ("win_ret_min", C.c_float),
                ("win_ret_max", C.c_float), ("win_len_min", C.c_int32), ("win_len_max", C.c_int32)]


class TrackDesc(C.Structure):
    _fields_ = [("rewards", C.c_void_p), ("done", C.c_void_p), ("done_size", C.c_int32), ("E", C.c_int32), ("W", C.c_int32), ("K", C.c_int32),
                ("comp", C.c_void_p * TRACK_MAX_COMPONENTS), ("comp_kind", C.c_int32 * TRACK_MAX_COMPONENTS), ("cum_reward", C.c_void_p),
                ("cum_steps", C.c_void_p), ("ring_ret", C.c_void_p), ("ring_len", C.c_void_p), ("ring_count", C.c_void_p), ("record", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64)]


class TrackSizes(C.Structure):
    _fields_ = [("workgroup", C.c_int32), ("n_partials", C.c_int32), ("partial_bytes", C.c_int64), ("finished_slots", C.c_int64),
                ("scratch_bytes", C.c_int64)]


REDUCTIONS = {"sum": 0, "mean": 1, "prod": 2, "max": 3, "min": 4, None: 5, "none": 5}


class ResetIO(C.Structure):
    _fields_ = [("reset_ids", C.c_void_p), ("n_reset_dev", C.c_void_p), ("n_reset_host", C.c_int32),
                ("initial_pos3", C.c_void_p), ("pos3", C.c_void_p), ("quat4", C.c_void_p), ("joint_pos13", C.c_void_p),
                ("joint_vel13", C.c_void_p), ("base_pos3", C.c_void_p), ("reset", C.c_void_p), ("progress", C.c_void_p),
                ("yaw_deg", C.c_void_p), ("target3", C.c_void_p), ("radius", C.c_float), ("draws", C.c_void_p),
                ("max_draws", C.c_int32), ("seed", C.c_uint64), ("n_draws_used", C.c_void_p), ("yaw_deg_len", C.c_int32),
                ("seed_dev", C.c_void_p)]


class Profile(C.Structure):
    _fields_ = [("raycast_ms", C.c_double), ("launches", C.c_int32), ("pairs_per_launch", C.c_uint64)]


# every symbol include/rover_step.h declares: (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "rover_create": (C.c_int, [C.POINTER(Cfg), C.POINTER(_P)]),
    "rover_destroy": (None, [_P]),
    "rover_last_error": (C.c_char_p, [_P]),
    "rover_version": (C.c_char_p, []),
    "rover_set_knn_map": (C.c_int, [_P, C.c_int, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32,
                                    C.c_float, C.c_float, C.c_float]),
    "rover_set_distribution": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32]),
    "rover_set_heightfield": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float]),
    "rover_set_stones": (C.c_int, [_P, _P, C.c_int32]),
    "rover_set_curriculum_level": (C.c_int, [_P, C.c_int32]),
    "rover_step": (C.c_int, [_P, C.POINTER(StepIn), C.POINTER(StepOut), C.c_uint32, _P]),
    "rover_get_observations": (C.c_int, [_P, C.POINTER(StepIn), C.POINTER(StepOut), _P]),
    "rover_calculate_metrics": (C.c_int, [_P, C.POINTER(StepIn), C.POINTER(StepOut), _P]),
    "rover_is_done": (C.c_int, [_P, C.POINTER(StepIn), C.POINTER(StepOut), _P]),
    "rover_compact_resets": (C.c_int, [_P, _P, _P, _P, _P]),
    "rover_get_depths": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "rover_get_collisions": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "rover_export_rays": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "rover_cast_rays": (C.c_int, [_P, _P, _P, _P, _P]),
    "rover_quat_to_euler": (C.c_int, [_P, _P, _P, C.c_int32, _P]),
    "rover_clearance": (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    "rover_shift_spawns": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "rover_sample_height": (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    "rover_generate_goals": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_float, _P, C.c_int32, C.c_uint64, _P, _P]),
    "rover_reset_envs": (C.c_int, [_P, C.POINTER(ResetIO), _P]),
    "rover_pre_physics_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rover_ackermann": (C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P]),
    "rover_get_info": (C.c_int, [_P, C.POINTER(Info)]),
    "rover_get_cull_info": (C.c_int, [_P, C.POINTER(CullInfo)]),
    "rover_get_raycast_plan": (C.c_int, [_P, C.POINTER(RaycastPlan)]),
    "rover_plan_raycast": (C.c_int, [C.POINTER(PlanQuery), C.POINTER(RaycastPlan)]),
    "rover_replay_raycast": (C.c_int, [_P, _P]),
    "rover_build_knn_map": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P]),
    "rover_build_knn_map_ref": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P, _P, _P]),
    "rover_build_heightfield": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P]),
    "rover_heightfield_limits": (C.c_int, [_P]),
    "rover_mars_heightfield": (C.c_int, [_P, C.POINTER(MarsDesc), _P, _P, _P]),
    "rover_mars_tiles": (C.c_int, [C.POINTER(MarsDesc), _P, _P, C.c_int64, _P]),
    "rover_linear_forward": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, C.c_int64, _P]),
    "rover_mlp_chain_forward": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "rover_mlp_chain_pair_forward": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int64, _P, C.c_int64, C.c_int32, _P]),
    "rover_linear_route": (C.c_char_p, [C.c_int32, C.c_int32, C.c_int32]),
    "rover_mlp_chain_route": (C.c_char_p, [C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "rover_mlp_chain_pair_route": (C.c_char_p, [C.c_int32, C.POINTER(ChainDesc), C.POINTER(ChainDesc)]),
    "rover_mlp_chain_act": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int64, C.POINTER(GaussHead), _P]),
    "rover_gaussian_head": (C.c_int, [_P, C.c_int32, C.POINTER(GaussHead), _P]),
    "rover_policy_noise": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, _P]),
    "rover_philox4x32": (C.c_int, [_P, _P, _P]),
    "rover_mlp_chain_act_route": (C.c_char_p, [C.c_int32, C.c_int32, C.c_int32, _P, _P, C.POINTER(GaussHead)]),
    "rover_mlp_chain_forward_bf16": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "rover_mlp_chain_act_bf16": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int64, C.POINTER(GaussHead), _P]),
    "rover_mlp_chain_route_bf16": (C.c_char_p, [C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "rover_mlp_chain_act_route_bf16": (C.c_char_p, [C.c_int32, C.c_int32, C.c_int32, _P, _P, C.POINTER(GaussHead)]),
    "rover_bf16_round": (C.c_int, [_P, C.c_int64, _P]),
    "rover_linear_forward_bf16": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, C.c_int64, _P]),
    "rover_linear_route_bf16": (C.c_char_p, [C.c_int32, C.c_int32, C.c_int32]),
    "rover_gae": (C.c_int, [_P, C.POINTER(GaeDesc), _P]),
    "rover_combine_moments": (C.c_int, [_P, _P, _P]),
    "rover_linear_backward": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P, C.c_int64,
                                        _P, _P, _P]),
    "rover_linear_backward_route": (C.c_char_p, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rover_ppo_loss": (C.c_int, [_P, C.POINTER(PpoLossDesc), _P]),
    "rover_optim_plan": (C.c_int, [C.c_int32, _P, _P, C.c_int64, _P]),
    "rover_optim_create": (C.c_int, [_P, C.POINTER(OptimDesc), _P]),
    "rover_optim_destroy": (C.c_int, [_P, C.c_int32]),
    "rover_optim_step": (C.c_int, [_P, C.c_int32, C.POINTER(OptimStepDesc), _P]),
    "rover_gru_cell": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "rover_gru_cell_route": (C.c_char_p, [C.c_int32, C.c_int32, C.c_int32]),
    "rover_gru_cell_bf16": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "rover_gru_cell_route_bf16": (C.c_char_p, [C.c_int32, C.c_int32, C.c_int32]),
    "rover_gated_sum": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, _P]),
    "rover_gru_cell_train": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int64, _P, C.c_int64,
                                       _P]),
    "rover_gru_cell_backward": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int32, C.c_int32, _P, C.c_int64, _P,
                                          C.c_int64, _P, C.c_int64, _P]),
    "rover_gru_cell_backward_route": (C.c_char_p, [C.c_int32, C.c_int32]),
    "rover_gated_sum_backward": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, _P, C.c_int64, _P]),
    "rover_linear_dgrad": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P, C.c_int64, _P]),
    "rover_linear_dgrad_route": (C.c_char_p, [C.c_int32, C.c_int32, C.c_int32]),
    "rover_obs_noise": (C.c_int, [_P, C.POINTER(ObsNoiseDesc), _P]),
    "rover_obs_noise_threshold": (C.c_int, [C.c_double, _P]),
    "rover_set_occlusion": (C.c_int, [_P, C.POINTER(OcclusionCfg)]),
    "rover_obs_occlusion": (C.c_int, [_P, C.POINTER(ObsOcclusionDesc), _P]),
    "rover_occlusion_order": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P]),
    "rover_scaler_plan": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(ScalerPlanDesc)]),
    "rover_scaler_update": (C.c_int, [_P, C.POINTER(ScalerUpdateDesc), _P]),
    "rover_scaler_apply": (C.c_int, [_P, C.POINTER(ScalerApplyDesc), _P]),
    "rover_motion_step": (C.c_int, [_P, C.POINTER(MotionDesc), _P]),
    "rover_motion_plane_fit": (C.c_int, [_P]),
    "rover_motion_step_bogie": (C.c_int, [_P, C.POINTER(MotionDesc), C.POINTER(BogieParams), _P]),
    "rover_motion_bogie_fit": (C.c_int, [_P]),
    "rover_episode_track": (C.c_int, [_P, C.POINTER(TrackDesc), _P]),
    "rover_track_sizes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(TrackSizes)]),
    "rover_set_evaluation": (C.c_int, [_P, C.c_int32]),
    "rover_eval_clear": (C.c_int, [_P, _P, C.c_int32, _P]),
    "rover_eval_read": (C.c_int, [_P, _P, _P, _P, _P]),
    "rover_set_option": (C.c_int, [_P, C.c_char_p, C.c_int64]),
    "rover_set_profiling": (C.c_int, [_P, C.c_int32]),
    "rover_get_profile": (C.c_int, [_P, C.POINTER(Profile)]),
}

_lib = None


def _sources():
    """The files the library is built from (csrc/SOURCES, one per line, relative to csrc/): build.sh compiles and hashes the same list."""
    with open(os.path.join(_CSRC, "SOURCES")) as f:
        return [os.path.join(_CSRC, line.strip()) for line in f if line.strip()]


def build(force: bool = False) -> str:
    """Compile the HIP library in-tree (hipcc cross-compiles gfx950 without a GPU)."""
    srcs = _sources() + [os.path.join(_CSRC, "SOURCES"), os.path.join(_CSRC, "build.sh")]
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["bash", os.path.join(_CSRC, "build.sh")])
    return LIB_PATH


def load():
    """dlopen librover_step.so and bind every declared symbol; raises if the library is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RoverError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(there is no CPU fallback for the rover step path)")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)      # AttributeError if the .so does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def version() -> str:
    """rover_version(): "rover_step <ver> (gfx950) src-<12 hex>": the hash of the sources the loaded library was built from."""
    return load().rover_version().decode()


def source_hash() -> str:
    """The same hash computed from the source files in the tree (what a fresh build.sh would embed)."""
    import hashlib
    h = hashlib.sha256()
    for f in _sources():
        h.update(open(f, "rb").read())
    return h.hexdigest()[:12]


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
    lib = load()
    rc = lib.rover_plan_raycast(C.byref(q), C.byref(out))
    if rc != 0:
        raise RoverError(f"rover_plan_raycast failed ({rc}): {lib.rover_last_error(None).decode()}")
    return {k: int(getattr(out, k)) for k, _ in RaycastPlan._fields_}


def philox4x32(counter, key):
    """rover_philox4x32: the four Philox4x32-10 words for ``counter`` (4 uint32) and ``key`` (2 uint32), computed on the host by the
    round function the kernels run.  No ctx, no device."""
    c = (C.c_uint32 * 4)(*[int(v) & 0xffffffff for v in counter])
    k = (C.c_uint32 * 2)(*[int(v) & 0xffffffff for v in key])
    out = (C.c_uint32 * 4)()
    lib = load()
    rc = lib.rover_philox4x32(c, k, out)
    if rc != 0:
        raise RoverError(f"rover_philox4x32 failed ({rc}): {lib.rover_last_error(None).decode()}")
    return tuple(int(v) for v in out)


def combine_moments(a, b):
    """The moments (count, mean, M2) of the union of two disjoint samples from their moments ``a`` and ``b`` (Chan's pairwise update: what
    shards do with the ``stats_out`` of their Engine.gae calls before they hand the result back as ``stats_in``).  Two float64 torch
    tensors of 3 elements: the same IEEE operations in the same order on their device (the same bits as the host helper), nothing
    synchronises; an empty side (count 0) leaves the other unchanged, as on the host.  Anything else (sequences, numpy arrays):
    rover_combine_moments on the host -> a float64 numpy array of 3."""
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):
        if a.dtype != torch.float64 or b.dtype != torch.float64 or a.numel() != 3 or b.numel() != 3:
            raise RoverError("combine_moments: expected two float64 tensors of 3 elements (count, mean, M2)")
        a, b = a.reshape(3), b.reshape(3)
        n = a[0] + b[0]
        d, f = b[1] - a[1], b[0] / n
        merged = torch.stack((n, a[1] + d * f, a[2] + b[2] + d * d * (a[0] * f)))
        return torch.where(a[0] == 0, b, torch.where(b[0] == 0, a, merged))
    ha, hb, out = _host(a, np.float64).reshape(-1), _host(b, np.float64).reshape(-1), np.empty(3, dtype=np.float64)
    if ha.shape != (3,) or hb.shape != (3,):
        raise RoverError("combine_moments: expected two triples (count, mean, M2)")
    lib = load()
    rc = lib.rover_combine_moments(ha.ctypes.data, hb.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise RoverError(f"rover_combine_moments failed ({rc}): {lib.rover_last_error(None).decode()}")
    return out


_FAKE = 16          # a non-null address for the descriptor of a route query (never read)


def gauss_head_desc(A, log_std=_FAKE, actions=_FAKE, log_prob=_FAKE, clip_log_std=True, min_log_std=-20.0, max_log_std=2.0, clip_actions=False,
                    low=-1.0, high=1.0, reduction="sum", deterministic=False, seed=0, step=0, step_dev=None, row_offset=0, taken_actions=None,
                    taken_stride=None, actions_stride=None, log_prob_stride=None, mean=None, mean_stride=None):
    """A rover_gauss_head from plain values (pointers as integers; the defaults are skrl's as the reference sets them, model.py:153-156).
    ``reduction``: a name of REDUCTIONS or a code."""
    red = reduction if isinstance(reduction, int) and not isinstance(reduction, bool) else REDUCTIONS[reduction]
    A = int(A)
    return GaussHead(log_std, A, int(bool(clip_log_std)), float(min_log_std), float(max_log_std), int(bool(clip_actions)), float(low), float(high),
                     int(red), int(bool(deterministic)), int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), step_dev, int(row_offset),
                     taken_actions, A if taken_stride is None else int(taken_stride), actions, A if actions_stride is None else int(actions_stride),
                     log_prob, (A if red == 5 else 1) if log_prob_stride is None else int(log_prob_stride), mean,
                     A if mean_stride is None else int(mean_stride))


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
    lib = load()
    rc = lib.rover_obs_noise_threshold(float(dropout), C.byref(out))
    if rc != 0:
        raise RoverError(f"rover_obs_noise_threshold failed ({rc}): {lib.rover_last_error(None).decode()}")
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
    lib = load()
    rc = lib.rover_occlusion_order(pts.ctypes.data, pts.shape[0], sp.ctypes.data if len(sp) else None, len(sp), de.ctypes.data if len(de) else None,
                                   len(de), cam.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise RoverError(f"rover_occlusion_order failed ({rc}): {lib.rover_last_error(None).decode()}")
    return out


def scaler_plan(m, n):
    """rover_scaler_plan: how rover_scaler_update splits ``m`` rows of ``n`` columns, as a dict (route, rows_per_chunk, n_chunks,
    scratch_bytes).  Host only, a pure function of (m, n)."""
    out = ScalerPlanDesc()
    lib = load()
    rc = lib.rover_scaler_plan(int(m), int(n), C.byref(out))
    if rc != 0:
        raise RoverError(f"rover_scaler_plan failed ({rc}): {lib.rover_last_error(None).decode()}")
    return {name: int(getattr(out, name)) for name, _ in ScalerPlanDesc._fields_}


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


def gae_desc(t, e, rewards=1 << 40, values=2 << 40, dones=3 << 40, last_values=4 << 40, returns=5 << 40, advantages=6 << 40, stats_out=None,
             stats_in=None, normalize=GAE_RAW, gamma=0.99, lam=0.95, **strides):
    """A rover_gae_desc from plain values (pointers as integers, disjoint by default; ``<name>_stride`` defaults to ``e``)."""
    st = lambda name: int(strides.pop(name + "_stride", e))
    d = GaeDesc(int(t), int(e), float(gamma), float(lam), rewards, st("rewards"), values, st("values"), dones, st("dones"), last_values, returns,
                st("returns"), advantages, st("advantages"), int(normalize), stats_out, stats_in)
    if strides:
        raise TypeError(f"gae_desc: unknown arguments {sorted(strides)}")
    return d


def ppo_loss_desc(m, a, mean_stride=None, actions_stride=None, d_mean_stride=None, **ptrs):
    """A rover_ppo_loss_desc from plain values: skrl's scalars, the strides default to ``a``, every pointer an integer (disjoint fake
    addresses by default; ``name=None`` or another address through ``ptrs``)."""
    names = ("mean", "log_std", "actions", "old_log_prob", "advantages", "value", "old_values", "returns", "d_mean", "d_value", "d_log_std", "stats")
    p = {name: (i + 1) << 40 for i, name in enumerate(names)}
    if set(ptrs) - set(names):
        raise TypeError(f"ppo_loss_desc: unknown arguments {sorted(set(ptrs) - set(names))}")
    p.update(ptrs)
    a = int(a)
    st = lambda v: a if v is None else int(v)
    return PpoLossDesc(int(m), a, p["mean"], st(mean_stride), p["log_std"], p["actions"], st(actions_stride), p["old_log_prob"], p["advantages"], p["value"],
                       p["old_values"], p["returns"], 1, -20.0, 2.0, REDUCTIONS["sum"], 0.2, 0.2, 1, 0.0, 1.0, p["d_mean"], st(d_mean_stride), p["d_value"],
                       p["d_log_std"], p["stats"])


def motion_desc(e, pos3=_FAKE, quat4=_FAKE, lin=_FAKE, ang=_FAKE, cmd_stride=3, substeps=1, dt=0.05, max_lin=1.0, max_ang=1.0, ride_height=0.3,
                joint_pos_targets13=None, joint_vel_targets13=None, joint_pos13=None, joint_vel13=None):
    """A rover_motion_desc from plain values (pointers as integers)."""
    return MotionDesc(pos3, quat4, lin, ang, int(cmd_stride), int(e), int(substeps), float(dt), float(max_lin), float(max_ang), float(ride_height),
                      joint_pos_targets13, joint_vel_targets13, joint_pos13, joint_vel13)


def motion_plane_fit():
    """rover_motion_plane_fit: the constant C [3, 6] of the motion model's plane fit, (z_c, p, q) = C z over the six wheel contacts
    (FL, FR, ML, MR, RL, RR) -> a float32 array.  Host only."""
    out = np.empty((3, 6), dtype=np.float32)
    lib = load()
    rc = lib.rover_motion_plane_fit(out.ctypes.data)
    if rc != 0:
        raise RoverError(f"rover_motion_plane_fit failed ({rc}): {lib.rover_last_error(None).decode()}")
    return out


def motion_bogie_fit():
    """rover_motion_bogie_fit: the constant D [6, 6] of the rocker-bogie posture solve, the inverse of the Jacobian at rest of the six
    wheel-origin heights by (z_c, roll, pitch, j0, j1, j2) -> a float32 array.  Host only."""
    out = np.empty((6, 6), dtype=np.float32)
    lib = load()
    rc = lib.rover_motion_bogie_fit(out.ctypes.data)
    if rc != 0:
        raise RoverError(f"rover_motion_bogie_fit failed ({rc}): {lib.rover_last_error(None).decode()}")
    return out


def heightfield_limits():
    """rover_heightfield_limits: the sizes that separate the code paths of rover_build_heightfield as a dict — ``small_nodes``: the
    largest bounding box (nodes, clipped to the grid) one lane group rasterises; larger boxes are cut at the grid's multiples of
    ``tile_i`` x ``tile_j`` nodes, one workgroup per tile; ``group_lanes``: the lanes of a group.  Host only."""
    out = (C.c_int32 * 4)()
    lib = load()
    rc = lib.rover_heightfield_limits(out)
    if rc != 0:
        raise RoverError(f"rover_heightfield_limits failed ({rc}): {lib.rover_last_error(None).decode()}")
    return {"small_nodes": int(out[0]), "tile_i": int(out[1]), "tile_j": int(out[2]), "group_lanes": int(out[3])}


def mars_desc(rows, cols, hill_window=(), hill_amp=(), g=(1.0,), class_tables=(), stamp_row=(), stamp_col=(), stamp_class=(), stamp_factor=(),
              stamp_kept=None):
    """A rover_mars_desc from host arrays -> (MarsDesc, the arrays it points into: keep them alive as long as the descriptor).
    ``hill_window`` [H, 6] (r0, r1, c0, c1, a0, b0), ``class_tables`` a sequence of square float64 arrays, ``stamp_kept`` defaults to
    all kept.  Nothing is checked here: the library does that."""
    win = np.ascontiguousarray(hill_window, dtype=np.int32).reshape(-1, 6)
    amp = np.ascontiguousarray(hill_amp, dtype=np.float64).reshape(-1)
    gg = np.ascontiguousarray(g, dtype=np.float64).reshape(-1)
    tabs = [np.ascontiguousarray(t, dtype=np.float64) for t in class_tables]
    side = np.asarray([t.shape[0] for t in tabs], dtype=np.int32)
    flat = np.concatenate([t.reshape(-1) for t in tabs]) if tabs else np.zeros(0, dtype=np.float64)
    sr, sc, sk = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (stamp_row, stamp_col, stamp_class))
    sf = np.ascontiguousarray(stamp_factor, dtype=np.float64).reshape(-1)
    kept = np.ones(len(sr), dtype=np.uint8) if stamp_kept is None else np.ascontiguousarray(np.asarray(stamp_kept) != 0, dtype=np.uint8).reshape(-1)
    if len(win) != len(amp) or not (len(sr) == len(sc) == len(sk) == len(sf) == len(kept)) or any(t.ndim != 2 or t.shape[0] != t.shape[1] for t in tabs):
        raise RoverError("mars_desc: hill arrays, stamp arrays or class tables of inconsistent shapes")
    ptr = lambda a: a.ctypes.data if a.size else None
    d = MarsDesc(int(rows), int(cols), len(amp), ptr(win), ptr(amp), ptr(gg), len(gg), len(tabs), ptr(side), ptr(flat), len(sr), ptr(sr), ptr(sc),
                 ptr(sk), ptr(sf), ptr(kept))
    return d, (win, amp, gg, side, flat, sr, sc, sk, sf, kept)


def mars_plan_desc(plan):
    """The rover_mars_desc of a ``terrain_gen.MarsPlan`` -> (MarsDesc, keep-alive)."""
    return mars_desc(plan.side, plan.side, plan.hill_windows(), plan.hill_amp, plan.g, plan.class_tables, plan.stamp_rows, plan.stamp_cols,
                     plan.stamp_class, plan.stamp_factor, plan.stamp_kept)


def mars_tiles(desc):
    """rover_mars_tiles: the per-tile stamp lists rover_mars_heightfield builds for ``desc`` (a MarsDesc) -> (tile_start [tiles + 1],
    tile_items) int32 arrays; tile (ti, tj) of MARS_TILE^2 nodes has the number ti ceil(cols / MARS_TILE) + tj.  Host only."""
    lib = load()
    n = C.c_int64()
    rc = lib.rover_mars_tiles(C.byref(desc), None, None, 0, C.byref(n))
    if rc == 0:
        tiles = ((desc.rows + MARS_TILE - 1) // MARS_TILE) * ((desc.cols + MARS_TILE - 1) // MARS_TILE)
        start, items = np.zeros(tiles + 1, dtype=np.int32), np.zeros(max(n.value, 1), dtype=np.int32)
        rc = lib.rover_mars_tiles(C.byref(desc), start.ctypes.data, items.ctypes.data, n.value, C.byref(n))
    if rc != 0:
        raise RoverError(f"rover_mars_tiles failed ({rc}): {lib.rover_last_error(None).decode()}")
    return start, items[:n.value]


def track_sizes(e, w=100, k=0):
    """rover_track_sizes: what rover_episode_track needs for ``e`` envs as a dict (workgroup, n_partials, partial_bytes, finished_slots,
    scratch_bytes).  Host only."""
    out = TrackSizes()
    lib = load()
    rc = lib.rover_track_sizes(int(e), int(w), int(k), C.byref(out))
    if rc != 0:
        raise RoverError(f"rover_track_sizes failed ({rc}): {lib.rover_last_error(None).decode()}")
    return {name: int(getattr(out, name)) for name, _ in TrackSizes._fields_}


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


PRECISIONS = ("f32", "bf16")


def _precision_suffix(precision):
    """"" / "_bf16": the suffix of the entry points of ``precision`` (rover_mlp_chain_forward / rover_mlp_chain_forward_bf16, rover_gru_cell /
    rover_gru_cell_bf16, rover_linear_forward / rover_linear_forward_bf16 and their route queries)."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, not {precision!r}")
    return "" if precision == "f32" else "_bf16"


def chain_act_route(m, k0, widths, activations, head=None, precision="f32"):
    """rover_mlp_chain_act_route: "mlp_small+gauss" / "chain16<16,10,8,1>+gauss" (the head inside the chain's last kernel),
    "<chain route>;gauss" (the head as a launch of its own), "none" for m = 0, None where rover_mlp_chain_act would refuse the call.
    ``head``: a GaussHead (gauss_head_desc) — default: the reference's settings with A = widths[-1].  ``precision="bf16"``:
    rover_mlp_chain_act_route_bf16 ("chain_bf16<16,10,8,1>+gauss", ...)."""
    k0, n, w, a = Engine._chain_shape(k0, widths, activations)
    if head is None:
        head = gauss_head_desc(widths[-1])
    return Engine._route(getattr(load(), "rover_mlp_chain_act_route" + _precision_suffix(precision))(int(m), k0, n, w, a, C.byref(head)))


def bf16_round(values):
    """rover_bf16_round: ``values`` (anything numpy turns into float32) rounded to bf16 as the bf16 chain kernels round their inputs,
    weights and hidden activations -> a float32 array of the same shape.  Host only."""
    x = np.ascontiguousarray(values, dtype=np.float32)
    out = np.empty_like(x)
    lib = load()
    rc = lib.rover_bf16_round(x.ctypes.data, x.size, out.ctypes.data)
    if rc != 0:
        raise RoverError(f"rover_bf16_round failed ({rc}): {lib.rover_last_error(None).decode()}")
    return out


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _rows(t, cols, m):
    """(pointer, row stride in elements) of ``t`` [m, cols] as the C ABI takes them.  None -> (None, 0); at most one row -> ``cols`` (a
    one-row tensor's stride(0) means nothing); otherwise stride(0) as it is, the 0 of a row-expanded tensor included: the C layer refuses
    a stride where it is not allowed, the binding does not invent a dense one."""
    if t is None:
        return None, 0
    return t.data_ptr(), (t.stride(0) if m > 1 else cols)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device_index=None):
    """The current stream of the device as the void* the C ABI takes.  torch.cuda.current_stream() costs ~3 us of Python per call —
    a fifth of a small batch's step when a step makes three calls —, the raw accessor a tenth of that."""
    if _raw_stream is not None and device_index is not None:
        return C.c_void_p(_raw_stream(device_index))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


class Engine:
    """One rover_ctx: owns the device tables, launches the step kernels on torch's current stream."""

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
        rc = self.lib.rover_create(C.byref(self.cfg), C.byref(h))
        if rc != 0:
            raise RoverError(f"rover_create failed ({rc}): {self.lib.rover_last_error(None).decode()}")
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

    def _check(self, rc, what):
        if rc != 0:
            raise RoverError(f"{what} failed ({rc}): {self.lib.rover_last_error(self._h).decode()}")

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
        self._check(self.lib.rover_set_knn_map(self._h, which, idx.ctypes.data, x, y, k, tris.ctypes.data,
                                               tris.shape[0], verts.ctypes.data, verts.shape[0], cell_size,
                                               float(shift[0]), float(shift[1])), "rover_set_knn_map")

    def set_distribution(self, points, sparse_idx, dense_idx):
        self.generation += 1
        pts = _host(points, np.float64)
        sp = _host(sparse_idx, np.int64)
        de = _host(dense_idx, np.int64)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise RoverError("set_distribution: points must be [P,3]")
        self._check(self.lib.rover_set_distribution(self._h, pts.ctypes.data, pts.shape[0], sp.ctypes.data, len(sp),
                                                    de.ctypes.data, len(de)), "rover_set_distribution")
        self.P, self.Ns, self.Nd = pts.shape[0], len(sp), len(de)

    def set_heightfield(self, heightmap, horizontal_scale=0.025, vertical_scale=1.0, shift=(0.0, 0.0)):
        self.generation += 1
        hm = _host(heightmap, np.float32)
        self._check(self.lib.rover_set_heightfield(self._h, hm.ctypes.data, hm.shape[0], hm.shape[1],
                                                   horizontal_scale, vertical_scale, float(shift[0]), float(shift[1])),
                    "rover_set_heightfield")

    def set_stones(self, info7):
        self.generation += 1
        info = _host(info7, np.float32)
        if info.ndim != 2 or info.shape[1] != 7:
            raise RoverError("set_stones: expected [S,7] (read_stone_info output)")
        self._check(self.lib.rover_set_stones(self._h, info.ctypes.data, info.shape[0]), "rover_set_stones")

    def set_curriculum_level(self, level):
        self.generation += 1
        self._check(self.lib.rover_set_curriculum_level(self._h, int(level)), "rover_set_curriculum_level")

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
        self._check(self.lib.rover_get_info(self._h, C.byref(i)), "rover_get_info")
        return i

    def raycast_plan(self):
        """The ray-cast plan in force and the other host-side values that select a step's code path (rover_get_raycast_plan) as a
        plain dict of ints; host only, no launch, no synchronisation."""
        p = RaycastPlan()
        self._check(self.lib.rover_get_raycast_plan(self._h, C.byref(p)), "rover_get_raycast_plan")
        return {k: int(getattr(p, k)) for k, _ in RaycastPlan._fields_}

    def cull_info(self):
        """Diagnostics of the culled ray cast (rover_get_cull_info) as a dict; synchronises the device."""
        i = CullInfo()
        self._check(self.lib.rover_get_cull_info(self._h, C.byref(i)), "rover_get_cull_info")
        d = {k: (list(getattr(i, k)) if k in ("triangles", "always_candidate_triangles", "cells_without_cone", "cells_with_far_bound") else int(getattr(i, k)))
             for k, _ in CullInfo._fields_}
        d["pairs_per_ray"] = d["candidate_pairs"] / d["rays"] if d["rays"] else 0.0
        return d

    # ---- step ---------------------------------------------------------------------------------
    def _chk(self, t, shape, dtype, name):
        if t is None:
            return
        if not t.is_cuda or t.device != self.device:
            raise RoverError(f"{name}: expected a tensor on {self.device}, got {t.device}")
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise RoverError(f"{name}: expected contiguous {dtype} {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")

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
        self._chk(rew, (e,), f, "rew")
        self._chk(reset, (e,), i64, "reset")
        self._chk(rock_collision, (e,), i64, "rock_collision")
        self._chk(reset_ids, (e,), i64, "reset_ids")
        self._chk(n_reset, (1,), torch.int32, "n_reset")
        self._chk(euler, (e, 3), f, "euler")
        self._chk(heading_diff, (e,), f, "heading_diff")
        self._chk(ray_dist, (e, self.P), f, "ray_dist")
        self._chk(wheel_dist, (e, 24), f, "wheel_dist")
        self._chk(body_dist, (e, 2), f, "body_dist")
        self._chk(stone_collision, (e,), i64, "stone_collision")
        self._chk(done_u8, (e,), torch.uint8, "done_u8")
        self._chk(ray_src, (e, self.P, 3), f, "ray_src")
        self._chk(hit_pt, (e, self.P, 3), f, "hit_pt")
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
        flags = (STEP_INCREMENT_PROGRESS if increment_progress else 0) | (STEP_COMPACT if compact else 0)
        self._check(self.lib.rover_step(self._h, C.byref(sin), C.byref(sout), flags, _stream(self._dev_index)), "rover_step")

    def get_observations(self, sin, sout):
        self._check(self.lib.rover_get_observations(self._h, C.byref(sin), C.byref(sout), _stream(self._dev_index)),
                    "rover_get_observations")

    def calculate_metrics(self, sin, sout):
        self._check(self.lib.rover_calculate_metrics(self._h, C.byref(sin), C.byref(sout), _stream(self._dev_index)),
                    "rover_calculate_metrics")

    def is_done(self, sin, sout):
        self._check(self.lib.rover_is_done(self._h, C.byref(sin), C.byref(sout), _stream(self._dev_index)), "rover_is_done")

    def get_depths(self, positions, rotations):
        """Camera.get_depths (camera.py:60-145): positions [E,3], rotations [E,3] euler angles -> (distances [E,P], points [E,P,3],
        sources [E,P,3])."""
        e, f = self.num_envs, torch.float32
        self._chk(positions, (e, 3), f, "positions")
        self._chk(rotations, (e, 3), f, "rotations")
        dist = torch.empty(e, self.P, device=positions.device)
        pts = torch.empty(e, self.P, 3, device=positions.device)
        src = torch.empty(e, self.P, 3, device=positions.device)
        self._check(self.lib.rover_get_depths(self._h, _ptr(positions), _ptr(rotations), _ptr(dist), _ptr(pts), _ptr(src), _stream(self._dev_index)),
                    "rover_get_depths")
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
        self._check(self.lib.rover_get_collisions(self._h, _ptr(positions), _ptr(rotations), _ptr(joints), _ptr(wheel), _ptr(body),
                                                  _stream(self._dev_index)), "rover_get_collisions")
        return wheel, body

    def export_rays(self):
        """The rays of the last cast in slot order (24 wheel, 2 body, P heightmap rays per env): (src [E,R,3], dir [E,R,3] — the ray
        record's direction -normalize(direction) —, cell [E,R] int32, dist [E,R]), R = 26 + P."""
        e, r = self.num_envs, 26 + self.P
        src = torch.empty(e, r, 3, device=self.device)
        dirs = torch.empty(e, r, 3, device=self.device)
        cell = torch.empty(e, r, dtype=torch.int32, device=self.device)
        dist = torch.empty(e, r, device=self.device)
        self._check(self.lib.rover_export_rays(self._h, _ptr(src), _ptr(dirs), _ptr(cell), _ptr(dist), _stream(self._dev_index)), "rover_export_rays")
        return src, dirs, cell, dist

    def cast_rays(self, src, dirs):
        """Casts caller-supplied rays (layout of export_rays: origins, record directions) through the sort + ray-cast kernels."""
        e, r, f = self.num_envs, 26 + self.P, torch.float32
        self._chk(src, (e, r, 3), f, "src")
        self._chk(dirs, (e, r, 3), f, "dir")
        dist = torch.empty(e, r, device=self.device)
        self._check(self.lib.rover_cast_rays(self._h, _ptr(src), _ptr(dirs), _ptr(dist), _stream(self._dev_index)), "rover_cast_rays")
        return dist

    def compact_resets(self, reset, reset_ids, n_reset):
        self._chk(reset, (self.num_envs,), torch.int64, "reset")
        self._chk(reset_ids, (self.num_envs,), torch.int64, "reset_ids")
        self._chk(n_reset, (1,), torch.int32, "n_reset")
        self._check(self.lib.rover_compact_resets(self._h, _ptr(reset), _ptr(reset_ids), _ptr(n_reset), _stream(self._dev_index)),
                    "rover_compact_resets")

    def quat_to_euler(self, quat, out=None):
        n = quat.shape[0]
        self._chk(quat, (n, 4), torch.float32, "quat")
        out = torch.empty(n, 3, device=self.device) if out is None else out
        self._chk(out, (n, 3), torch.float32, "euler")
        self._check(self.lib.rover_quat_to_euler(self._h, _ptr(quat), _ptr(out), n, _stream(self._dev_index)), "rover_quat_to_euler")
        return out

    def build_knn_map(self, vertices, triangles, n_x, n_y, res=0.1, k=200, ranking="exact_f32", cell_x_f16=None, cell_y_f16=None):
        """rover_utils.py:48-123 on the GPU: -> map_indices [X, Y, K] int32 (device tensor), nearest first.
        ``ranking``: "exact_f32" (exact f32 squared distance, ties by id) or "reference_fp16" (the reference's fp16 distances,
        rover_utils.py:71-102; ``cell_*_f16`` = optional fp16 coordinate tables, see rover_build_knn_map_ref)."""
        v = _host(vertices, np.float32)
        t = _host(triangles, np.int32)
        if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
            raise RoverError("build_knn_map: expected vertices [V,3] and triangles [T,3]")
        out = torch.empty(int(n_x), int(n_y), int(k), dtype=torch.int32, device=self.device)
        if ranking == "exact_f32":
            self._check(self.lib.rover_build_knn_map(self._h, v.ctypes.data, v.shape[0], t.ctypes.data, t.shape[0], int(n_x), int(n_y),
                                                     float(res), int(k), _ptr(out)), "rover_build_knn_map")
            return out
        if ranking != "reference_fp16":
            raise RoverError(f"build_knn_map: unknown ranking {ranking!r}")
        tabs = []
        for tab, n in ((cell_x_f16, n_x), (cell_y_f16, n_y)):
            if tab is None:
                tabs.append(None)
                continue
            a = np.ascontiguousarray(np.asarray(tab, dtype=np.float16)).view(np.uint16)
            if a.shape != (int(n),):
                raise RoverError(f"build_knn_map: fp16 cell table must have {n} entries")
            tabs.append(a)
        self._check(self.lib.rover_build_knn_map_ref(self._h, v.ctypes.data, v.shape[0], t.ctypes.data, t.shape[0], int(n_x), int(n_y),
                                                     float(res), int(k), None if tabs[0] is None else tabs[0].ctypes.data,
                                                     None if tabs[1] is None else tabs[1].ctypes.data, _ptr(out)),
                    "rover_build_knn_map_ref")
        return out

    def build_heightfield(self, vertices, triangles, n0, n1, horizontal_scale=0.025, shift=(0.0, 0.0), fill=0.0):
        """rover_build_heightfield: for every node (i, j) of an ``n0`` x ``n1`` grid at ``horizontal_scale`` metres, node (0, 0) at
        ``shift``, the highest point of the mesh above it (the definition is in include/rover_step.h) -> (hm [n0, n1] float32 device
        tensor in metres, nodes no triangle covers — they hold ``fill`` —, triangles skipped).  ``vertices`` [V, 3] / ``triangles`` [T, 3]:
        anything numpy understands, or torch tensors; float32 / int32 contiguous tensors on this device are passed as they are."""
        def arg(a, np_dtype, t_dtype):
            if isinstance(a, torch.Tensor) and a.is_cuda and a.device == self.device and a.dtype == t_dtype and a.is_contiguous():
                return a, a.data_ptr(), tuple(a.shape)
            h = _host(a, np_dtype)
            return h, h.ctypes.data, h.shape
        v, v_ptr, v_shape = arg(vertices, np.float32, torch.float32)
        t, t_ptr, t_shape = arg(triangles, np.int32, torch.int32)
        if len(v_shape) != 2 or v_shape[1] != 3 or len(t_shape) != 2 or t_shape[1] != 3:
            raise RoverError("build_heightfield: expected vertices [V,3] and triangles [T,3]")
        n0, n1 = int(n0), int(n1)
        out = torch.empty(max(n0, 0), max(n1, 0), dtype=torch.float32, device=self.device) if max(n0, n1) <= 131072 else None
        stats = (C.c_int64 * 2)()
        self._check(self.lib.rover_build_heightfield(self._h, v_ptr if v_shape[0] else None, v_shape[0], t_ptr if t_shape[0] else None, t_shape[0],
                                                     n0, n1, float(horizontal_scale), float(shift[0]), float(shift[1]), float(fill),
                                                     _ptr(out) if out is not None and out.numel() else None, stats), "rover_build_heightfield")
        return out, int(stats[0]), int(stats[1])

    def mars_heightfield(self, plan, rock_mask=True):
        """rover_mars_heightfield: the heightfield of the reference's Mars terrain generator from ``plan`` — a ``terrain_gen.MarsPlan``, or a
        ``MarsDesc`` (mars_desc: any rectangle) -> (hf [rows, cols] float64 device tensor in metres, rock_mask uint8 device tensor: 1 where
        a kept stamp covers the node; None with ``rock_mask=False``).  The definition is in include/rover_step.h; synchronous."""
        desc, keep = (plan, None) if isinstance(plan, MarsDesc) else mars_plan_desc(plan)
        ok = 1 <= desc.rows <= MARS_MAX_SIDE and 1 <= desc.cols <= MARS_MAX_SIDE
        hf = torch.empty(desc.rows, desc.cols, dtype=torch.float64, device=self.device) if ok else None
        mask = torch.empty(desc.rows, desc.cols, dtype=torch.uint8, device=self.device) if ok and rock_mask else None
        self._check(self.lib.rover_mars_heightfield(self._h, C.byref(desc), _ptr(hf), _ptr(mask), _stream(self._dev_index)), "rover_mars_heightfield")
        del keep
        return hf, mask

    ACTIVATIONS = {"none": 0, None: 0, "leakyrelu": 1, "tanh": 2, "relu": 3, "elu": 4}

    @staticmethod
    def _f32_rows(t, name, what, shape=None):
        """``t`` must be a float32 GPU matrix with unit column stride (a column slice of a wider row-major tensor will do), of ``shape`` if given."""
        if t is None or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or (shape is not None and tuple(t.shape) != shape):
            raise RoverError(f"{what}: {name} must be a float32 GPU matrix{'' if shape is None else ' [%d,%d]' % shape} with unit column stride")
        return t

    def linear_forward(self, x, weight, bias, activation, out, precision="f32"):
        """out[:, :N] = act(x[:, :K] @ weight.T + bias); x / out may be column slices of wider row-major tensors.
        ``precision="bf16"``: x and weight rounded to bf16 as they are read, f32 accumulation, bias, activation and output
        (rover_linear_forward_bf16; the arithmetic is stated in rover_step.h)."""
        name = "rover_linear_forward" + _precision_suffix(precision)
        m, k = x.shape
        n = weight.shape[0]
        self._f32_rows(x, "x", "linear_forward")
        self._f32_rows(out, "out", "linear_forward")
        if k > 0:
            self._chk(weight, (n, k), torch.float32, "weight")
        self._chk(bias, (n,), torch.float32, "bias")
        if out.shape[0] != m or out.shape[1] != n:
            raise RoverError(f"linear_forward: out must be [{m},{n}]")
        self._check(getattr(self.lib, name)(self._h, *_rows(x, k, m), m, k, _ptr(weight), _ptr(bias), n,
                                            self.ACTIVATIONS[activation], *_rows(out, n, m), _stream(self._dev_index)), name)
        return out

    @staticmethod
    def chain_shape(layers):
        """(k0, widths, activations) of ``layers`` (objects with .weight [n, k], .activation): what the chain route queries take."""
        return layers[0].weight.shape[1], [l.weight.shape[0] for l in layers], [l.activation for l in layers]

    @classmethod
    def chain_fits(cls, layers):
        """True if ``layers`` can run as one rover_mlp_chain_forward launch — the library's answer: rover_mlp_chain_route names a kernel.
        Whether a chain fits does not depend on the number of rows (only which kernel runs it does): asked at one fixed row count."""
        return len(layers) > 0 and cls.chain_route(1, *cls.chain_shape(layers)) is not None

    def _chain(self, what, x, layers, out, keep, out_name="out"):
        """-> the ChainDesc of ``layers`` (objects with .weight [n, k], .bias [n], .activation) from x [m, k0] to out [m, n_last], all checked
        (errors under ``what``, the calling method's name).  The arrays it points at go into ``keep``: they live until the call returns."""
        m, k0 = x.shape
        self._f32_rows(x, "x", what)
        self._f32_rows(out, out_name, what)
        n, k = len(layers), k0
        for l in layers:
            self._chk(l.weight, (l.weight.shape[0], k), torch.float32, "weight")
            self._chk(l.bias, (l.weight.shape[0],), torch.float32, "bias")
            k = l.weight.shape[0]
        if out.shape[0] != m or out.shape[1] != k:
            raise RoverError(f"{what}: {out_name} must be [{m},{k}]")
        w = (C.c_void_p * n)(*[_ptr(l.weight) for l in layers])
        b = (C.c_void_p * n)(*[_ptr(l.bias) for l in layers])
        widths = (C.c_int32 * n)(*[l.weight.shape[0] for l in layers])
        acts = (C.c_int32 * n)(*[self.ACTIVATIONS[l.activation] for l in layers])
        keep.extend((w, b, widths, acts))
        return ChainDesc(*_rows(x, k0, m), k0, n, C.addressof(w), C.addressof(b), C.addressof(widths), C.addressof(acts), *_rows(out, k, m))

    def chain_forward(self, x, layers, out, precision="f32"):
        """out = layers[-1](... layers[0](x)) in one kernel; ``layers``: objects with .weight [n, k], .bias [n], .activation.
        ``precision="bf16"``: bf16 operands, f32 accumulation (rover_mlp_chain_forward_bf16; the arithmetic is stated in rover_step.h)."""
        name = "rover_mlp_chain_forward" + _precision_suffix(precision)
        keep = []
        d = self._chain("chain_forward", x, layers, out, keep)
        self._check(getattr(self.lib, name)(self._h, d.x, d.x_stride, x.shape[0], d.K0, d.n_layers, d.weights, d.biases, d.widths,
                                            d.activations, d.y, d.y_stride, _stream(self._dev_index)), name)
        return out

    def chain_pair_forward(self, xa, layers_a, out_a, xb, layers_b, out_b, copy_src=None, copy_dst=None, copy_cols=0):
        """Two 2-layer chains over the same rows (the two encoders: rover_mlp_chain_pair_forward) and, optionally,
        copy_dst[:, :copy_cols] = copy_src[:, :copy_cols] — side by side in one launch per stage at small batches."""
        if xa.shape[0] != xb.shape[0]:
            raise RoverError("chain_pair_forward: the two chains must have the same number of rows")
        keep = []
        da, db = self._chain("chain_pair_forward", xa, layers_a, out_a, keep), self._chain("chain_pair_forward", xb, layers_b, out_b, keep)
        if copy_cols:
            for t, name in ((copy_src, "copy_src"), (copy_dst, "copy_dst")):
                if self._f32_rows(t, name, "chain_pair_forward").shape[0] != xa.shape[0] or t.shape[1] < copy_cols:
                    raise RoverError(f"chain_pair_forward: {name} must have the same rows and >= copy_cols columns")
        copy = lambda t: _rows(t if copy_cols else None, int(copy_cols), xa.shape[0])
        self._check(self.lib.rover_mlp_chain_pair_forward(self._h, xa.shape[0], C.byref(da), C.byref(db), *copy(copy_src), *copy(copy_dst), int(copy_cols),
                                                          _stream(self._dev_index)), "rover_mlp_chain_pair_forward")

    # ---- the actor's Gaussian head (rover_gauss_head) --------------------------------------------------
    def _gauss_head(self, what, m, log_std, actions, log_prob, mean=None, taken_actions=None, step_dev=None, reduction="sum", **kw):
        """-> GaussHead over checked tensors (log_std [A]; actions [m, A]; log_prob [m, 1], or [m, A] with reduction None)."""
        a = int(log_std.numel())
        self._chk(log_std, (a,), torch.float32, "log_std")
        if reduction not in REDUCTIONS:
            raise RoverError(f"{what}: unknown reduction {reduction!r}")
        self._f32_rows(actions, "actions", what, (m, a))
        self._f32_rows(log_prob, "log_prob", what, (m, a if REDUCTIONS[reduction] == 5 else 1))
        if taken_actions is not None:
            self._f32_rows(taken_actions, "taken_actions", what, (m, a))
        if mean is not None:
            self._f32_rows(mean, "mean", what, (m, a))
        if step_dev is not None and (not step_dev.is_cuda or step_dev.dtype != torch.int64 or step_dev.numel() != 1):
            raise RoverError(f"{what}: step_dev must be one int64 word on the GPU (read as uint64)")
        dp = lambda t: None if t is None else t.data_ptr()
        (tp, ts), (ap, as_), (lp, ls), (mp, ms) = (_rows(t, cols, m) for t, cols in ((taken_actions, a), (actions, a), (log_prob, log_prob.shape[1]), (mean, a)))
        return gauss_head_desc(a, dp(log_std), ap, lp, reduction=reduction, step_dev=dp(step_dev), taken_actions=tp, taken_stride=ts, actions_stride=as_,
                               log_prob_stride=ls, mean=mp, mean_stride=ms, **kw)

    def chain_act(self, x, layers, mean_out, log_std, actions, log_prob, precision="f32", **head):
        """chain_forward with the Gaussian head on its output (rover_mlp_chain_act): ``mean_out`` receives what chain_forward writes,
        ``actions`` / ``log_prob`` the head's results.  ``head``: taken_actions, step_dev, reduction and the scalar fields of
        gauss_head_desc (seed, step, row_offset, deterministic, clip_*, ...).  ``precision="bf16"``: rover_mlp_chain_act_bf16 (the f32
        head on the bf16 chain's f32 mean)."""
        name = "rover_mlp_chain_act" + _precision_suffix(precision)
        keep = []
        d = self._chain("chain_act", x, layers, mean_out, keep, "mean_out")
        desc = self._gauss_head("chain_act", x.shape[0], log_std, actions, log_prob, **head)
        self._check(getattr(self.lib, name)(self._h, d.x, d.x_stride, x.shape[0], d.K0, d.n_layers, d.weights, d.biases, d.widths, d.activations,
                                            d.y, d.y_stride, C.byref(desc), _stream(self._dev_index)), name)
        return actions, log_prob

    def gaussian_head(self, mean, log_std, actions, log_prob, **head):
        """The head on a given ``mean`` [m, A], A <= 16 (rover_gaussian_head): one launch."""
        self._f32_rows(mean, "mean", "gaussian_head")
        desc = self._gauss_head("gaussian_head", mean.shape[0], log_std, actions, log_prob, mean=mean, **head)
        self._check(self.lib.rover_gaussian_head(self._h, mean.shape[0], C.byref(desc), _stream(self._dev_index)), "rover_gaussian_head")
        return actions, log_prob

    def policy_noise(self, m, a, seed=0, step=0, step_dev=None, row_offset=0, out=None):
        """eps [m, a] as the head draws it for (seed, step + *step_dev, row_offset) (rover_policy_noise)."""
        if out is None:
            out = torch.empty(int(m), int(a), device=self.device)
        self._f32_rows(out, "out", "policy_noise", (int(m), int(a)))
        self._check(self.lib.rover_policy_noise(self._h, int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), _ptr(step_dev), int(row_offset), int(m),
                                                int(a), *_rows(out, int(a), int(m)), _stream(self._dev_index)), "rover_policy_noise")
        return out

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
        self._check(self.lib.rover_obs_noise(self._h, C.byref(desc), _stream(self._dev_index)), "rover_obs_noise")
        return out

    def configure_occlusion(self, camera=(0.0, 0.0, 0.7), step=0.05, clearance=0.03, max_steps=256, miss=5.0):
        """The line-of-sight stage's configuration (rover_set_occlusion): needs set_distribution and set_heightfield, derives the column
        order and the tile-max table of the heightfield, and has to be called again after either of the two is set again."""
        cfg = occlusion_cfg(camera, step, clearance, max_steps, miss)
        self._check(self.lib.rover_set_occlusion(self._h, C.byref(cfg)), "rover_set_occlusion")

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
        self._check(self.lib.rover_obs_occlusion(self._h, C.byref(desc), _stream(self._dev_index)), "rover_obs_occlusion")
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
        self._check(self.lib.rover_scaler_update(self._h, C.byref(desc), _stream(self._dev_index)), "rover_scaler_update")

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
        self._check(self.lib.rover_scaler_apply(self._h, C.byref(desc), _stream(self._dev_index)), "rover_scaler_apply")
        return out

    def motion_step(self, pos, quat, lin, ang, *, dt, substeps=1, max_lin=1.0, max_ang=1.0, ride_height=0.3, joints=None,
                    suspension="plane", iters=4, max_bogie=0.6):
        """``substeps`` sub-steps of length ``dt`` of the terrain-following motion model on ``pos`` [e, 3] and ``quat`` [e, 4] (w, x, y, z),
        IN PLACE (rover_motion_step, one launch; needs set_heightfield): the commands ``lin`` / ``ang`` [e] scaled by ``max_lin`` /
        ``max_ang`` move the body, the six wheel contacts' terrain heights give z, roll and pitch.  ``lin`` and ``ang`` may be one column
        of a wider matrix (``tracker[:, 0]``): their common stride is passed on.  ``joints``: None, or (joint_pos_targets, joint_vel_targets,
        joint_pos, joint_vel), each [e, 13] — after the last sub-step the state becomes the targets.
        ``suspension="bogie"`` (rover_motion_step_bogie) solves the rocker-bogie posture instead of fitting a plane: ``iters`` chord
        iterations put all six wheels on the ground, and the three passive joint angles, clamped to +-``max_bogie`` rad, go to columns
        0-2 of joint_pos.  ``iters`` and ``max_bogie`` are not read with ``suspension="plane"``."""
        what = "motion_step"
        if suspension not in SUSPENSIONS:
            raise RoverError(f"{what}: suspension must be one of {SUSPENSIONS}, not {suspension!r}")
        e = pos.shape[0] if pos is not None and pos.dim() == 2 else -1
        self._chk(pos, (e, 3), torch.float32, "pos")
        self._chk(quat, (e, 4), torch.float32, "quat")
        if pos is None or quat is None or e < 0:
            raise RoverError(f"{what}: pos [e, 3] and quat [e, 4] must be given")
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
        desc = motion_desc(e, pos.data_ptr(), quat.data_ptr(), lin.data_ptr(), ang.data_ptr(), stride, substeps, dt, max_lin, max_ang, ride_height, *jp)
        if suspension == "bogie":
            par = BogieParams(int(iters), float(max_bogie))
            self._check(self.lib.rover_motion_step_bogie(self._h, C.byref(desc), C.byref(par), _stream(self._dev_index)), "rover_motion_step_bogie")
            return
        self._check(self.lib.rover_motion_step(self._h, C.byref(desc), _stream(self._dev_index)), "rover_motion_step")

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
        self._check(self.lib.rover_episode_track(self._h, C.byref(desc), _stream(self._dev_index)), "rover_episode_track")
        return desc

    chain_act_route = staticmethod(chain_act_route)
    bf16_round = staticmethod(bf16_round)

    # ---- the student's recurrent block (rover_gru_cell, rover_gated_sum) -------------------------------------
    def gru_cell(self, x, h_in, w_ih, w_hh, b_ih, b_hh, h_out, reset_mask=None, precision="f32"):
        """One layer of torch.nn.GRU for one time step (rover_gru_cell): h_out = cell(x [m, k], h_in [m, h]); w_ih [3h, k], w_hh [3h, h],
        b_ih / b_hh [3h] or None.  x, h_in and h_out may be column slices / padded rows; ``reset_mask``: optional [m] bool / uint8 —
        marked rows read h_in as zero.  h_out must not overlap h_in (the library refuses it).  ``precision="bf16"``: the operands of the
        matrix products rounded to bf16 as they are read; gates, blend and h_out in f32 on the unrounded h_in (rover_gru_cell_bf16)."""
        name = "rover_gru_cell" + _precision_suffix(precision)
        what = name[len("rover_"):]
        self._f32_rows(x, "x", what)
        m, k = x.shape
        hd = w_hh.shape[1] if w_hh is not None and w_hh.dim() == 2 else -1
        self._f32_rows(h_in, "h_in", what, (m, hd))
        self._f32_rows(h_out, "h_out", what, (m, hd))
        if k > 0:
            self._chk(w_ih, (3 * hd, k), torch.float32, "w_ih")
        self._chk(w_hh, (3 * hd, hd), torch.float32, "w_hh")
        self._chk(b_ih, (3 * hd,), torch.float32, "b_ih")
        self._chk(b_hh, (3 * hd,), torch.float32, "b_hh")
        reset_mask = self._mask(reset_mask, m)
        self._check(getattr(self.lib, name)(self._h, *_rows(x, k, m), *_rows(h_in, hd, m), m, k, hd, _ptr(w_ih) if k > 0 else None, _ptr(w_hh), _ptr(b_ih),
                                            _ptr(b_hh), _ptr(reset_mask), *_rows(h_out, hd, m), _stream(self._dev_index)), name)
        return h_out

    @classmethod
    def gru_cell_route(cls, m, k, h, precision="f32"):
        """The instantiation gru_cell runs for [m, k] inputs and a hidden width h ("gru_cell<4>", "gru_cell<1>"; ``precision="bf16"``:
        "gru_cell_bf16<128,64>"); "none" for m = 0, None where the call would be refused.  Host only."""
        return cls._route(getattr(load(), "rover_gru_cell_route" + _precision_suffix(precision))(int(m), int(k), int(h)))

    def gru_cell_train(self, x, h_in, w_ih, w_hh, b_ih, b_hh, h_out, gates, reset_mask=None):
        """gru_cell that also stores ``gates`` [m, 4h] = r | z | n | q for gru_cell_backward (rover_gru_cell_train); h_out has gru_cell's bits."""
        what = "gru_cell_train"
        self._f32_rows(x, "x", what)
        m, k = x.shape
        hd = w_hh.shape[1] if w_hh is not None and w_hh.dim() == 2 else -1
        self._f32_rows(h_in, "h_in", what, (m, hd))
        self._f32_rows(h_out, "h_out", what, (m, hd))
        self._f32_rows(gates, "gates", what, (m, 4 * hd))
        if k > 0:
            self._chk(w_ih, (3 * hd, k), torch.float32, "w_ih")
        self._chk(w_hh, (3 * hd, hd), torch.float32, "w_hh")
        self._chk(b_ih, (3 * hd,), torch.float32, "b_ih")
        self._chk(b_hh, (3 * hd,), torch.float32, "b_hh")
        reset_mask = self._mask(reset_mask, m)
        self._check(self.lib.rover_gru_cell_train(self._h, *_rows(x, k, m), *_rows(h_in, hd, m), m, k, hd, _ptr(w_ih) if k > 0 else None, _ptr(w_hh),
                                                  _ptr(b_ih), _ptr(b_hh), _ptr(reset_mask), *_rows(h_out, hd, m), *_rows(gates, 4 * hd, m),
                                                  _stream(self._dev_index)), "rover_gru_cell_train")
        return h_out

    def _mask(self, reset_mask, m):
        """an optional [m] bool / uint8 reset mask as the uint8 tensor the C ABI reads"""
        if reset_mask is not None:
            if reset_mask.dtype == torch.bool:
                reset_mask = reset_mask.view(torch.uint8)
            self._chk(reset_mask, (m,), torch.uint8, "reset_mask")
        return reset_mask

    def gru_cell_backward(self, dh_above, dh_next, gates, h_in, w_hh, dgi, dgh, dh_in, reset_mask=None):
        """rover_gru_cell_backward: one layer, one time step, one launch.  dh_above / dh_next (or None) / h_in / dh_in [m, h], gates
        [m, 4h] as gru_cell_train stored them, dgi / dgh [m, 3h]; all float32 rows with unit column stride (slices will do)."""
        what = "gru_cell_backward"
        hd = w_hh.shape[1] if w_hh is not None and w_hh.dim() == 2 else -1
        m = self._f32_rows(dh_above, "dh_above", what).shape[0]
        for t, name, cols in ((dh_above, "dh_above", hd), (gates, "gates", 4 * hd), (h_in, "h_in", hd), (dgi, "dgi", 3 * hd), (dgh, "dgh", 3 * hd),
                              (dh_in, "dh_in", hd)) + (() if dh_next is None else ((dh_next, "dh_next", hd),)):
            self._f32_rows(t, name, what, (m, cols))
        self._chk(w_hh, (3 * hd, hd), torch.float32, "w_hh")
        reset_mask = self._mask(reset_mask, m)
        self._check(self.lib.rover_gru_cell_backward(self._h, *_rows(dh_above, hd, m), *_rows(dh_next, hd, m), *_rows(gates, 4 * hd, m), *_rows(h_in, hd, m),
                                                     _ptr(reset_mask), _ptr(w_hh), m, hd, *_rows(dgi, 3 * hd, m), *_rows(dgh, 3 * hd, m),
                                                     *_rows(dh_in, hd, m), _stream(self._dev_index)), "rover_gru_cell_backward")
        return dh_in

    @classmethod
    def gru_cell_backward_route(cls, m, h):
        """The instantiation gru_cell_backward runs ("gru_bwd<4>", "gru_bwd<1>"); "none" for m = 0, None where refused.  Host only."""
        return cls._route(load().rover_gru_cell_backward_route(int(m), int(h)))

    def gated_sum_backward(self, d_out, mul, pre, d_mul=None, d_pre=None):
        """rover_gated_sum_backward: d_mul = d_out * sigmoid(pre), d_pre = (d_out * mul) * s (1 - s) over [m, n]; each output optional.
        mul / pre may be one row expanded over the rows (row stride 0); the outputs are per row."""
        what = "gated_sum_backward"
        m, n = self._f32_rows(d_out, "d_out", what).shape
        self._f32_rows(pre, "pre", what, (m, n))
        for t, name in ((mul, "mul"), (d_mul, "d_mul"), (d_pre, "d_pre")):
            if t is not None:
                self._f32_rows(t, name, what, (m, n))
        if d_pre is not None and mul is None:
            raise RoverError(f"{what}: d_pre needs mul")
        self._check(self.lib.rover_gated_sum_backward(self._h, *_rows(d_out, n, m), *_rows(mul, n, m), *_rows(pre, n, m), m, n, *_rows(d_mul, n, m),
                                                      *_rows(d_pre, n, m), _stream(self._dev_index)), "rover_gated_sum_backward")

    def linear_dgrad(self, y, dy, weight, activation, dx):
        """rover_linear_dgrad: dx = (dy * act'(y)) @ weight for any widths; ``y`` may be None with activation None.  Enqueues only."""
        what = "linear_dgrad"
        n, k = weight.shape
        m = self._f32_rows(dy, "dy", what).shape[0]
        if dy.shape[1] != n:
            raise RoverError(f"{what}: dy must be [{m},{n}]")
        if y is not None or self.ACTIVATIONS[activation] != 0:
            self._f32_rows(y, "y", what, (m, n))
        self._chk(weight, (n, k), torch.float32, "weight")
        self._f32_rows(dx, "dx", what, (m, k))
        self._check(self.lib.rover_linear_dgrad(self._h, *_rows(y, n, m), *_rows(dy, n, m), m, k, _ptr(weight), n, self.ACTIVATIONS[activation],
                                                *_rows(dx, k, m), _stream(self._dev_index)), "rover_linear_dgrad")
        return dx

    @classmethod
    def linear_dgrad_route(cls, m, k, n):
        """What linear_dgrad launches ("dgrad<1,1>x10", ...); "none" for m = 0, None where the call would be refused.  Host only."""
        return cls._route(load().rover_linear_dgrad_route(int(m), int(k), int(n)))

    def gated_sum(self, add, mul, pre, out):
        """out = add + mul * sigmoid(pre) over [m, n] (rover_gated_sum), one launch.  All four are float32 GPU matrices with unit column
        stride; an input may be a one-row matrix expanded over the rows (row stride 0)."""
        what = "gated_sum"
        self._f32_rows(out, "out", what)
        m, n = out.shape
        for t, name in ((add, "add"), (mul, "mul"), (pre, "pre")):
            self._f32_rows(t, name, what, (m, n))
        self._check(self.lib.rover_gated_sum(self._h, *_rows(add, n, m), *_rows(mul, n, m), *_rows(pre, n, m), m, n, *_rows(out, n, m),
                                             _stream(self._dev_index)), "rover_gated_sum")
        return out

    # ---- the rollout side of PPO (rover_gae) -------------------------------------------------------------
    def _gae_rows(self, t, name, dtype, T=None, E=None):
        """``t`` must be a [T, E] or skrl-shaped [T, E, 1] GPU tensor of ``dtype`` with unit env stride (a padded buffer's view will do)
        -> (pointer, time stride in elements, T, E)."""
        ok = t is not None and t.is_cuda and t.device == self.device and t.dtype == dtype and (t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 1))
        if ok:
            sh = (int(t.shape[0]), int(t.shape[1]))
            ok = (sh[1] <= 1 or t.stride(1) == 1) and (T is None or sh == (T, E)) and (sh[0] <= 1 or t.stride(0) >= sh[1])
        if not ok:
            raise RoverError(f"gae: {name} must be a {dtype} tensor{'' if T is None else ' [%d,%d] or [%d,%d,1]' % (T, E, T, E)} on {self.device} "
                             "with unit env stride and a time stride >= E")
        return (*_rows(t, sh[1], sh[0]), sh[0], sh[1])

    def _gae_stats(self, t, name):
        if t is not None and (not t.is_cuda or t.device != self.device or t.dtype != torch.float64 or t.numel() != 3 or not t.is_contiguous()):
            raise RoverError(f"gae: {name} must be 3 contiguous float64 words (count, mean, M2) on {self.device}")
        return None if t is None else t.data_ptr()

    def gae(self, rewards, values, dones, last_values, returns, advantages, gamma=0.99, lam=0.95, normalize=True, stats_out=None, stats_in=None):
        """rover_gae: returns and advantages of a stored rollout in one pass.  rewards / values / returns / advantages: float32 [T, E] or
        [T, E, 1]; dones: torch.bool or uint8 of that shape; last_values: float32 [E] or [E, 1], contiguous.  Time strides are taken from
        the tensors (padded buffers and skrl-shaped storage work in place); ``returns`` may be ``values``.  ``normalize``: False = raw A,
        True = (A - mean) / (std + 1e-8) with this call's own moments — or, when ``stats_in`` (3 float64 on the device) is given, with
        those.  ``stats_out`` (3 float64 on the device) receives (count, mean, M2) of this call's raw A.  Enqueues only."""
        rp, rs, T, E = self._gae_rows(rewards, "rewards", torch.float32)
        vp, vs, _, _ = self._gae_rows(values, "values", torch.float32, T, E)
        if dones is not None and dones.dtype == torch.bool:
            dones = dones.view(torch.uint8)
        dp, ds, _, _ = self._gae_rows(dones, "dones", torch.uint8, T, E)
        op, os_, _, _ = self._gae_rows(returns, "returns", torch.float32, T, E)
        ap, as_, _, _ = self._gae_rows(advantages, "advantages", torch.float32, T, E)
        if last_values is None or tuple(last_values.shape) not in ((E,), (E, 1)):
            raise RoverError(f"gae: last_values must be [{E}] or [{E},1]")
        self._chk(last_values, tuple(last_values.shape), torch.float32, "last_values")
        if stats_in is not None and not normalize:
            raise RoverError("gae: stats_in is only read when normalize is set")
        mode = GAE_RAW if not normalize else (GAE_NORMALIZE if stats_in is None else GAE_NORMALIZE_GIVEN)
        d = GaeDesc(T, E, float(gamma), float(lam), rp, rs, vp, vs, dp, ds, last_values.data_ptr(), op, os_, ap, as_, mode,
                    self._gae_stats(stats_out, "stats_out"), self._gae_stats(stats_in, "stats_in"))
        self._check(self.lib.rover_gae(self._h, C.byref(d), _stream(self._dev_index)), "rover_gae")
        return returns, advantages

    # ---- the learner side of PPO (rover_linear_backward, rover_ppo_loss) ---------------------------------
    def linear_backward(self, x, y, dy, weight, activation, dx=None, dweight=None, dbias=None):
        """rover_linear_backward: the backward of ``y = act(x @ weight.T + bias)``.  ``y`` is the layer's output as linear_forward wrote
        it, ``dy`` the gradient at it; x / y / dy / dx may be column slices of wider row-major tensors; ``dweight`` [n, k] and ``dbias``
        [n] are contiguous.  Each output is optional (None: not computed); ``x`` may be None without ``dweight``, ``y`` with activation None.
        Enqueues only."""
        what = "linear_backward"
        n, k = weight.shape
        m = self._f32_rows(dy, "dy", what).shape[0]
        if dy.shape[1] != n:
            raise RoverError(f"{what}: dy must be [{m},{n}]")
        if y is not None or self.ACTIVATIONS[activation] != 0:        # without an activation the derivative needs no y
            self._f32_rows(y, "y", what, (m, n))
        if k > 0:
            self._chk(weight, (n, k), torch.float32, "weight")
        if x is not None:
            self._f32_rows(x, "x", what, (m, k))
        elif dweight is not None and k > 0:
            raise RoverError(f"{what}: dweight needs x")
        if dx is not None:
            self._f32_rows(dx, "dx", what, (m, k))
        if dweight is not None and k > 0:
            self._chk(dweight, (n, k), torch.float32, "dweight")
        if dbias is not None:
            self._chk(dbias, (n,), torch.float32, "dbias")
        self._check(self.lib.rover_linear_backward(self._h, *_rows(x, k, m), *_rows(y, n, m), *_rows(dy, n, m), m, k, _ptr(weight), n,
                                                   self.ACTIVATIONS[activation], *_rows(dx, k, m), _ptr(dweight), _ptr(dbias),
                                                   _stream(self._dev_index)), "rover_linear_backward")

    def ppo_loss(self, mean, log_std, actions, old_log_prob, advantages, value, old_values, returns, d_mean, d_value, d_log_std, stats,
                 ratio_clip=0.2, value_clip=0.2, clip_predicted_values=True, entropy_loss_scale=0.0, value_loss_scale=1.0, clip_log_std=True,
                 min_log_std=-20.0, max_log_std=2.0, reduction="sum"):
        """rover_ppo_loss: the PPO minibatch loss at the nets' outputs and its gradients.  mean / actions / d_mean: float32 [m, A] (column
        slices will do); the per-row arrays float32 [m] or [m, 1], contiguous; log_std / d_log_std [A]; ``stats``: 4 float64 on the
        device, receives (policy_loss, value_loss, entropy_loss, kl).  Enqueues only; capturable."""
        what = "ppo_loss"
        m, a = self._f32_rows(mean, "mean", what).shape
        self._f32_rows(actions, "actions", what, (m, a))
        self._f32_rows(d_mean, "d_mean", what, (m, a))
        for t, name in ((old_log_prob, "old_log_prob"), (advantages, "advantages"), (value, "value"), (old_values, "old_values"), (returns, "returns"),
                        (d_value, "d_value")):
            if t is None or tuple(t.shape) not in ((m,), (m, 1)):
                raise RoverError(f"{what}: {name} must be [{m}] or [{m},1]")
            self._chk(t, tuple(t.shape), torch.float32, name)
        self._chk(log_std, (a,), torch.float32, "log_std")
        self._chk(d_log_std, (a,), torch.float32, "d_log_std")
        if stats is None or not stats.is_cuda or stats.dtype != torch.float64 or stats.numel() != 4 or not stats.is_contiguous():
            raise RoverError(f"{what}: stats must be 4 contiguous float64 words on the GPU")
        if reduction not in REDUCTIONS:
            raise RoverError(f"{what}: unknown reduction {reduction!r}")
        d = PpoLossDesc(m, a, *_rows(mean, a, m), log_std.data_ptr(), *_rows(actions, a, m),
                        old_log_prob.data_ptr(), advantages.data_ptr(), value.data_ptr(), old_values.data_ptr(), returns.data_ptr(),
                        int(bool(clip_log_std)), float(min_log_std), float(max_log_std), REDUCTIONS[reduction], float(ratio_clip), float(value_clip),
                        int(bool(clip_predicted_values)), float(entropy_loss_scale), float(value_loss_scale), *_rows(d_mean, a, m), d_value.data_ptr(), d_log_std.data_ptr(), stats.data_ptr())
        self._check(self.lib.rover_ppo_loss(self._h, C.byref(d), _stream(self._dev_index)), "rover_ppo_loss")
        return stats

    # ---- the optimiser step (rover_optim_*) ---------------------------------------------------------------
    @classmethod
    def optim_plan(cls, numel):
        """rover_optim_plan: the chunks the optimiser kernels walk for tensors of ``numel`` elements -> [(tensor, first, length)], in
        tensor order then element order.  Host only: no ctx, no device.  The chunk length is the library's constant: read it off the
        plan of one long tensor."""
        sizes = [int(v) for v in numel]
        arr = (C.c_int64 * max(len(sizes), 1))(*sizes)
        lib, n = load(), C.c_int64(0)
        rc = lib.rover_optim_plan(len(sizes), arr, None, 0, C.byref(n))
        if rc == 0:
            chunks = (OptimChunk * max(n.value, 1))()
            rc = lib.rover_optim_plan(len(sizes), arr, chunks, n.value, C.byref(n))
        if rc != 0:
            raise RoverError(f"rover_optim_plan failed ({rc}): {lib.rover_last_error(None).decode()}")
        return [(int(c.tensor), int(c.first), int(c.length)) for c in chunks[:n.value]]

    def _optim_word(self, t, name, dtype, what):
        if t is None or not t.is_cuda or t.device != self.device or t.dtype != dtype or t.numel() != 1:
            raise RoverError(f"{what}: {name} must be one {dtype} word on {self.device}")
        return t.data_ptr()

    def optim_create(self, params, grads, exp_avg, exp_avg_sq, step, stopped):
        """rover_optim_create: binds contiguous float32 ``params`` and their ``grads`` (two lists of GPU tensors, pairwise of one shape;
        empty tensors are allowed) to the caller's state — ``exp_avg`` / ``exp_avg_sq``: flat float32 of sum(numel) elements in tensor
        order, zeroed; ``step``: one int64; ``stopped``: one int32 — and returns the handle.  Every tensor must stay alive, and stay
        the same storage, as long as the handle is used."""
        what = "optim_create"
        params, grads = list(params), list(grads)
        if len(params) != len(grads):
            raise RoverError(f"{what}: {len(params)} params but {len(grads)} grads")
        for i, (p, g) in enumerate(zip(params, grads)):
            self._chk(p, tuple(p.shape), torch.float32, f"params[{i}]")
            self._chk(g, tuple(p.shape), torch.float32, f"grads[{i}]")
        n = len(params)
        numel = [p.numel() for p in params]
        total = sum(numel)
        self._chk(exp_avg, (total,), torch.float32, "exp_avg")
        self._chk(exp_avg_sq, (total,), torch.float32, "exp_avg_sq")
        ptrs = lambda ts: (C.c_void_p * max(n, 1))(*[t.data_ptr() if t.numel() else None for t in ts])
        pa, ga, na = ptrs(params), ptrs(grads), (C.c_int64 * max(n, 1))(*numel)
        d = OptimDesc(n, C.cast(pa, C.c_void_p), C.cast(ga, C.c_void_p), C.cast(na, C.c_void_p), exp_avg.data_ptr() if total else None,
                      exp_avg_sq.data_ptr() if total else None, self._optim_word(step, "step", torch.int64, what),
                      self._optim_word(stopped, "stopped", torch.int32, what))
        h = C.c_int32(-1)
        self._check(self.lib.rover_optim_create(self._h, C.byref(d), C.byref(h)), "rover_optim_create")
        return int(h.value)

    def optim_destroy(self, handle):
        self._check(self.lib.rover_optim_destroy(self._h, int(handle)), "rover_optim_destroy")

    def optim_step(self, handle, lr, beta1=0.9, beta2=0.999, eps=1e-8, grad_norm_clip=0.0, gate=None, gate_threshold=0.0, norm_out=None):
        """rover_optim_step: clip_grad_norm_ (``grad_norm_clip`` <= 0: none) and one Adam step over the handle's tensors in two launches.
        ``gate`` (one float64 on the device, e.g. ``stats[3:]`` of ppo_loss): the step is skipped, and the handle's ``stopped`` latch
        set, when the latch is set already or ``gate > gate_threshold``.  ``norm_out`` (one float64 on the device) receives the
        gradient norm before clipping.  Enqueues only; capturable."""
        what = "optim_step"
        d = OptimStepDesc(float(lr), float(beta1), float(beta2), float(eps), float(grad_norm_clip),
                          None if gate is None else self._optim_word(gate, "gate", torch.float64, what), float(gate_threshold),
                          None if norm_out is None else self._optim_word(norm_out, "norm_out", torch.float64, what))
        self._check(self.lib.rover_optim_step(self._h, int(handle), C.byref(d), _stream(self._dev_index)), "rover_optim_step")

    @classmethod
    def linear_backward_route(cls, m, k, n, want_dx):
        """What linear_backward launches ("wgrad<3,4>/64;dgrad<1,4>", ...: the weight-gradient instantiation and its M-split, then the
        dx kernel); "zero" for m = 0, None where the call would be refused."""
        return cls._route(load().rover_linear_backward_route(int(m), int(k), int(n), int(bool(want_dx))))

    # ---- which kernel a forward call runs (host only: no ctx, no launch) ----------------------------
    @staticmethod
    def _route(name):
        return None if name is None else name.decode()

    @classmethod
    def _chain_shape(cls, k0, widths, activations):
        n = len(widths)
        if len(activations) != n:
            raise RoverError("chain route: one activation per layer")
        return (int(k0), n, (C.c_int32 * n)(*[int(w) for w in widths]),
                (C.c_int32 * n)(*[a if isinstance(a, int) else cls.ACTIVATIONS[a] for a in activations]))

    @classmethod
    def linear_route(cls, m, k, n, precision="f32"):
        """The instantiation linear_forward runs for an [m, k] x [n, k]^T layer ("linear_act<3,4>x2", ...; ``precision="bf16"``:
        "linear_bf16<128,128>"); "none" for m = 0, None where the call would be refused."""
        return cls._route(getattr(load(), "rover_linear_route" + _precision_suffix(precision))(int(m), int(k), int(n)))

    @classmethod
    def chain_route(cls, m, k0, widths, activations, precision="f32"):
        """The kernel chain_forward runs ("splitk<6,2>", "mlp_small", "chain16<16,10,8,1>", ...; ``precision="bf16"``:
        "chain_bf16<5,4,0,0>", ...); activations: names or codes."""
        k0, n, w, a = cls._chain_shape(k0, widths, activations)
        return cls._route(getattr(load(), "rover_mlp_chain_route" + _precision_suffix(precision))(int(m), k0, n, w, a))

    @classmethod
    def chain_pair_route(cls, m, a, b):
        """The launches of chain_pair_forward: "pair(splitk<TN,RT>)" or "seq(<a>;<b>)"; a, b = (k0, widths, activations)."""
        descs = []
        for k0, widths, acts in (a, b):
            k0, n, w, ac = cls._chain_shape(k0, widths, acts)
            descs.append((ChainDesc(None, k0, k0, n, None, None, C.addressof(w), C.addressof(ac), None, 0), w, ac))
        return cls._route(load().rover_mlp_chain_pair_route(int(m), C.byref(descs[0][0]), C.byref(descs[1][0])))

    # ---- evaluation mode (rover.py:122-137, 620-641, 670-672) -------------------------------------
    def set_evaluation(self, enable=True):
        """Turns the per-env outcome latch on (fresh zeroed codes and steps, synchronises) or off (frees them)."""
        self.generation += 1
        self._check(self.lib.rover_set_evaluation(self._h, 1 if enable else 0), "rover_set_evaluation")

    def eval_clear(self, env_ids=None):
        """Re-arms the given LOCAL env ids (int64 device tensor), or every env: code 0, step 0.  With ids the call synchronises."""
        self.generation += 1
        n = 0
        if env_ids is not None:
            n = env_ids.shape[0]
            self._chk(env_ids, (n,), torch.int64, "env_ids")
        self._check(self.lib.rover_eval_clear(self._h, _ptr(env_ids), n, _stream(self._dev_index)), "rover_eval_clear")

    def eval_read(self, eval_res=None, eval_step=None, summary8=None):
        """Enqueues copies of the codes [E], the latch steps [E] and / or the summary [8] (counts of codes 0..3, sums of the steps
        over codes 0..3) into the given int64 device tensors; no host sync."""
        e = self.num_envs
        self._chk(eval_res, (e,), torch.int64, "eval_res")
        self._chk(eval_step, (e,), torch.int64, "eval_step")
        self._chk(summary8, (8,), torch.int64, "summary8")
        self._check(self.lib.rover_eval_read(self._h, _ptr(eval_res), _ptr(eval_step), _ptr(summary8), _stream(self._dev_index)),
                    "rover_eval_read")

    def set_option(self, name, value):
        self.generation += 1
        self._check(self.lib.rover_set_option(self._h, name.encode(), int(value)), "rover_set_option")

    def set_profiling(self, enable=True, every=1):
        """Bracket the ray-cast launch of every `every`-th step with hipEvents (get_profile() sums them)."""
        self.generation += 1
        self._check(self.lib.rover_set_profiling(self._h, max(1, int(every)) if enable else 0), "rover_set_profiling")

    def get_profile(self):
        p = Profile()
        self._check(self.lib.rover_get_profile(self._h, C.byref(p)), "rover_get_profile")
        return p

    def replay_raycast(self, stream=None):
        s = _stream(self._dev_index) if stream is None else C.c_void_p(stream)
        self._check(self.lib.rover_replay_raycast(self._h, s), "rover_replay_raycast")

    # ---- reset path ----------------------------------------------------------------------------
    def clearance(self, xy):
        n = xy.shape[0]
        self._chk(xy, (n, 2), torch.float32, "xy")
        out = torch.empty(n, device=self.device)
        self._check(self.lib.rover_clearance(self._h, _ptr(xy), n, _ptr(out), _stream(self._dev_index)), "rover_clearance")
        return out

    def shift_spawns(self, pos3, max_iter=100000):
        n = pos3.shape[0]
        self._chk(pos3, (n, 3), torch.float32, "pos3")
        self._check(self.lib.rover_shift_spawns(self._h, _ptr(pos3), n, int(max_iter), _stream(self._dev_index)), "rover_shift_spawns")
        return pos3

    def sample_height(self, xy):
        n = xy.shape[0]
        self._chk(xy, (n, 2), torch.float32, "xy")
        out = torch.empty(n, device=self.device)
        self._check(self.lib.rover_sample_height(self._h, _ptr(xy), n, _ptr(out), _stream(self._dev_index)), "rover_sample_height")
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
        self._check(self.lib.rover_generate_goals(self._h, _ptr(env_ids), n, _ptr(initial_pos3), _ptr(target3),
                                                  float(radius), _ptr(draws), int(max_draws), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                  _ptr(n_draws_used), _stream(self._dev_index)), "rover_generate_goals")

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
        io = self._reset_io(*args, **kw)
        self._check(self.lib.rover_reset_envs(self._h, C.byref(io), _stream(self._dev_index)), "rover_reset_envs")

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
        self._check(self.lib.rover_ackermann(self._h, _ptr(lin), _ptr(ang), n, _ptr(steer), _ptr(vel), _stream(self._dev_index)),
                    "rover_ackermann")
        return steer, vel
