"""The C ABI of librover_step.so as ctypes sees it (include/rover_step.h): constants, struct mirrors, the symbol table, the loader and the
two checked call paths.  ``_core``, ``_scene``, ``_sim`` and ``_learn`` hold the entry points of one C unit each; ``_lib`` is the public face."""
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
    _fields_ = [("num_envs", C.c_int32), ("num_envs_global", C.c_int32), ("env_offset", C.c_int32), ("device", C.c_int32),
                ("curriculum_level", C.c_int32), ("max_episode_length", C.c_int32), ("pos_reward", C.c_float), ("heading_contraint_reward", C.c_float),
                ("motion_contraint_reward", C.c_float), ("goal_angle_reward", C.c_float), ("boogie_contraint_reward", C.c_float)]


class StepIn(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("pos", "quat", "joints", "target", "lin_hist", "ang_hist", "euler_pre", "progress")]


class StepOut(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("obs_stride", C.c_int64), ("rew", C.c_void_p), ("reset", C.c_void_p), ("rock_collision", C.c_void_p),
                ("ex_pos_reward", C.c_void_p), ("ex_collision_penalty", C.c_void_p), ("ex_uprightness_penalty", C.c_void_p),
                ("ex_heading_contraint_penalty", C.c_void_p), ("ex_motion_contraint_penalty", C.c_void_p), ("ex_goal_angle_penalty", C.c_void_p),
                ("ex_torque_penalty_driving", C.c_void_p), ("ex_torque_penalty_steering", C.c_void_p), ("reset_ids", C.c_void_p),
                ("n_reset", C.c_void_p), ("euler", C.c_void_p), ("heading_diff", C.c_void_p), ("ray_dist", C.c_void_p), ("wheel_dist", C.c_void_p),
                ("body_dist", C.c_void_p), ("stone_collision", C.c_void_p), ("stone_margin", C.c_float), ("done_u8", C.c_void_p),
                ("ray_src", C.c_void_p), ("hit_pt", C.c_void_p)]


class Info(C.Structure):
    _fields_ = [("P", C.c_int32), ("Ns", C.c_int32), ("Nd", C.c_int32), ("rays_per_env_padded", C.c_int32), ("K", C.c_int32 * 2), ("K8", C.c_int32 * 2),
                ("X", C.c_int32 * 2), ("Y", C.c_int32 * 2), ("table_bytes", C.c_uint64 * 2), ("workspace_bytes", C.c_uint64),
                ("raycast_variant", C.c_int32), ("cell_index_mode", C.c_int32), ("ray_precision", C.c_int32), ("raycast_sorted", C.c_int32),
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


class DriveParams(C.Structure):
    _fields_ = [("wheel_radius", C.c_float), ("steer_rate", C.c_float), ("wheel_accel", C.c_float), ("slip", C.c_void_p)]


SUSPENSIONS = ("plane", "bogie")
DRIVES = ("command", "wheels")
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
    _fields_ = [("reset_ids", C.c_void_p), ("n_reset_dev", C.c_void_p), ("n_reset_host", C.c_int32), ("initial_pos3", C.c_void_p), ("pos3", C.c_void_p),
                ("quat4", C.c_void_p), ("joint_pos13", C.c_void_p), ("joint_vel13", C.c_void_p), ("base_pos3", C.c_void_p), ("reset", C.c_void_p),
                ("progress", C.c_void_p), ("yaw_deg", C.c_void_p), ("target3", C.c_void_p), ("radius", C.c_float), ("draws", C.c_void_p),
                ("max_draws", C.c_int32), ("seed", C.c_uint64), ("n_draws_used", C.c_void_p), ("yaw_deg_len", C.c_int32), ("seed_dev", C.c_void_p)]


class Profile(C.Structure):
    _fields_ = [("raycast_ms", C.c_double), ("launches", C.c_int32), ("pairs_per_launch", C.c_uint64)]


# every struct typedef include/rover_step.h declares: its mirror (tests/test_abi_mirror_host.py compares each pair, and misses no mirror)
TYPEDEFS = {
    "rover_cfg": Cfg, "rover_step_in": StepIn, "rover_step_out": StepOut, "rover_info": Info, "rover_cull_info": CullInfo,
    "rover_raycast_plan": RaycastPlan, "rover_plan_query": PlanQuery, "rover_chain_desc": ChainDesc, "rover_gauss_head": GaussHead,
    "rover_gae_desc": GaeDesc, "rover_ppo_loss_desc": PpoLossDesc, "rover_optim_chunk": OptimChunk, "rover_optim_desc": OptimDesc,
    "rover_optim_step_desc": OptimStepDesc, "rover_obs_noise_desc": ObsNoiseDesc, "rover_occlusion_cfg": OcclusionCfg,
    "rover_obs_occlusion_desc": ObsOcclusionDesc, "rover_scaler_plan_desc": ScalerPlanDesc, "rover_scaler_update_desc": ScalerUpdateDesc,
    "rover_scaler_apply_desc": ScalerApplyDesc, "rover_motion_desc": MotionDesc, "rover_bogie_params": BogieParams,
    "rover_drive_params": DriveParams, "rover_mars_desc": MarsDesc,
    "rover_track_record": TrackRecord, "rover_track_desc": TrackDesc, "rover_track_sizes_out": TrackSizes, "rover_reset_io": ResetIO,
    "rover_profile": Profile,
}

# every symbol include/rover_step.h declares: (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "rover_create": (C.c_int, [C.POINTER(Cfg), C.POINTER(_P)]),
    "rover_destroy": (None, [_P]),
    "rover_last_error": (C.c_char_p, [_P]),
    "rover_version": (C.c_char_p, []),
    "rover_set_knn_map": (C.c_int, [_P, C.c_int, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.c_float, C.c_float, C.c_float]),
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
    "rover_motion_step_drive": (C.c_int, [_P, C.POINTER(MotionDesc), C.POINTER(DriveParams), C.POINTER(BogieParams), _P]),
    "rover_motion_drive_fit": (C.c_int, [_P]),
    "rover_episode_track": (C.c_int, [_P, C.POINTER(TrackDesc), _P]),
    "rover_track_sizes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(TrackSizes)]),
    "rover_set_evaluation": (C.c_int, [_P, C.c_int32]),
    "rover_eval_clear": (C.c_int, [_P, _P, C.c_int32, _P]),
    "rover_eval_read": (C.c_int, [_P, _P, _P, _P, _P]),
    "rover_set_option": (C.c_int, [_P, C.c_char_p, C.c_int64]),
    "rover_set_profiling": (C.c_int, [_P, C.c_int32]),
    "rover_get_profile": (C.c_int, [_P, C.POINTER(Profile)]),
}

# the ctx entry points that end in no ``void *stream`` (EngineBase._call appends the current stream to every other one)
NO_STREAM = frozenset((
    "rover_set_knn_map", "rover_set_distribution", "rover_set_heightfield", "rover_set_stones", "rover_set_curriculum_level", "rover_get_info",
    "rover_get_cull_info", "rover_get_raycast_plan", "rover_build_knn_map", "rover_build_knn_map_ref", "rover_build_heightfield",
    "rover_optim_create", "rover_optim_destroy", "rover_set_occlusion", "rover_set_evaluation", "rover_set_option", "rover_set_profiling",
    "rover_get_profile"))

_lib = None
_FAKE = 16          # a non-null address for the descriptor of a route query (never read)


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


def host_call(name, *args):
    """Calls the host-only entry point ``name`` (no ctx) and raises RoverError, with the NULL ctx's error text, unless it returns ROVER_OK."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RoverError(f"{name} failed ({rc}): {lib.rover_last_error(None).decode()}")


def _route(name):
    return None if name is None else name.decode()


def route_query(name, *args):
    """The text the route query ``name`` returns (which kernel a call would run), None where the call would be refused.  Host only."""
    return _route(getattr(load(), name)(*args))


def as_dict(s):
    """A struct of integer fields as a plain dict, in field order."""
    return {k: int(getattr(s, k)) for k, _ in s._fields_}


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


class EngineBase:
    """What the per-unit halves of Engine share: the checked call on the ctx ``_h`` of ``lib`` and the operand checks."""

    def _check(self, rc, what):
        if rc != 0:
            raise RoverError(f"{what} failed ({rc}): {self.lib.rover_last_error(self._h).decode()}")

    def _call(self, name, *args, stream=None):
        """Calls the ctx entry point ``name`` with the handle in front and, unless it is one of NO_STREAM, a stream behind ``args`` (the
        current one, or the raw ``stream``); raises RoverError with the ctx's error text unless it returns ROVER_OK."""
        if name not in NO_STREAM:
            args += (_stream(self._dev_index) if stream is None else C.c_void_p(stream),)
        self._check(getattr(self.lib, name)(self._h, *args), name)

    def _chk(self, t, shape, dtype, name):
        if t is None:
            return
        if not t.is_cuda or t.device != self.device:
            raise RoverError(f"{name}: expected a tensor on {self.device}, got {t.device}")
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise RoverError(f"{name}: expected contiguous {dtype} {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")

    @staticmethod
    def _f32_rows(t, name, what, shape=None):
        """``t`` must be a float32 GPU matrix with unit column stride (a column slice of a wider row-major tensor will do), of ``shape`` if given."""
        if t is None or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or (shape is not None and tuple(t.shape) != shape):
            raise RoverError(f"{what}: {name} must be a float32 GPU matrix{'' if shape is None else ' [%d,%d]' % shape} with unit column stride")
        return t
