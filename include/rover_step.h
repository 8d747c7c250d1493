/*
 * rover_step.h — C ABI of librover_step.so: the MI355X (gfx950) implementation of the rover task's
 * vectorised env.step() hot path of abmoRobotics/isaac_rover_2.0.
 *
 * The reference is pure Python/PyTorch and has no FFI; each entry point below names the reference
 * function(s) it replaces (paths relative to omniisaacgymenvs/ in the reference repository).
 * INTEGRATION.md shows the ctypes stub a maintainer of the reference would add to call them from
 * tasks/rover.py.
 *
 * Conventions
 *  - Plain C, no torch types.  All `*_d` / step pointers are DEVICE pointers the caller owns (e.g.
 *    tensor.data_ptr()); the library borrows them for the duration of the call and never frees them.
 *  - `set_*` calls take HOST or DEVICE pointers (hipMemcpyDefault), copy into library-owned device memory,
 *    and synchronise; they are init-time calls.
 *  - Step calls only enqueue work on `stream` (a hipStream_t passed as void*; NULL = default stream) and
 *    do not synchronise.  A ctx belongs to one host thread at a time; distinct ctxs are independent.
 *  - Every function returns 0 on success or a negative ROVER_E_* code; rover_last_error() gives the text.
 *    No C++ exception crosses the boundary.
 *  - float = IEEE binary32, env-major row-major arrays, quaternions (w,x,y,z), int64 flags like the
 *    reference's torch.long buffers (tasks/base/rl_task.py:98-107).
 */
#ifndef ROVER_STEP_H
#define ROVER_STEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ROVER_API __attribute__((visibility("default")))

#define ROVER_OK            0
#define ROVER_E_INVALID    -1   /* bad argument / shape                         */
#define ROVER_E_STATE      -2   /* required set_* call missing                  */
#define ROVER_E_HIP        -3   /* HIP runtime error (text has the HIP message) */
#define ROVER_E_NOMEM      -4

#define ROVER_MAP_TERRAIN   0   /* tasks/utils/terrain/knn_terrain/{map_indices,triangles,vertices}.pt (camera.py:154-161)      */
#define ROVER_MAP_ROCKS     1   /* tasks/utils/terrain/knn_rocks/{...}.pt (rock_detect.py:151-158)  */

/* rover_step() flags */
#define ROVER_STEP_INCREMENT_PROGRESS 1u  /* progress_buf += 1 first (rl_task.py:250)                      */
#define ROVER_STEP_COMPACT            2u  /* also emit reset_ids / n_reset (rover.py:356)                   */

typedef struct rover_ctx rover_ctx;

/* Constants the reference keeps in cfg/task/Rover.yaml:11,37-46 and hard-codes in rover.py:119,101,353 */
typedef struct {
    int32_t num_envs;              /* envs handled by this ctx (this GPU's shard)                         */
    int32_t num_envs_global;       /* self.num_envs of rover.py:517 (collision_penalty); 0 = num_envs     */
    int32_t env_offset;            /* global id of local env 0 (compaction emits global ids)              */
    int32_t device;                /* HIP device ordinal                                                   */
    int32_t curriculum_level;      /* rover.py:101,353: rock collision active when >= 2                    */
    int32_t max_episode_length;    /* rover.py:119 (3000)                                                  */
    float pos_reward;              /* Rover.yaml:39 */
    float heading_contraint_reward;/* Rover.yaml:43 */
    float motion_contraint_reward; /* Rover.yaml:44 */
    float goal_angle_reward;       /* Rover.yaml:45 */
    float boogie_contraint_reward; /* Rover.yaml:46 */
} rover_cfg;

/* Sim state in (rover.py:274-275,291,343,470-476; Memory rover.py:60-77).  Device pointers. */
typedef struct {
    const float *pos;        /* [E,3]  RoverView.get_world_poses()[0]                                     */
    const float *quat;       /* [E,4]  RoverView.get_world_poses()[1], (w,x,y,z)                          */
    const float *joints;     /* [E,13] RoverView.get_joint_positions()  (legend rock_detect.py:175-187)   */
    const float *target;     /* [E,3]  self.target_positions                                              */
    const float *lin_hist;   /* [E,3]  linear_velocity.tracker, newest first                              */
    const float *ang_hist;   /* [E,3]  angular_velocity.tracker                                           */
    const float *euler_pre;  /* [E,3]  self.rover_rot captured in pre_physics_step (rover.py:343)         */
    int64_t *progress;       /* [E]    progress_buf (in/out)                                              */
} rover_step_in;

/* Outputs (rl_task.py:98-107 buffers, rover.py:524-531 extras).  Device pointers; NULL = not wanted
 * for the optional ones. */
typedef struct {
    float *obs;                    /* [E, obs_stride] obs_buf; row = [4 proprio | Ns sparse | Nd dense]   */
    int64_t obs_stride;            /* elements per obs row; 0 = 4+Ns+Nd                                   */
    float *rew;                    /* [E] rew_buf                                                         */
    int64_t *reset;                /* [E] reset_buf                                                       */
    int64_t *rock_collision;       /* [E] self.rock_collison (rover.py:667-668)                           */
    float *ex_pos_reward;          /* [E] extras, rover.py:524-531 — all optional                         */
    int64_t *ex_collision_penalty;
    float *ex_uprightness_penalty;
    float *ex_heading_contraint_penalty;
    float *ex_motion_contraint_penalty;
    float *ex_goal_angle_penalty;
    float *ex_torque_penalty_driving;
    float *ex_torque_penalty_steering;
    int64_t *reset_ids;            /* [E] ascending global env ids with reset != 0 (ROVER_STEP_COMPACT)   */
    int32_t *n_reset;              /* [1]                                                                 */
    float *euler;                  /* optional [E,3] self.rover_rotation (rover.py:275)                   */
    float *heading_diff;           /* optional [E]   self.heading_diff  (rover.py:283)                    */
    float *ray_dist;               /* optional [E,P] Camera.get_depths distances (camera.py:145)          */
    float *wheel_dist;             /* optional [E,24] rock_detect.py:146                                  */
    float *body_dist;              /* optional [E,2]  rock_detect.py:147                                  */
    /* ADDITIONAL output, not part of the reference's step (its per-step collision term is the ray-based
     * rock_collision above): the stone_info occupancy mask BASELINE.json configs[2] names.  1 where
     * nearest_rock(pos_xy) = min_s(|pos_xy - stone_s| - r_s) <= stone_margin, the clearance test of
     * check_goal_collision / avoid_pos_rock_collision (rover.py:536-539,655-658) applied to the rover itself.
     * Written by the collision stage (rover_get_observations / rover_step); never feeds reward or done. */
    int64_t *stone_collision;      /* optional [E]; needs rover_set_stones                                */
    float stone_margin;            /* metres, <= 1.4 (the reach of the occupancy grid); 0 = centre inside a disc */
    /* ADDITIONAL output: reset != 0 as one byte per env — the form the multi-GPU gather ships (SURVEY.md 8e:
     * "done [E/8] u8 or i64"); written by the is_done stage next to the int64 reset_buf. */
    uint8_t *done_u8;              /* optional [E]                                                         */
    /* The other two return values of Camera.get_depths (camera.py:118-120,145: `return output_distances, output_pt, sources`;
     * rover.py:286 binds and drops them): per terrain ray its origin (camera.py:212) and the point the reference calls the
     * intersection, sources - d * k with d = -normalize(direction) and k the ray's distance (ray_casting.py:63; for a miss
     * k = 11.0).  In the as-shipped fp16 mode both are fp16 values (widened to f32), each operation rounded to fp16. */
    float *ray_src;                /* optional [E,P,3]                                                     */
    float *hit_pt;                 /* optional [E,P,3]                                                     */
} rover_step_out;

/* ---- lifetime ------------------------------------------------------------------------------------ */
ROVER_API int rover_create(const rover_cfg *cfg, rover_ctx **out);        /* RoverTask.__init__ rover.py:81-185 */
ROVER_API void rover_destroy(rover_ctx *ctx);
ROVER_API const char *rover_last_error(const rover_ctx *ctx);             /* ctx may be NULL: last create error */
ROVER_API const char *rover_version(void);

/* ---- init-time tables ------------------------------------------------------------------------------ */
/* Camera._load_triangles_with_indices camera.py:154-161 / Rock_Detection rock_detect.py:151-158.
 * map_idx [X][Y][K] int32 (the layout after the two swapaxes), tris [T][3] int32, verts [V][3] IEEE half bits.
 * The library re-packs the three tables into one per-cell contiguous fp16 block [X*Y][9][K8]. */
ROVER_API int rover_set_knn_map(rover_ctx *ctx, int which, const int32_t *map_idx, int32_t X, int32_t Y, int32_t K,
                                const int32_t *tris, int32_t T, const uint16_t *verts_f16, int32_t V,
                                float cell_size, float shift_x, float shift_y);
/* Heightmap (heightmap_distribution.py:11-134): points [P][3] float64 in the post-swap frame, index lists */
ROVER_API int rover_set_distribution(rover_ctx *ctx, const double *points, int32_t P, const int64_t *sparse_idx,
                                     int32_t Ns, const int64_t *dense_idx, int32_t Nd);
/* heightmap_tensor.pt, rover.py:210-213 */
ROVER_API int rover_set_heightfield(rover_ctx *ctx, const float *hm, int32_t N0, int32_t N1, float horizontal_scale,
                                    float vertical_scale, float shift_x, float shift_y);
/* read_stone_info output [S][7] float32 (utils/terrain_utils/terrain_utils.py:416-424) */
ROVER_API int rover_set_stones(rover_ctx *ctx, const float *info7, int32_t S);
ROVER_API int rover_set_curriculum_level(rover_ctx *ctx, int32_t level);  /* rover.py:353 */

/* ---- per-step hot path ----------------------------------------------------------------------------- */
/* One fused RLTask.post_physics_step (rl_task.py:239-259): get_observations + calculate_metrics + is_done
 * (+ progress increment, + done compaction), same dataflow and order as the reference. */
ROVER_API int rover_step(rover_ctx *ctx, const rover_step_in *in, const rover_step_out *out, uint32_t flags, void *stream);
/* The same three stages as separate calls, for a task that keeps the reference's method split:
 * RoverTask.get_observations rover.py:272-336 (writes obs, rock_collision, optional intermediates) */
ROVER_API int rover_get_observations(rover_ctx *ctx, const rover_step_in *in, const rover_step_out *out, void *stream);
/* RoverTask.calculate_metrics rover.py:460-531 (reads out->rock_collision and the heading/position state
 * left by the last rover_get_observations on this ctx; writes rew + extras) */
ROVER_API int rover_calculate_metrics(rover_ctx *ctx, const rover_step_in *in, const rover_step_out *out, void *stream);
/* RoverTask.is_done rover.py:610-647 (writes reset) */
ROVER_API int rover_is_done(rover_ctx *ctx, const rover_step_in *in, const rover_step_out *out, void *stream);
/* Camera.get_depths(positions, rotations) camera.py:60-145 as its own call: positions [E,3], rotations [E,3] EULER angles (what the
 * reference passes: self.rover_rotation, rover.py:286) -> distances [E,P], points [E,P,3], sources [E,P,3] (each optional).  Runs the
 * step's ray pipeline on the given poses (ray precision / cell index mode / ray-cast variant as set); the observation state of the
 * ctx (heading, euler of the last rover_get_observations) is left untouched. */
ROVER_API int rover_get_depths(rover_ctx *ctx, const float *positions, const float *rotations_euler, float *distances,
                               float *points, float *sources, void *stream);
/* Rock_Detection.get_collisions(positions, rotations, joint_states) rock_detect.py:52-149 as its own call (the task holds
 * self.Rock_detector and calls it at rover.py:291): positions [E,3], rotations [E,3] EULER angles (self.rover_rotation), joints [E,13]
 * (RoverView.get_joint_positions; NULL = all zero) -> wheel_dist [E,24], body_dist [E,2] (each optional), the reference's
 * (output_distances[:, 0:24], output_distances[:, 24:]).  Same ray pipeline and options as the step.
 * rover_get_depths and rover_get_collisions overwrite the ctx's ray workspace (ray records, sorted list, distances, cull counters:
 * what rover_replay_raycast / rover_get_cull_info / the profile describe afterwards is THIS call's rays); they leave the observation
 * state (euler, heading) alone and do not stand in for rover_get_observations: rover_calculate_metrics still requires that one. */
ROVER_API int rover_get_collisions(rover_ctx *ctx, const float *positions, const float *rotations_euler, const float *joints,
                                   float *wheel_dist, float *body_dist, void *stream);
/* The ray phase on its own, for parity tests that must not depend on the pose trigonometry (ray_casting.py:3-66 + the cell lookup
 * camera.py:233-264 + min over K, camera.py:116-117):
 *  rover_export_rays: the rays of the last cast on this ctx in slot order — per env 24 wheel, 2 body, P heightmap rays: origins
 *    src [E,26+P,3], the ray records' directions dir [E,26+P,3] (= -normalize(direction), ray_casting.py:31, as the kernels use it),
 *    cell ids cell [E,26+P] int32, distances dist [E,26+P] (each optional).
 *  rover_cast_rays: casts caller-supplied rays in the same layout (origins + record directions; slots 0..25 against the rocks map,
 *    the rest against the terrain map) through the step's sort + ray-cast kernels (variant / precision / cell index mode as set) and
 *    returns their distances dist [E,26+P].  Overwrites the ray workspace like rover_get_depths.  The directions are used as they are:
 *    with the culled / staged ray cast (variants 3, 4), whose rejection proofs assume what -normalize() produces, a finite direction
 *    whose squared length is not within 1e-5 of 1 (4e-3 with ray_precision 2) is ROVER_E_INVALID — the call synchronises the stream to
 *    find out; variants 1 and 2 evaluate every triangle and take any direction. */
ROVER_API int rover_export_rays(rover_ctx *ctx, float *src, float *dir, int32_t *cell, float *dist, void *stream);
ROVER_API int rover_cast_rays(rover_ctx *ctx, const float *src, const float *dir, float *dist, void *stream);
/* reset_buf.nonzero() rover.py:356 without the host sync: ids ascending (+env_offset), count to n_reset[0] */
ROVER_API int rover_compact_resets(rover_ctx *ctx, const int64_t *reset, int64_t *reset_ids, int32_t *n_reset, void *stream);
/* tensor_quat_to_eul tasks/utils/math/tensor_quat_to_euler.py:6-31 */
ROVER_API int rover_quat_to_euler(rover_ctx *ctx, const float *quat, float *euler, int32_t n, void *stream);

/* ---- reset / spawn / goal validation (rover.py:533-564, 588-608, 649-661) ---------------------------- */
/* nearest_rock = min_s(|p - stone_s| - r_s)  (rover.py:536-538,655-658); xy [n][2] -> out [n].  The minimum is torch.min's: +inf
 * without stones, and NaN for every query as soon as one stone holds a NaN in x, y or r (the decisions made on it — spawn shift, goal
 * validation, the step's stone mask — then find no collision anywhere, as `NaN <= thr` does in the reference). */
ROVER_API int rover_clearance(rover_ctx *ctx, const float *xy, int32_t n, float *out, void *stream);
/* avoid_pos_rock_collision rover.py:649-661: per env, x += 0.05 while clearance <= 1.4; pos [n][3] in place */
ROVER_API int rover_shift_spawns(rover_ctx *ctx, float *pos3, int32_t n, int32_t max_iter, void *stream);
/* get_pos_height rover.py:588-608: xy [n][2] -> out [n] */
ROVER_API int rover_sample_height(rover_ctx *ctx, const float *xy, int32_t n, float *out, void *stream);
/* generate_goals + random_goals + check_goal_collision rover.py:533-564, radius 8 (rover.py:578), then the
 * goal z lookup of set_targets rover.py:582-583.  env_ids [n] int64 (local ids into target3/initial_pos3);
 * draws = [max_draws][n] uniforms in [0,1) replacing torch.rand (NULL = library Philox stream seeded by
 * `seed`); reproduces the env_ids = mask*env_ids aliasing of rover.py:540.  n_draws_used[0] (optional)
 * receives the number of draws consumed, or -1 if max_draws ran out before every goal was clear. */
ROVER_API int rover_generate_goals(rover_ctx *ctx, const int64_t *env_ids, int32_t n, const float *initial_pos3,
                                   float *target3, float radius, const float *draws, int32_t max_draws, uint64_t seed,
                                   int32_t *n_draws_used, void *stream);

/* ---- device-side reset orchestration ("next" row f-2): reset_idx + set_targets rover.py:416-453,566-584 ----- */
/* Consumes the compacted reset ids of the last step WITHOUT the host sync of rover.py:357: the count is read from
 * device memory (n_reset_dev) by the kernels.  For every listed env: pose = initial_pos, orientation = the
 * reference's (w,x,y,z) <- scipy (x,y,z,w) yaw quirk with d = yaw_deg[i] or a Philox draw in [0,360], joint
 * positions / velocities zeroed, reset = 0, progress = 0; then (if target3 != NULL) goals are re-drawn and validated
 * exactly like rover_generate_goals, including the goal z lookup.  All pointers are device pointers. */
typedef struct {
    const int64_t *reset_ids;     /* [E] ascending GLOBAL env ids (rover_step's reset_ids)                         */
    const int32_t *n_reset_dev;   /* [1] device count; NULL = use n_reset_host                                     */
    int32_t n_reset_host;
    const float *initial_pos3;    /* [E,3] self.initial_pos                                                        */
    float *pos3, *quat4;          /* [E,3], [E,4] RoverView poses (in place)                                       */
    float *joint_pos13, *joint_vel13; /* [E,13] optional                                                           */
    float *base_pos3;             /* [E,3] optional self.base_pos                                                  */
    int64_t *reset, *progress;    /* [E] reset_buf, progress_buf                                                   */
    const int32_t *yaw_deg;       /* [yaw_deg_len] optional: replaces random.randint(0, 360) (rover.py:429); entry i
                                   * belongs to reset_ids[i]                                                        */
    float *target3;               /* [E,3] optional self.target_positions: re-draw + validate goals                */
    float radius;                 /* rover.py:578 (8)                                                              */
    const float *draws;           /* optional [max_draws][n] uniforms (needs n_reset_host)                         */
    int32_t max_draws;
    uint64_t seed;
    int32_t *n_draws_used;        /* optional [1]                                                                  */
    int32_t yaw_deg_len;          /* entries in yaw_deg: >= n_reset_host, or >= num_envs when n_reset_dev is used   */
    const uint64_t *seed_dev;     /* optional [1] device word ADDED to `seed` (mod 2^64) when the kernels run: a caller that replays the
                                   * call from a captured hipGraph keeps its step counter there, so that every replay draws anew   */
} rover_reset_io;
ROVER_API int rover_reset_envs(rover_ctx *ctx, const rover_reset_io *io, void *stream);

/* ---- action side ("next" row f-1) --------------------------------------------------------------------------- */
/* pre_physics_step rover.py:338-414 minus the reset branch, one kernel: euler_pre = tensor_quat_to_eul(quat) (:343),
 * Memory.input_state for both histories (:379-380, in place, newest first), Ackermann (:391) and the scatter of
 * 4 steering angles / 6 wheel speeds into the [E,13] joint-target arrays at the indices of
 * robots/articulations/views/rover_view.py:45-46.  actions [E,2]; euler_pre / targets optional; actions_nn optional [E,2,3]:
 * self.actions_nn (:366: the newest action prepended, the oldest dropped), in place. */
ROVER_API int rover_pre_physics_step(rover_ctx *ctx, const float *actions, const float *quat, float *lin_hist,
                                     float *ang_hist, float *euler_pre, float *joint_pos_targets13,
                                     float *joint_vel_targets13, float *actions_nn, void *stream);
/* Ackermann tasks/utils/kinematics.py:13-67 on its own:
 * lin, ang [n] -> steering [n][6], velocities [n][6] in wheel order FL,FR,ML,MR,RL,RR */
ROVER_API int rover_ackermann(rover_ctx *ctx, const float *lin, const float *ang, int32_t n, float *steering,
                              float *velocities, void *stream);

/* ---- evaluation mode: per-rover outcome codes (rover.py:122-137 buffers, :620-641 is_done, :670-672 check_collision) ------- */
/* The reference's is_evaluation branch.  Per env a code, 0 until the env's FIRST outcome, then never changed and never cleared by a
 * reset (only the first outcome of each rover counts, rover.py:124-129):
 *   1  collided (check_collision, :670-672 — run by get_observations only at curriculum level >= 2, :292-293), or out of area:
 *      target distance >= 9.5 (:622-624; no reset below 11),
 *   2  reached the goal: target distance <= 0.18 (:627-628),
 *   3  timed out: progress >= max_episode_length (:630-631),
 * checked in that order (a collision of the same step beats everything, then out of area, goal, timeout).  A tilt reset or the
 * d >= 11 reset gives no code of its own.  ADDITIONAL output (not in the reference): eval_step, the env's progress at the step its code
 * latched (the steps to the outcome).  The latch runs inside the metrics pass of rover_step (both stages, reference order),
 * rover_get_observations (collision, level >= 2) and rover_is_done (the other three); rover_calculate_metrics, rover_get_depths,
 * rover_get_collisions and rover_cast_rays never latch.  While evaluation is on, those calls need in->progress.
 * The file dump of :632-640 (torch.save at global_step % max_episode_length == 0) is the caller's: RoverTask(eval_save_dir=...).
 *
 * rover_set_evaluation: init-time.  enable != 0 allocates the ctx's two [E] int64 arrays (eval_res, eval_step), zeroes them and
 *   synchronises the device; enable = 0 frees them and turns the latch off.  With evaluation off the step's outputs and kernels are
 *   those of a ctx that never had it. */
ROVER_API int rover_set_evaluation(rover_ctx *ctx, int32_t enable);
/* Resets env_ids [n] (LOCAL ids, a device pointer) to code 0 and step 0, or every env when env_ids is NULL (n is then ignored): a new
 * evaluation window, or chosen envs re-armed.  The ids are checked on the host (the call synchronises `stream` when env_ids is given):
 * an id outside [0, num_envs) or n outside [0, num_envs] is ROVER_E_INVALID.  ROVER_E_STATE while evaluation is off. */
ROVER_API int rover_eval_clear(rover_ctx *ctx, const int64_t *env_ids, int32_t n, void *stream);
/* Copies the state out on `stream`, enqueue only (no synchronisation); every pointer is an optional DEVICE pointer:
 * eval_res [E] int64 (self.rover_eval_res, rover.py:130), eval_step [E] int64, summary8 [8] int64 = count of codes 0..3, then the sum of
 * eval_step over the envs of codes 0..3 (exact integer sums).  ROVER_E_STATE while evaluation is off. */
ROVER_API int rover_eval_read(rover_ctx *ctx, int64_t *eval_res, int64_t *eval_step, int64_t *summary8, void *stream);

/* ---- KNN map builder ("next" row f-3): tasks/utils/rover_utils.py:48-123 ------------------------------------ */
/* For every cell (x, y) of an X x Y map at `res` metres per cell (cell position = (x res, y res), rover_utils.py:75-81)
 * the K triangles whose centroid ((v0+v1+v2)/3, :68-70) is nearest in xy, ascending.  vertices [V,3] float32,
 * triangles [T,3] int32 (host or device pointers); map_idx_out [X,Y,K] int32 is a DEVICE pointer.  Ranking is exact f32
 * squared distance with ties broken by triangle id; the reference ranks fp16-rounded distances with torch.topk (ties
 * unspecified), so its maps agree with this one only up to that rounding.  Synchronous (init-time tool); needs no
 * prior set_* call.  A vertex index outside [0, V) reads vertex 0; a triangle with a NaN centroid ranks after every other.
 * Fails with ROVER_E_INVALID when T < K, K > 4096, a centroid is infinite, or a search ring holds more than 8192 candidates. */
ROVER_API int rover_build_knn_map(rover_ctx *ctx, const float *vertices, int32_t V, const int32_t *triangles, int32_t T,
                                  int32_t X, int32_t Y, float res, int32_t K, int32_t *map_idx_out);

/* The same builder ranking EXACTLY like the reference does (rover_utils.py:71-102): triangle centroids and cell coordinates
 * are fp16 tensors there, so per axis the difference is rounded to fp16, the norm is the f32 sqrt of the f32 sum of squares
 * rounded to fp16, and torch.topk picks the K smallest of those fp16 distances (tie order unspecified; here: by triangle id).
 * cell_x_f16 [X] / cell_y_f16 [Y] (IEEE half bits, host or device; NULL = fp16(float(i) * res), what ATen's CUDA arange yields)
 * are the coordinate tables of the reference's torch.arange(0, X*res, res, dtype=float16) (:75-76) — ATen's CPU arange
 * evaluates that in vector-width-dependent fp16 steps, so a map built by the reference on a CPU is reproduced by passing the
 * table that host produced.  Result per cell: the same multiset of fp16 distances as the reference's list, the same triangles
 * except among those tied with the K-th distance. */
ROVER_API int rover_build_knn_map_ref(rover_ctx *ctx, const float *vertices, int32_t V, const int32_t *triangles, int32_t T,
                                      int32_t X, int32_t Y, float res, int32_t K, const uint16_t *cell_x_f16,
                                      const uint16_t *cell_y_f16, int32_t *map_idx_out);

/* ---- heightfield from a triangle mesh: what rover_set_heightfield takes, made from the mesh the rays hit ------------------------
 * For every node of an N0 x N1 grid the highest point of the mesh above it.  vertices [V,3] float32 and triangles [T,3] int32 are host
 * or device pointers; hm_out [N0][N1] float32 is a DEVICE pointer and holds metres (a scene built from it has vertical_scale 1); stats
 * is a host pointer and may be NULL: {nodes no triangle covers, triangles skipped}.  Synchronous (init-time tool); needs no prior set_*
 * call.  This is the project's own definition (the reference ships its heightfield as an asset, without a generator):
 *
 *  1. Node (i, j) sits at world (shift_x + i hs, shift_y + j hs), hs = horizontal_scale: the point whose lookup rover_sample_height
 *     rounds to (i, j).  In sub-units, 256 per node spacing, its coordinates are (256 i, 256 j).
 *  2. A vertex's xy is snapped once, in double: X = (int64) rint((((double) x - (double) shift_x) / (double) hs) * 256.0), in that
 *     order (rint: to nearest, ties to even); Y likewise.  z stays the f32 value, read as a double.
 *  3. A triangle is SKIPPED and counted in stats[1] when an index lies outside [0, V), when a coordinate (x, y or z) of one of its
 *     vertices is not finite, or when a snapped |X| or |Y| exceeds 2^25 (that limit keeps every edge function within 2^53: exact in
 *     int64 and exactly convertible to double).  A triangle with area = (bx - ax)(cy - ay) - (by - ay)(cx - ax) == 0 — a vertical
 *     wall, a sliver snapped flat — contributes nothing and is not counted.
 *  4. At node p = (px, py):  wa = (cx - bx)(py - by) - (cy - by)(px - bx),  wb = (ax - cx)(py - cy) - (ay - cy)(px - cx),
 *     wc = (bx - ax)(py - ay) - (by - ay)(px - ax); where area < 0 all three and the area are negated.  The node is covered iff
 *     wa >= 0 && wb >= 0 && wc >= 0: edges and vertices are inclusive, a shared edge belongs to both triangles.  All of it is integer
 *     arithmetic, so coverage is exact, watertight and independent of any order.
 *  5. z = (float)((((double) wa * za + (double) wb * zb) + (double) wc * zc) / (double) area): one IEEE rounding per operation (no
 *     fused multiply-add), the correctly rounded f64 division, then one rounding to f32.
 *  6. hm[i][j] is the maximum of z over the covering triangles — a rock on the terrain wins over the ground under it — in the IEEE
 *     order with -0 below +0.  A node that no triangle covers gets `fill` and is counted in stats[0].
 *
 * The maximum is taken with an integer atomic on an order-preserving key of the f32 bits, so the result is the same bits on every run.
 * The arguments are validated before the ctx is looked at (with a NULL ctx rover_last_error(NULL) has the text).  ROVER_E_INVALID: N0 or
 * N1 outside 1 .. 131072, horizontal_scale not finite or <= 0, a shift not finite, V < 0, T < 0, vertices NULL with V > 0, triangles NULL
 * with T > 0, hm_out NULL, a NULL ctx. */
ROVER_API int rover_build_heightfield(rover_ctx *ctx, const float *vertices, int32_t V, const int32_t *triangles, int32_t T,
                                      int32_t N0, int32_t N1, float horizontal_scale, float shift_x, float shift_y,
                                      float fill, float *hm_out, int64_t stats[2]);
/* Host only (no ctx, no device): the sizes that separate the rasteriser's code paths.  out[0]: the largest bounding box, in nodes
 * (clipped to the grid), that a group of out[3] lanes rasterises on its own; a larger box is cut along the grid's multiples of
 * out[1] (i) x out[2] (j) nodes into tiles, one workgroup each.  ROVER_E_INVALID for a NULL out. */
ROVER_API int rover_heightfield_limits(int32_t out[4]);

/* ---- Mars terrain generator: the heightfield of Gaussian hills and rock stamps -----------------------------------------------------
 * What the reference's gaussian_terrain + add_rocks_terrain (utils/terrain_utils/terrain_generation.py) leave in height_field_raw, from a
 * plan that names every hill and every rock stamp (isaac_rover_amd/terrain_gen.py makes one from a seed).  Every array of the descriptor
 * is a HOST pointer; the library copies what the kernel reads. */
#define ROVER_MARS_MAX_SIDE     131072   /* largest rows, cols */
#define ROVER_MARS_MAX_CLASSES  16
#define ROVER_MARS_MAX_TABLE    129      /* largest side of a class table */
#define ROVER_MARS_TILE         16       /* the kernel's tile: 16 x 16 nodes per workgroup */
typedef struct rover_mars_desc {
    int32_t rows, cols;              /* the field [rows][cols] */
    int32_t n_hills;
    const int32_t *hill_window;      /* [n_hills][6] r0, r1, c0, c1, a0, b0: rows r0 .. r1 - 1 and columns c0 .. c1 - 1 are covered */
    const double *hill_amp;          /* [n_hills] */
    const double *g;                 /* [g_len] the 1-D hill table */
    int32_t g_len;
    int32_t n_classes;
    const int32_t *class_side;       /* [n_classes] side of each square class table */
    const double *class_tables;      /* the tables one after the other, class k row-major [side_k][side_k] */
    int32_t n_stamps;
    const int32_t *stamp_row;        /* [n_stamps] first row of the stamp's square */
    const int32_t *stamp_col;        /* [n_stamps] first column */
    const int32_t *stamp_class;      /* [n_stamps] */
    const double *stamp_factor;      /* [n_stamps] */
    const uint8_t *stamp_kept;       /* [n_stamps] 0: the stamp is not applied (nothing else of it is checked or read by the kernel) */
} rover_mars_desc;
/* hf [rows][cols] float64 and rock_mask [rows][cols] uint8 (may be NULL) are DEVICE pointers.  Synchronous (init-time tool); needs no
 * prior set_* call.  The definition, per node (r, c):
 *
 *   h = 0.0
 *   for every hill i = 0 .. n_hills - 1 with r0 <= r < r1 and c0 <= c < c1, in index order:
 *       h = h + (g[a0 + r - r0] * g[b0 + c - c0]) * hill_amp[i]
 *   for every stamp s = 0 .. n_stamps - 1 with stamp_kept[s] and 0 <= r - stamp_row[s] < side and 0 <= c - stamp_col[s] < side
 *   (side = class_side[stamp_class[s]]), in index order:
 *       h = h + T[r - stamp_row[s]][c - stamp_col[s]] * stamp_factor[s]            (T: the table of the stamp's class)
 *   hf[r][c] = h;  rock_mask[r][c] = 1 if some stamp took part, else 0
 *
 * Every product and every sum is one IEEE float64 rounding, in the written order; no fused multiply-add.  That is the per-node view of
 * the reference's sequential `field[slice] += table * factor`, so the result is the reference's bit for bit.  The kernel gathers (one
 * workgroup per ROVER_MARS_TILE^2 nodes walks that tile's stamps in ascending order): no atomics, the same bits on every run.
 * The per-tile stamp lists are built inside the call from the descriptor; rover_mars_tiles returns them.
 *
 * The arguments are validated before the ctx is looked at (with a NULL ctx rover_last_error(NULL) has the text; it starts with
 * "mars_heightfield:").  ROVER_E_INVALID: a NULL descriptor or hf; rows or cols outside 1 .. ROVER_MARS_MAX_SIDE; n_hills, n_classes or
 * n_stamps negative; n_classes above ROVER_MARS_MAX_CLASSES; a needed array NULL; g_len < 1; a class_side outside
 * 1 .. ROVER_MARS_MAX_TABLE; a hill_window that is not 0 <= r0 <= r1 <= rows, 0 <= c0 <= c1 <= cols, a0 >= 0, a0 + r1 - r0 <= g_len
 * (b0 likewise); a hill_amp or the stamp_factor of a kept stamp that is not finite; a kept stamp whose class is out of range or whose
 * square is not inside the field; a NULL ctx. */
ROVER_API int rover_mars_heightfield(rover_ctx *ctx, const rover_mars_desc *desc, double *hf, uint8_t *rock_mask, void *stream);
/* Host only (no ctx, no device), a pure function: the tile lists the launch builds.  Tile (ti, tj) holds the nodes
 * ROVER_MARS_TILE ti .. + 15 x ROVER_MARS_TILE tj .. + 15 and has the number t = ti ceil(cols / 16) + tj.  tile_start
 * [ceil(rows / 16) ceil(cols / 16) + 1] and tile_items [capacity]: tile t's list is tile_items[tile_start[t] .. tile_start[t + 1] - 1],
 * the ascending ids of the kept stamps whose square meets the tile.  *n_items = the total length.  tile_start and tile_items may both be
 * NULL to ask for n_items alone.  ROVER_E_INVALID as above (messages start with "mars_tiles:"), for a NULL n_items, for a capacity below
 * n_items when the lists are asked for, and where the total length exceeds 2^31 - 1. */
ROVER_API int rover_mars_tiles(const rover_mars_desc *desc, int32_t *tile_start, int32_t *tile_items, int64_t capacity, int64_t *n_items);

/* ---- policy-side consumer of the obs layout ("next" row f-4): learning/model.py:105-121 Layer = Linear + activation --- */
#define ROVER_ACT_NONE      0
#define ROVER_ACT_LEAKYRELU 1   /* nn.LeakyReLU(), slope 0.01 (cfg/trainSKRL/RoverPPOSKRL.yaml:5,9) */
#define ROVER_ACT_TANH      2   /* the actor head, model.py:182 */
#define ROVER_ACT_RELU      3
#define ROVER_ACT_ELU       4
/* y[:, 0:N] = act(x[:, 0:K] @ weight^T + bias); weight [N][K] (torch nn.Linear layout), bias [N] or NULL, N <= 256.
 * x / y are addressed as (pointer, row stride in floats), so a layer can read an obs slice (model.py:186-187) and write
 * into a column block of the concat buffer (:191-192) without copies.  f32-input MFMA, fp32 accumulate. */
ROVER_API int rover_linear_forward(rover_ctx *ctx, const float *x, int64_t x_stride, int32_t M, int32_t K,
                                   const float *weight, const float *bias, int32_t N, int32_t activation, float *y,
                                   int64_t y_stride, void *stream);

/* A chain of 2 or 4 such layers in ONE kernel: y = L_n(... L_1(x[:, 0:K0])), L_i(v) = act_i(W_i v + b_i) — an Encoder
 * (learning/model.py:122-150: 634 -> 80 -> 60) or the MLP with its head (:176-195: 124 -> 256 -> 160 -> 128 -> 2).  Only x and the
 * last layer's output touch HBM: the activations stay in the MFMA accumulator registers, which are the next layer's B operand as
 * they are (csrc/rover_mlp.hip).  weights[i] is nn.Linear's [widths[i]][widths[i-1]] (K0 for i = 0), biases[i] may be NULL.
 * Built tile shapes: 2 layers with widths <= 96, <= 64; 4 layers with widths <= 256, <= 160, <= 128, <= 16 and activation 0, 1 or 3
 * (none / LeakyReLU / ReLU) on the three hidden layers (else ROVER_E_INVALID: use rover_linear_forward per layer).  That rule, and
 * which kernel a chain gets at which batch size, lives in ONE place, chain_route() of csrc/rover_mlp.hip; a caller that has to know
 * beforehand asks rover_mlp_chain_route below (non-NULL: the chain fits) instead of restating widths or row counts, as the Python
 * binding's chain_fits() and the policy nets' forward plan (learning/model.py) do.  Same numerics as rover_linear_forward up to the
 * summation order inside a layer.
 * Small batches (M < 20 480 with a 2-layer chain) go through a split-k scratch buffer that the ctx owns and grows on demand: the
 * chain entry points of one ctx must therefore run on ONE stream at a time (two forwards overlapped on different streams need two
 * ctxs), and the first small-batch call of a given size must not happen inside a stream capture (it may hipMalloc and synchronise);
 * warm it up once before capturing. */
ROVER_API int rover_mlp_chain_forward(rover_ctx *ctx, const float *x, int64_t x_stride, int32_t M, int32_t K0, int32_t n_layers,
                                      const float *const *weights, const float *const *biases, const int32_t *widths,
                                      const int32_t *activations, float *y, int64_t y_stride, void *stream);

/* Two 2-layer chains over the SAME M rows — the two encoders of the actor / critic (learning/model.py:188-190: sparse and dense
 * heightmap slices of one obs row; neither depends on the other) — and, optionally, the copy of the proprioception columns into the
 * concat buffer (:191: dst[r][0:copy_cols] = src[r][0:copy_cols]; copy_cols = 0: none).  Small batches (M < 20 480, both chains of
 * the same built tile shape) run the two side by side: ONE launch for both first layers (split along k), one for both second layers
 * and the copy — a third of the actor forward's launches at the reference's default numEnvs 512 (cfg/task/Rover.yaml:11).  Otherwise
 * the chains run one after the other.  Results are those of two rover_mlp_chain_forward calls either way. */
typedef struct {
    const float *x; int64_t x_stride; int32_t K0, n_layers;
    const float *const *weights; const float *const *biases; const int32_t *widths; const int32_t *activations;
    float *y; int64_t y_stride;
} rover_chain_desc;
ROVER_API int rover_mlp_chain_pair_forward(rover_ctx *ctx, int32_t M, const rover_chain_desc *a, const rover_chain_desc *b,
                                           const float *copy_src, int64_t copy_src_stride, float *copy_dst, int64_t copy_dst_stride,
                                           int32_t copy_cols, void *stream);

/* Which kernel instantiation the three calls above would launch for these shapes — host only: no ctx, no launch, no pointer read
 * but widths / activations (and, for the pair, those of the two descriptors).  Returns the instantiation's name:
 *   rover_linear_route: "linear_act<1,1>" (one 32-column tile per workgroup) below 65 536 rows, else "linear_act<NT,4>" with
 *     NT = 1..5 output tiles, "x2" appended when the columns are split in two halves ("linear_act<3,4>x2", "linear_act<4,4>x2");
 *   rover_mlp_chain_route: "splitk<TN,RT>" (TN in {5, 6}, RT in {1, 2}: the two kernels of the split-k path), "mlp_small",
 *     "chain16<5,4,0,0>", "chain16<6,4,0,0>" or "chain16<16,10,8,1>";
 *   rover_mlp_chain_pair_route: "pair(splitk<TN,RT>)" when both chains run side by side, else "seq(<a>;<b>)" (one after the other,
 *     the copy as a hipMemcpy2DAsync).
 * "none" where the call launches nothing (M = 0); NULL where it would be refused with ROVER_E_INVALID for its shapes.  Some names are
 * composed in a buffer of the calling thread: a returned pointer is valid until that thread's next route query (any of these three or
 * rover_mlp_chain_act_route). */
ROVER_API const char *rover_linear_route(int32_t M, int32_t K, int32_t N);
ROVER_API const char *rover_mlp_chain_route(int32_t M, int32_t K0, int32_t n_layers, const int32_t *widths,
                                            const int32_t *activations);
ROVER_API const char *rover_mlp_chain_pair_route(int32_t M, const rover_chain_desc *a, const rover_chain_desc *b);

/* ---- the actor's Gaussian head: act() = sampled action + log-probability (learning/model.py:152-195 under skrl's GaussianMixin) ---- */
/* Semantics of torch.distributions.Normal.  With mean [M, A] (the Tanh head's output), ls = log_std [A]:
 *   ls'      = clamp(ls, min_log_std, max_log_std) if clip_log_std, else ls;        sigma = exp(ls')
 *   actions  = mean + sigma * eps  (deterministic: mean), then clamp(actions, low, high) if clip_actions
 *   x        = taken_actions if given, else the returned (possibly clamped) f32 actions
 *   log_prob = reduce_j [ -((x_j - mean_j) / sigma_j)^2 / 2 - ls'_j - 0.5 log(2 pi) ]   ([M, 1]; ROVER_REDUCE_NONE: the terms, [M, A])
 * log_prob is computed from x - mean, never from eps, so a call with taken_actions = the actions an earlier call returned gives that
 * call's log_prob bit for bit.
 * Noise: Philox4x32-10 (the generator of the goal / reset-yaw draws), for global row g = row_offset + r, call counter t and
 * component pair p = j / 2:
 *   w = philox(counter = (g, t & 0xffffffff, t >> 32, 0x50000000 | p), key = (seed & 0xffffffff, seed >> 32))
 *   u0 = ((w[0] >> 8) + 1) 2^-24 in (0, 1],  u1 = (w[1] >> 8) 2^-24 in [0, 1),  rad = sqrt(-2 ln u0)
 *   eps[2 p] = rad cos(2 pi u1),  eps[2 p + 1] = rad sin(2 pi u1)                  (finite, |eps| <= sqrt(48 ln 2) = 5.7681)
 * The fourth counter word is 0 in the goal / yaw draws: the streams are disjoint under one seed.  A draw depends on (seed, t, g, j)
 * alone — not on M, not on the kernel that runs the head, not on how a batch is sharded (a shard passes its env_offset as row_offset).
 * The call counter is t = step + *step_dev (mod 2^64; step_dev NULL: step alone), read by the kernels WHEN THEY RUN.  The library never
 * writes it: the caller advances *step_dev, with work enqueued on the SAME stream after the call (one increment per act), inside the
 * captured region when the call is captured — then an eager call and a graph replay read and advance the same word and cannot drift
 * apart.  A caller that evaluates log_prob for taken_actions, or passes an explicit step, does not advance it. */
#define ROVER_REDUCE_SUM  0     /* skrl's reduction="sum" (the reference's, model.py:153-156) */
#define ROVER_REDUCE_MEAN 1
#define ROVER_REDUCE_PROD 2
#define ROVER_REDUCE_MAX  3
#define ROVER_REDUCE_MIN  4
#define ROVER_REDUCE_NONE 5     /* log_prob is [M, A] */
typedef struct {
    const float *log_std;         /* [A] device: log_std_parameter (model.py:183)                                              */
    int32_t A;                    /* 1 .. 16 components                                                                         */
    int32_t clip_log_std;         /* clamp log_std to [min_log_std, max_log_std] (needs min <= max)                             */
    float min_log_std, max_log_std;
    int32_t clip_actions;         /* clamp the sampled actions to [low, high] (needs low <= high)                               */
    float low, high;
    int32_t reduction;            /* ROVER_REDUCE_*                                                                             */
    int32_t deterministic;        /* actions = mean                                                                             */
    uint64_t seed, step;
    const uint64_t *step_dev;     /* optional [1] device word added to step when the kernels run (see above)                    */
    int64_t row_offset;           /* global row of row 0: >= 0, row_offset + M <= 2^32                                          */
    const float *taken_actions;   /* optional [M, A] device: log_prob is evaluated at these                                     */
    int64_t taken_stride;
    float *actions;               /* [M, A] out */
    int64_t actions_stride;
    float *log_prob;              /* [M, 1] out, [M, A] with ROVER_REDUCE_NONE */
    int64_t log_prob_stride;
    const float *mean;            /* rover_gaussian_head: the given mean [M, A].  rover_mlp_chain_act: unused (NULL) — the mean is  */
    int64_t mean_stride;          /*   the chain's output y ("mean_actions")                                                    */
} rover_gauss_head;
/* rover_mlp_chain_forward with the head on its last layer's output (widths[n_layers - 1] == head->A): y receives the mean, exactly as
 * rover_mlp_chain_forward writes it.  For A <= 4 on the two kernels that end the actor's forward ("mlp_small", "chain16<16,10,8,1>")
 * the head runs INSIDE that kernel (the whole head of a row sits in one lane's accumulator registers): as many launches as the forward.
 * Every other chain runs its forward and then the head as one more launch.  Chains outside the built tile shapes are refused like
 * rover_mlp_chain_forward refuses them (run the layers one by one, then rover_gaussian_head).  The chain entry points' rule carries
 * over: one stream per ctx at a time, the first small-batch call of a size warmed up outside a stream capture. */
ROVER_API int rover_mlp_chain_act(rover_ctx *ctx, const float *x, int64_t x_stride, int32_t M, int32_t K0, int32_t n_layers,
                                  const float *const *weights, const float *const *biases, const int32_t *widths,
                                  const int32_t *activations, float *y, int64_t y_stride, const rover_gauss_head *head, void *stream);
/* The head on a given mean (head->mean [M, A], A <= 16): one launch, one thread per row. */
ROVER_API int rover_gaussian_head(rover_ctx *ctx, int32_t M, const rover_gauss_head *head, void *stream);
/* eps [M, A] (A <= 16) alone, as the head draws it for (seed, step + *step_dev, row_offset). */
ROVER_API int rover_policy_noise(rover_ctx *ctx, uint64_t seed, uint64_t step, const uint64_t *step_dev, int64_t row_offset, int32_t M,
                                 int32_t A, float *eps, int64_t eps_stride, void *stream);
/* Host only (no ctx, no device): out[4] = Philox4x32-10(counter[4], key[2]) — the round function the kernels run, on the CPU. */
ROVER_API int rover_philox4x32(const uint32_t *counter, const uint32_t *key, uint32_t *out);
/* What rover_mlp_chain_act would launch — host only, no pointer is read but widths / activations and the descriptor's own fields
 * (its pointers are only tested for NULL): "mlp_small+gauss" / "chain16<16,10,8,1>+gauss" when the head is fused into the chain's last
 * kernel, "<rover_mlp_chain_route's name>;gauss" when it is a launch of its own, "none" for M = 0, NULL where the call would be
 * refused with ROVER_E_INVALID (rover_last_error(NULL) says why).  The pointer is valid until the calling thread's next route query. */
ROVER_API const char *rover_mlp_chain_act_route(int32_t M, int32_t K0, int32_t n_layers, const int32_t *widths,
                                                const int32_t *activations, const rover_gauss_head *head);

/* ---- the same chains with bf16 operands and f32 accumulation: inference for rollouts (precision = "bf16") ------------------------- */
/* CDNA4's f32-input MFMA runs at 1/16 of the bf16 rate, and the f32 chain kernels above are bound by it.  A rollout needs the sampled
 * action, its log-probability under the policy that ACTED, and the value: all three may come from a lower-precision forward, since PPO's
 * ratio is pi_new / pi_behaviour with the behaviour policy's own stored log_prob.  Training stays f32; these entry points have no
 * backward.
 * The arithmetic, for a chain y = L_n(... L_1(x)) — the tests hold the kernels to it:
 *   inputs and weights   every element of x and of each W_i is rounded to bf16 as it is read: round to nearest even, NaN stays NaN,
 *                        +-Inf stays +-Inf (a finite f32 above the largest bf16 becomes Inf).  rover_bf16_round is that rounding.
 *   products and sums    a product of two bf16 values is exact in f32; the products of a row are summed in f32 in a fixed order.
 *   bias and activation  the f32 bias is added in f32; the activation is the f32 kernels' own, in f32.
 *   between layers       the output of every layer but the last is rounded to bf16 (as above) before the next layer reads it.
 *   last layer           its output is f32, not rounded.
 *   Gaussian head        the f32 head (above) on that f32 mean: noise, clamps, log_prob and taken_actions semantics unchanged.
 * No bf16 copy of the weights is kept anywhere: they are read as f32 and converted as they are staged, so a weight changed in place
 * (rover_optim_step writes through raw pointers) is seen by the next call.
 * Same parameters, shapes and refusals as rover_mlp_chain_forward / rover_mlp_chain_act, with one addition: K0 = 0 is accepted (a chain
 * over an empty obs slice, model.py's Encoder(0, ...): the first layer is act_1(b_1), as rover_linear_forward computes it for K = 0; x and
 * weights[0] are not read and may be NULL), so that a net with an absent heightmap part runs in one precision.  ONE kernel per tile shape covers every batch
 * size — "chain_bf16<5,4,0,0>", "chain_bf16<6,4,0,0>" (2 layers), "chain_bf16<16,10,8,1>" (4 layers); rover_mlp_chain_act_bf16 runs the
 * head inside the 4-layer kernel for A <= 4 ("chain_bf16<16,10,8,1>+gauss"), else as one more launch ("...;gauss").  There is no
 * split-k family: the ctx's scratch buffer is not used, nothing allocates or synchronises, and the first call may happen inside a stream
 * capture.  No atomics: the same bits on every run.  The route queries follow the f32 ones' contract (the instantiation's name, "none"
 * for M = 0, NULL where the shapes are refused); the fit rule is the f32 chains', in one place (chain_fit() of csrc/rover_mlp.hip). */
ROVER_API int rover_mlp_chain_forward_bf16(rover_ctx *ctx, const float *x, int64_t x_stride, int32_t M, int32_t K0, int32_t n_layers,
                                           const float *const *weights, const float *const *biases, const int32_t *widths,
                                           const int32_t *activations, float *y, int64_t y_stride, void *stream);
ROVER_API int rover_mlp_chain_act_bf16(rover_ctx *ctx, const float *x, int64_t x_stride, int32_t M, int32_t K0, int32_t n_layers,
                                       const float *const *weights, const float *const *biases, const int32_t *widths,
                                       const int32_t *activations, float *y, int64_t y_stride, const rover_gauss_head *head,
                                       void *stream);
ROVER_API const char *rover_mlp_chain_route_bf16(int32_t M, int32_t K0, int32_t n_layers, const int32_t *widths,
                                                 const int32_t *activations);
ROVER_API const char *rover_mlp_chain_act_route_bf16(int32_t M, int32_t K0, int32_t n_layers, const int32_t *widths,
                                                     const int32_t *activations, const rover_gauss_head *head);
/* rover_linear_forward_bf16: ONE Layer under the same contract — x and W rounded to bf16 as they are read, exact products summed in
 * f32 in a fixed order, f32 bias and activation, f32 output.  Whoever reads y next rounds it as it reads, so a net run layer by layer
 * through this call has the arithmetic of a chain ("rounded before the next layer reads it").  Parameters and refusals are
 * rover_linear_forward's (N <= 256, K >= 0, rows at a stride); no split-k, no scratch, capturable.  rover_linear_route_bf16:
 * "linear_bf16<128,128>" (128 rows x 128 columns per workgroup), "none" for M = 0, NULL where refused. */
ROVER_API int rover_linear_forward_bf16(rover_ctx *ctx, const float *x, int64_t x_stride, int32_t M, int32_t K, const float *weight,
                                        const float *bias, int32_t N, int32_t activation, float *y, int64_t y_stride, void *stream);
ROVER_API const char *rover_linear_route_bf16(int32_t M, int32_t K, int32_t N);
/* Host only (no ctx, no device): out[i] = the bf16 rounding of in[i] as an f32 — the one definition the kernels share. */
ROVER_API int rover_bf16_round(const float *in, int64_t n, float *out);

/* ---- Operand rules: the array arguments of the learning entry points ------------------------------------------------------------------ */
/* rover_gae, rover_linear_backward, rover_linear_dgrad, rover_ppo_loss, rover_optim_create / _step, rover_gru_cell / _bf16 / _train,
 * rover_gru_cell_backward, rover_gated_sum / _backward, rover_obs_noise, rover_obs_occlusion and rover_scaler_update / _apply check their
 * arrays by one set of
 * rules (csrc/rover_operands.h).  An operand is (pointer, row stride in elements, rows, cols); a one-row array has no stride argument.
 * An operand the call does not look at (an input no requested output needs, stats_in outside NORMALIZE_GIVEN, ...) is not checked at all,
 * whatever its pointer and stride; an optional operand given as NULL neither.  For the others, in this order, each rule over all operands
 * before the next; the first breach is ROVER_E_INVALID before any launch, nothing is written, and rover_last_error names the operand(s):
 *   1. a required operand with elements is NULL;
 *   2. a row stride is outside cols .. 2^40 (where an entry point says so a stride of 0 is legal too: one row serves every row);
 *   3. a pointer is not aligned as the entry point requires;
 *   4. "extent too large": rows x stride x element size passes 2^62 bytes, or the array would pass the end of the address space — so no
 *      extent the later rules compute can wrap;
 *   5. a written operand overlaps a read one ("<b> overlaps <a>", a before b in the entry point's argument order).  Where an entry point
 *      says a pair may be the same array it may coincide exactly, same pointer and same stride; any other overlap of the two is refused
 *      ("... without being the same array");
 *   6. two written operands overlap.  State an entry point updates, and the few small records noted below, count as written.
 * Operands that are only read may overlap each other.  Shape, range and scalar checks come first, and an empty call (M = 0, E = 0)
 * returns ROVER_OK before any pointer is asked for, unless its entry says otherwise.
 * The ctx is looked at last: with a NULL ctx every refusal above is still made and reported through rover_last_error(NULL), and a call
 * that keeps every rule is refused with "<entry>: null ctx" (ROVER_E_INVALID). */

/* ---- the rollout side of PPO: returns and advantages of a stored rollout in one pass (skrl's compute_gae inside PPO._update) -------- */
/* The reference trains through skrl: RandomMemory(memory_size=60) (train.py:82), rollouts 60, discount_factor 0.99, lambda 0.95
 * (cfg/trainSKRL/RoverPPOSKRL.yaml:12-16).  skrl is no part of this repository: the semantics are restated from a reading of skrl
 * 0.10 / 1.x, not verified against an installed copy, and are this project's definition.  With rewards, values [T, E] f32, dones [T, E]
 * u8 (a torch.bool's storage, non-zero = done), last_values [E]:
 *   adv = 0 per env;  for t = T-1 .. 0:  nv = values[t+1] (t = T-1: last_values)
 *       adv = rewards[t] - values[t] + gamma (dones[t] ? 0 : 1) (nv + lam adv);  A[t] = adv
 *   returns = A + values;   advantages = (A - mean(A)) / (std(A) + 1e-8), mean and UNBIASED std over all T E elements
 * NaN and Inf get no special handling: they propagate as the formula says (a done flag multiplies by 0).  Time-limit bootstrapping
 * (rewards += gamma values truncated at record time) is the caller's one elementwise line, not part of the kernel.  The weight update
 * that consumes returns and advantages is rover_ppo_loss + rover_linear_backward below (learning/ppo.py drives them).
 * Every [T, E] array is (device pointer, TIME stride in elements >= E); the env stride is 1, so skrl-shaped [T, E, 1] tensors and
 * padded buffers are read and written in place.  returns may alias values (same pointer and stride); advantages aliases nothing the
 * call reads.
 * normalize: ROVER_GAE_RAW — advantages = A; ROVER_GAE_NORMALIZE — normalised with this call's own moments (needs T E >= 2: the
 * unbiased std of one element is NaN, which the call refuses rather than emits); ROVER_GAE_NORMALIZE_GIVEN — normalised with stats_in.
 * stats_out (optional, device double[3]) receives (count, mean, M2 = sum of squared deviations) of this call's RAW A in every mode;
 * stats_in (device double[3], ROVER_GAE_NORMALIZE_GIVEN only) is read by the kernel when it runs.  That is how shards normalise with
 * the global moments: each rank runs RAW + stats_out, the triples are combined (rover_combine_moments, or the same expression on
 * device tensors) and every rank runs NORMALIZE_GIVEN with the result.
 * returns[:, e] and the raw A[:, e] depend on env e's column alone — not on E, nor on how the envs are cut into shards: two
 * half-shards reproduce the whole bit for bit.  The moments are f64, merged from per-block partials in a fixed order with Chan's
 * formula: no floating-point atomics, the same inputs give the same bits on every run.
 * The call allocates nothing and does not synchronise (the partials' buffer belongs to the ctx since rover_create): it can be captured
 * in a graph.  Calls of one ctx run on ONE stream at a time.  Launches: one (RAW or NORMALIZE_GIVEN without stats_out), else two (the
 * scan, then the kernel that merges the partials, writes stats_out and normalises); none for E = 0 (ROVER_OK).
 * ROVER_E_INVALID before any launch: T outside 1 .. 4096, E < 0, T E >= 2^31, an unknown normalize, NORMALIZE with T E < 2, and the
 * operand rules: stats_out is optional, returns and values may be the same array, stats_in counts under NORMALIZE_GIVEN only and then
 * stands clear of every array and of stats_out like a written operand. */
#define ROVER_GAE_RAW             0
#define ROVER_GAE_NORMALIZE       1
#define ROVER_GAE_NORMALIZE_GIVEN 2
typedef struct {
    int32_t T, E;                 /* 1 <= T <= 4096 time steps, E >= 0 envs, T E < 2^31                                         */
    float gamma, lam;             /* discount_factor, lambda                                                                    */
    const float *rewards;   int64_t rewards_stride;
    const float *values;    int64_t values_stride;
    const uint8_t *dones;   int64_t dones_stride;
    const float *last_values;     /* [E] the critic's value of the state after the last stored step                             */
    float *returns;         int64_t returns_stride;
    float *advantages;      int64_t advantages_stride;
    int32_t normalize;            /* ROVER_GAE_*                                                                                */
    double *stats_out;            /* optional device [3]                                                                        */
    const double *stats_in;       /* device [3], required with ROVER_GAE_NORMALIZE_GIVEN                                        */
} rover_gae_desc;
ROVER_API int rover_gae(rover_ctx *ctx, const rover_gae_desc *d, void *stream);
/* Host only (no ctx, no device): out[3] = the moments (count, mean, M2) of the union of two disjoint samples with moments a[3], b[3] —
 * Chan, Golub & LeVeque's pairwise update, the one the kernels run.  An empty side (count 0) leaves the other unchanged; out may be a or b. */
ROVER_API int rover_combine_moments(const double *a, const double *b, double *out);

/* ---- the learner side of PPO: the backward of one Layer and the minibatch loss (skrl's PPO._update on torch autograd) --------------- */
/* The reference trains with skrl's PPO_DEFAULT_CONFIG overridden by cfg/trainSKRL/RoverPPOSKRL.yaml (learning_epochs 4, mini_batches 60,
 * learning_rate 1e-4, grad_norm_clip 1.0, ratio_clip 0.2, value_clip 0.2, clip_predicted_values True, entropy_loss_scale 0,
 * value_loss_scale 1, kl_threshold 0.008; no preprocessors, no scheduler).  skrl is not installed: everything below is restated from a
 * reading of skrl 1.x and of ATen's backward formulas (derivatives.yaml: leaky_relu / tanh / relu / elu backward from the result, clamp,
 * minimum), and is this project's definition.
 *
 * rover_linear_backward: the backward of y = act(x W^T + b) as rover_linear_forward computes it.  x [M, K], y [M, N] (the layer's
 * post-activation OUTPUT as the forward wrote it) and dy [M, N] are (device pointer, row stride in elements); weight [N][K] contiguous.
 *   dz = dy * act'(y), the derivative taken from y alone:  none 1;  LeakyReLU y > 0 ? 1 : 0.01f;  ReLU y > 0 ? 1 : 0;
 *                                                           Tanh 1 - y*y;  ELU y > 0 ? 1 : y + 1
 *   dx [M, K] = dz W   (pointer, row stride)      dweight [N][K] = dz^T x   (contiguous)      dbias [N] = column sums of dz
 * Each output is optional (NULL: not computed).  Inputs an output does not need may be NULL: y with activation 0, x without dweight,
 * weight without dx.  N <= 256 always, K <= 256 when dx is wanted (the first encoder layers, K = 634 / 1 112, never need dx); K = 0 is
 * legal (dweight is empty, dbias is still written); M = 0 writes zeros to dweight and dbias.  NaN and Inf propagate as the formulas say.
 * dweight / dbias: an f32-input MFMA reduction over M, cut into splits whose f32 partials go to a scratch buffer of the ctx and are
 * added in the order of the splits — no floating-point atomics, the same inputs give the same bits on every run.  The scratch follows
 * the chain entry points' rule: it grows on demand (the first call of a size outside a stream capture), one stream per ctx at a time.
 * ROVER_E_INVALID before any launch: M < 0, K < 0, N outside 1 .. 256, K > 256 with dx, an unknown activation, and the operand rules: y
 * counts only with an activation, x only for dweight with K > 0, weight and dx only for dx with K > 0; dbias is optional.  M = 0 needs
 * no pointer, but the strides of dy, y, x and dx are still checked. */
ROVER_API int rover_linear_backward(rover_ctx *ctx, const float *x, int64_t x_stride, const float *y, int64_t y_stride, const float *dy,
                                    int64_t dy_stride, int32_t M, int32_t K, const float *weight, int32_t N, int32_t activation, float *dx,
                                    int64_t dx_stride, float *dweight, float *dbias, void *stream);
/* What rover_linear_backward would launch — host only, like rover_linear_route: "wgrad<NT,NW>/S" (linear_wgrad_kernel<NT, NW> over S
 * splits of M, merged when S > 1), followed by ";dgrad<NT,NW>" (";dgrad<NT,4>x2": two column halves) when want_dx and K > 0; "zero" for
 * M = 0; NULL where the call would be refused.  The split rule (csrc/rover_train.hip linear_backward_route): M >= 8 192 — NW = 4, NT =
 * the N tiles of 32 in groups of at most 3, S = M / 1 024 rounded down to a power of two, at most 64; below — NW = NT = 1, S = 1 / 2 / 4
 * / 8 from 0 / 128 / 256 / 512 rows.  The pointer is valid until the calling thread's next route query. */
ROVER_API const char *rover_linear_backward_route(int32_t M, int32_t K, int32_t N, int32_t want_dx);

/* rover_linear_dgrad: the dx of rover_linear_backward alone, for ANY N >= 1 and K >= 1: dx [M, K] = (dy * act'(y)) W with W [N][K]
 * contiguous, the same activations and derivative rules, the same kernel (a reduction over N in 32-wide slabs, one accumulator per
 * element in the order of n) on a route without the 256 limits — the recurrent student's layers need it (K = 300, N = 900 / 1 746).
 * y counts only with an activation.  M = 0 launches nothing.  ROVER_E_INVALID before any launch: the shapes, an unknown activation, the
 * operand rules.  Allocates nothing, does not synchronise, no atomics, capturable. */
ROVER_API int rover_linear_dgrad(rover_ctx *ctx, const float *y, int64_t y_stride, const float *dy, int64_t dy_stride, int32_t M, int32_t K,
                                 const float *weight, int32_t N, int32_t activation, float *dx, int64_t dx_stride, void *stream);
/* What rover_linear_dgrad would launch — host only: "dgrad<NT,NW>xNY" (linear_dgrad_kernel<NT, NW> on NY column tiles of dx): below
 * 65 536 rows NT = NW = 1; from there NW = 4 and NT = 2 (1 when K <= 32).  "none" for M = 0; NULL where the call would be refused
 * (M < 0, N < 1, K < 1 or more than 65 535 column tiles).  The pointer is valid until the calling thread's next route query. */
ROVER_API const char *rover_linear_dgrad_route(int32_t M, int32_t K, int32_t N);

/* rover_ppo_loss: skrl's PPO minibatch loss at the nets' outputs, and its gradients with respect to them.  With ls', sigma and
 * lp_i = sum_j [...] exactly as the rover_gauss_head comment defines them for taken actions a (reduction: ROVER_REDUCE_SUM only, the
 * reference's), c = ratio_clip, vc = value_clip:
 *   r_i = exp(lp_i - old_log_prob_i)                      kl = mean((r - 1) - (lp - old_log_prob))
 *   policy_loss  = -mean(min(adv r, adv clamp(r, 1 - c, 1 + c)))
 *   v'           = old_values + clamp(value - old_values, -vc, vc) if clip_predicted_values, else value
 *   value_loss   = value_loss_scale mean((returns - v')^2)
 *   entropy_loss = -entropy_loss_scale * mean over M and A of (0.5 + 0.5 log 2pi + ls'_j)
 * and L = policy_loss + value_loss + entropy_loss.  The gradients are autograd's for those expressions, its tie rules included (a min
 * tie splits the gradient in half, clamp passes the gradient on the closed interval), [.] = 1 if true else 0:
 *   dL/dr_i     = -(adv_i / M) [1 - c <= r_i <= 1 + c  or  adv_i r_i < adv_i clamp(r_i)]
 *   d_mean_ij   = dL/dr_i r_i (a_ij - mean_ij) / sigma_j^2
 *   d_log_std_j = [min <= ls_j <= max, or no clip_log_std] (sum_i dL/dr_i r_i ((a_ij - mean_ij)^2 / sigma_j^2 - 1) - entropy_loss_scale / A)
 *   d_value_i   = value_loss_scale (2 / M) (v'_i - returns_i) [|value_i - old_values_i| <= vc, or no clipping]
 * stats (device double[4]) = (policy_loss, value_loss, entropy_loss, kl).  The per-row terms are f32 (the order of operations is
 * written out in csrc/rover_train.hip); the sums over M are f64, merged from per-block partials in a fixed order as rover_gae merges its
 * moments: the same inputs give the same bits.  NaN and Inf propagate as the formulas say.
 * The partials' buffer belongs to the ctx since rover_create: the call allocates nothing, does not synchronise and can be captured.
 * Launches: one, plus the merge; none for M = 0 (ROVER_OK).  One stream per ctx at a time.
 * ROVER_E_INVALID before any launch: A outside 1 .. 16, M < 0, a reduction other than ROVER_REDUCE_SUM, min_log_std > max_log_std with
 * clip_log_std, a negative (or NaN) ratio_clip / value_clip, and the operand rules (every pointer is required; d_mean, d_value,
 * d_log_std and stats are written). */
typedef struct {
    int32_t M, A;                 /* rows of the minibatch; 1 .. 16 action components                                            */
    const float *mean;      int64_t mean_stride;       /* [M, A] the actor's output ("mean_actions")                            */
    const float *log_std;                               /* [A] log_std_parameter                                                 */
    const float *actions;   int64_t actions_stride;    /* [M, A] the actions taken in the rollout                               */
    const float *old_log_prob, *advantages;             /* [M]                                                                   */
    const float *value, *old_values, *returns;          /* [M] the critic's output; the rollout's values; rover_gae's returns    */
    int32_t clip_log_std;  float min_log_std, max_log_std;       /* as in rover_gauss_head                                      */
    int32_t reduction;            /* ROVER_REDUCE_SUM                                                                            */
    float ratio_clip, value_clip;
    int32_t clip_predicted_values;
    float entropy_loss_scale, value_loss_scale;
    float *d_mean;          int64_t d_mean_stride;     /* [M, A] out */
    float *d_value;                                     /* [M] out    */
    float *d_log_std;                                   /* [A] out    */
    double *stats;                                      /* [4] out    */
} rover_ppo_loss_desc;
ROVER_API int rover_ppo_loss(rover_ctx *ctx, const rover_ppo_loss_desc *d, void *stream);

/* ---- the optimiser step: gradient-norm clip + Adam over a list of tensors, with the KL early stop decided on the device ------------ */
/* torch.nn.utils.clip_grad_norm_(params, clip) followed by torch.optim.Adam.step() (no weight decay, no amsgrad, one step counter for
 * all tensors) over n_tensors f32 tensors in two launches, restated from a reading of torch 2.x; this is the project's definition.
 *
 * rover_optim_plan — host only, no ctx, no device, a pure function: the chunks both kernels walk, one workgroup per chunk.  The tensors
 * are cut in tensor order, then element order, into chunks of one fixed length (a constant of the library, csrc/rover_internal.h
 * OPTIM_CHUNK; callers read it off the plan of one long tensor and never assume a value); the last chunk of a tensor is shorter, a
 * tensor of numel 0 yields no chunk.  *n_chunks (required) receives the count; chunks (optional) receives the records when capacity
 * >= the count.  ROVER_E_INVALID (rover_last_error(NULL)): numel or n_chunks NULL, n_tensors outside 1 .. 256, a negative numel, total
 * elements >= 2^31, chunks given with capacity < the count (or capacity < 0). */
typedef struct { int32_t tensor, first, length; } rover_optim_chunk;      /* elements [first, first + length) of tensor `tensor` */
ROVER_API int rover_optim_plan(int32_t n_tensors, const int64_t *numel, rover_optim_chunk *chunks, int64_t capacity, int64_t *n_chunks);

/* rover_optim_create: binds a tensor list and its state to a handle of the ctx.  params / grads / numel are HOST arrays of n_tensors
 * entries (device pointers to contiguous f32 tensors, 4-byte aligned; a pointer may be NULL where numel is 0); they are read during
 * the call only.  The state belongs to the CALLER, lives on the device and must outlive the handle: exp_avg and exp_avg_sq (flat,
 * sum(numel) floats each, tensor i at offset numel[0] + .. + numel[i-1]; zeroed by the caller before the first step), step (one
 * int64: Adam's step count, 0 at first) and stopped (one int32 latch, 0 = open).  The ctx owns only the device chunk table, one f64
 * partial per chunk and a 16-byte record per handle, all allocated HERE (never in the step) and freed by rover_optim_destroy or by
 * rover_destroy.  *handle >= 0.  A destroyed handle's number may be given out again.
 * ROVER_E_INVALID before anything is allocated: a NULL descriptor / handle / array, n_tensors outside 1 .. 256, a negative numel,
 * total elements >= 2^31; the operand rules for the state (step 8-byte aligned, stopped, exp_avg and exp_avg_sq 4-byte aligned, all
 * written; the moments have no element when the total is 0); and, by the same bounded extents, for the lists: a NULL or misaligned
 * params[i] / grads[i] with numel[i] > 0, a parameter overlapping its own or another tensor's gradient, another parameter or the state,
 * a gradient overlapping the state.  (Two gradients may overlap: they are only read.)  The ctx is needed only to keep the handle.
 * rover_optim_destroy: ROVER_E_INVALID for a handle that is not live. */
typedef struct {
    int32_t n_tensors;
    float *const *params;         /* host [n_tensors] of device pointers */
    const float *const *grads;    /* host [n_tensors] of device pointers */
    const int64_t *numel;         /* host [n_tensors]                    */
    float *exp_avg, *exp_avg_sq;  /* device, sum(numel) floats each      */
    int64_t *step;                /* device [1]                          */
    int32_t *stopped;             /* device [1]                          */
} rover_optim_desc;
ROVER_API int rover_optim_create(rover_ctx *ctx, const rover_optim_desc *d, int32_t *handle);
ROVER_API int rover_optim_destroy(rover_ctx *ctx, int32_t handle);

/* rover_optim_step: one gated step.  Exactly two launches; the call allocates nothing, does not synchronise and can be captured in a
 * graph.  One stream per ctx at a time, like rover_ppo_loss.  gate (optional, device double[1], e.g. stats + 3 of rover_ppo_loss) and
 * norm_out (optional, device double[1]) are read / written by the kernels when they run.
 * Launch 1, prepare: one workgroup of 256 threads per chunk sums g*g in f64 (exact products; per thread in element order, then a
 *   fixed tree over the lanes, then the waves in order) and stores its partial.  Workgroup 0 evaluates the gate:
 *       if *stopped != 0, or gate is given and *gate > gate_threshold:  *stopped = 1        (a plain >: a NaN gate does not stop,
 *       else:                                                           *step += 1           as float(kl) > threshold on the host)
 *   and leaves the decision and the step count now in force in the handle's record.
 * Launch 2, apply: every workgroup reads the record and returns if stopped: parameters, exp_avg, exp_avg_sq, step and norm_out are
 *   then bit-unchanged.  Otherwise it adds the partials in chunk order (thread i takes i, i + 256, ..., then a fixed tree: the same
 *   order in every workgroup, as rover_gae's finishing kernel merges) and forms in f64, with t = *step after the increment:
 *       norm = sqrt(sum)        coef = grad_norm_clip > 0 ? min(1, grad_norm_clip / (norm + 1e-6)) : 1        (a NaN stays a NaN)
 *       bc1 = 1 - beta1^t       bc2 = 1 - beta2^t       (powers by repeated squaring)
 *   rounds coef, 1 - beta1, beta2, 1 - beta2, lr / bc1, sqrt(bc2) and eps to f32 ONCE and updates every element in f32, one rounding
 *   per written operation, in this order:
 *       g' = g * coef
 *       m  = m + (g' - m) * (1 - beta1)
 *       v  = beta2 * v + ((1 - beta2) * g') * g'
 *       p  = p - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))
 *   norm_out receives norm, the total gradient norm BEFORE clipping.
 * Gradients are READ ONLY: unlike torch's clip_grad_norm_, the clipped gradient g' is not written back.  NaN and Inf propagate as the
 * formulas say.  No floating-point atomics: the same inputs give the same bits on every run, whatever the alignment of the tensors
 * (16-byte loads and stores where a tensor's bases allow, scalar ones otherwise, the same arithmetic in the same order).
 * ROVER_E_INVALID before any launch, in this order: a NULL descriptor, lr < 0 or not finite, beta1 / beta2 outside [0, 1), eps < 0 or
 * not finite, a NaN grad_norm_clip or gate_threshold; the operand rules for gate and norm_out (both optional, 8-byte aligned); a NULL
 * ctx; a handle that is not live; norm_out overlapping a parameter, a gradient, exp_avg, exp_avg_sq, step or stopped of the handle. */
typedef struct {
    double lr, beta1, beta2, eps;
    double grad_norm_clip;        /* <= 0: no clipping                                                          */
    const double *gate;           /* optional device [1]                                                        */
    double gate_threshold;
    double *norm_out;             /* optional device [1]                                                        */
} rover_optim_step_desc;
ROVER_API int rover_optim_step(rover_ctx *ctx, int32_t handle, const rover_optim_step_desc *d, void *stream);

/* ---- the student policy's recurrent block (tasks/utils/learning_by_cheating/student_model.py:42-131; learning/student.py) ---- */
/* rover_gru_cell: ONE layer of torch.nn.GRU for ONE time step in one launch.  This is the project's definition of the cell; gate order
 * r, z, n; w_ih [3H][K], w_hh [3H][H] (nn.GRU's weight_ih_l*, weight_hh_l*), b_ih / b_hh [3H] or NULL (zeros):
 *   r  = sigmoid(x.W_ir^T + b_ir + h.W_hr^T + b_hr)
 *   z  = sigmoid(x.W_iz^T + b_iz + h.W_hz^T + b_hz)
 *   n  = tanh   (x.W_in^T + b_in + r * (h.W_hn^T + b_hn))
 *   h' = (1 - z) * n + z * h
 * evaluated in f32 in this order (the library is built with -ffp-contract=off: one rounding per operation):
 *   s_r = fma-chain over k of x then of h (exact f32 MFMA, v_mfma_f32_32x32x2_f32; one accumulator over K + H), likewise s_z;
 *   s_in over K alone, s_hn over H alone;  sigmoid(v) = 1 / (1 + expf(-v));
 *   r = sigmoid((s_r + b_ir) + b_hr);  z = sigmoid((s_z + b_iz) + b_hz);  n = tanhf((s_in + b_in) + r * (s_hn + b_hn));
 *   h' = (1 - z) * n + z * h   (two products, then their sum).
 * x [M, K], h_in [M, H] and h_out [M, H] are f32 rows at a row stride in floats (column slices of wider tensors will do).
 * reset_mask: optional uint8 [M]; a row with a non-zero byte reads its h_in as zero, in the products and in z * h (an addition to
 * the reference, whose student_loader.act never resets the state; NULL = the reference's behaviour).
 * One workgroup computes a 32-column tile of h' from whole rows of h_in that other workgroups are still reading: h_out may not even
 * be h_in.  M = 0 launches nothing; K = 0 is legal (x and w_ih do not count).  Widths: H = 1 .. 2 097 120 (65 535 tiles of 32 columns),
 * K >= 0; anything else, or a breach of the operand rules (b_ih, b_hh and reset_mask are optional; h_out is the one written operand):
 * ROVER_E_INVALID.  Neither [M, 3H] pre-activation tensor is written to memory.  The call allocates nothing, does not synchronise, uses no atomics (the same inputs give the same bits, and a
 * row's result does not depend on the other rows) and can be captured in a graph. */
ROVER_API int rover_gru_cell(rover_ctx *ctx, const float *x, int64_t x_stride, const float *h_in, int64_t h_in_stride, int32_t M, int32_t K,
                             int32_t H, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                             const uint8_t *reset_mask, float *h_out, int64_t h_out_stride, void *stream);
/* What rover_gru_cell would launch — host only, no ctx: "gru_cell<4>" (128 rows per workgroup) when ceil(M / 128) x ceil(H / 32)
 * workgroups are at least 512, else "gru_cell<1>" (32 rows per workgroup); "none" for M = 0; NULL where the call would refuse the
 * shapes.  Every limit on M, K and H lives behind this query. */
ROVER_API const char *rover_gru_cell_route(int32_t M, int32_t K, int32_t H);

/* rover_gru_cell_bf16: the same cell with bf16 operands in its matrix products and everything else in f32 (precision = "bf16",
 * inference only).  Parameters, shapes, strides, reset_mask, refusals (overlap included), M = 0 and K = 0 are
 * rover_gru_cell's.  The arithmetic — the tests hold the kernel to it:
 *   operands      every element of x, h_in, w_ih and w_hh is rounded to bf16 as it is read for the products (rover_bf16_round: nearest
 *                 even, NaN stays NaN, +-Inf stays +-Inf).  No bf16 copy of the weights or of the state exists anywhere.
 *   products      exact in f32, summed in f32 in a fixed order on v_mfma_f32_16x16x32_bf16: s_r and s_z over K + H, s_in over the x slabs
 *                 alone, s_hn over the h slabs alone.  x and h are each zero-filled to a multiple of 32, so no k-step mixes the two
 *                 (r multiplies s_hn only).
 *   epilogue      rover_gru_cell's, operation for operation, in f32: the f32 biases, sigmoid(v) = 1 / (1 + expf(-v)), tanhf,
 *                 h' = (1 - z) * n + z * h with the UNROUNDED f32 h_in (0 on a reset row).  h_out is f32.
 * The state stays f32 on purpose: with z near 1 the cell is h' = h + (1 - z)(n - h), and a state rounded to 8 significant bits every
 * step would drop every update below 2^-9 |h|.
 * rover_gru_cell_route_bf16 — host only, no ctx: "gru_cell_bf16<128,64>" (128 rows x 64 columns of the hidden state per workgroup, at
 * every batch size); "none" for M = 0; NULL where the call would refuse the shapes. */
ROVER_API int rover_gru_cell_bf16(rover_ctx *ctx, const float *x, int64_t x_stride, const float *h_in, int64_t h_in_stride, int32_t M,
                                  int32_t K, int32_t H, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                                  const uint8_t *reset_mask, float *h_out, int64_t h_out_stride, void *stream);
ROVER_API const char *rover_gru_cell_route_bf16(int32_t M, int32_t K, int32_t H);

/* rover_gru_cell_train: rover_gru_cell with one more output for the backward, gates [M, 4H] at a row stride (>= 4H): r | z | n | q with
 * q = s_hn + b_hn as written above.  h_out has the same bits as rover_gru_cell's on the same inputs (the same kernel body; the extra
 * stores are a template flag of the epilogue, the inference instantiations are unchanged) and the route is rover_gru_cell_route's.
 * gates is a second written operand (required here).  Otherwise as rover_gru_cell. */
ROVER_API int rover_gru_cell_train(rover_ctx *ctx, const float *x, int64_t x_stride, const float *h_in, int64_t h_in_stride, int32_t M,
                                   int32_t K, int32_t H, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                                   const uint8_t *reset_mask, float *h_out, int64_t h_out_stride, float *gates, int64_t gates_stride,
                                   void *stream);

/* rover_gru_cell_backward: the backward of ONE layer for ONE time step in one launch.  dh_above [M, H] is the gradient that arrives at
 * h' from the layer above (or from the heads), dh_next [M, H] the one from the next time step (NULL at the last step: zeros); gates
 * [M, 4H] is what rover_gru_cell_train stored, h_in and reset_mask what it read.  With g = dh_above + dh_next and h = h_in, read as 0 on
 * a reset row, every line one f32 rounding in this order:
 *   d_n = g * (1 - z);   a_n = d_n * (1 - n * n)
 *   d_z = g * (h - n);   a_z = d_z * (z * (1 - z))
 *   d_r = a_n * q;       a_r = d_r * (r * (1 - r))
 *   dgi [M, 3H] = [a_r | a_z | a_n]          (the gradient at x.W_ih^T + b_ih)
 *   dgh [M, 3H] = [a_r | a_z | a_n * r]      (the gradient at h.W_hh^T + b_hh)
 *   dh_in [M, H] = (sum over j < 3H of dgh_j * w_hh[j][.], exact f32 MFMA, one accumulator in the order of j) + g * z
 * and dh_in is 0 on a reset row: nothing flows across an episode boundary.  The weight gradients are the caller's reductions over all
 * time steps (dW_ih = dgi^T x, dW_hh = dgh^T h with reset rows of h zeroed: rover_linear_backward), and dx = dgi W_ih is one
 * rover_linear_dgrad.  dgh is formed from gates while the product stages it; the workgroups of one column tile store dgi and dgh.
 * All arrays are f32 rows at a row stride in floats.  Operand rules: dh_next and reset_mask are optional; dgi, dgh and dh_in are
 * written.  M = 0 launches nothing.  Allocates nothing, does not synchronise, no atomics (the same inputs give the same bits, and a
 * row's result does not depend on the other rows), capturable. */
ROVER_API int rover_gru_cell_backward(rover_ctx *ctx, const float *dh_above, int64_t dh_above_stride, const float *dh_next,
                                      int64_t dh_next_stride, const float *gates, int64_t gates_stride, const float *h_in,
                                      int64_t h_in_stride, const uint8_t *reset_mask, const float *w_hh, int32_t M, int32_t H, float *dgi,
                                      int64_t dgi_stride, float *dgh, int64_t dgh_stride, float *dh_in, int64_t dh_in_stride, void *stream);
/* What rover_gru_cell_backward would launch — host only, no ctx: "gru_bwd<4>" (128 rows per workgroup) when ceil(M / 128) x ceil(H / 32)
 * workgroups are at least 512, else "gru_bwd<1>"; "none" for M = 0; NULL where the call would refuse the shapes (M < 0, H outside
 * 1 .. 2 097 120).  Every limit on M and H lives behind this query. */
ROVER_API const char *rover_gru_cell_backward_route(int32_t M, int32_t H);

/* rover_gated_sum: out = add + mul * sigmoid(pre), elementwise over [M, N] in one launch (sigmoid as above; the product, then the sum).
 * The belief x_b + l_e * sigmoid(x_a) (student_model.py:79-85; x_a arrives LeakyReLU'd: ga's last Layer has its activation before the
 * nn.Sigmoid) and the decoder's decoded + e * sigmoid(gate) (:121-131).  All four arrays are f32 rows at a row stride in floats; an
 * INPUT's stride may be 0 (its one row serves every output row), out's may not; M N < 2^38.  out may not be an input, not even
 * exactly (operand rules).  M = 0 launches nothing.  Allocates nothing, does not synchronise, capturable. */
ROVER_API int rover_gated_sum(rover_ctx *ctx, const float *add, int64_t add_stride, const float *mul, int64_t mul_stride, const float *pre,
                              int64_t pre_stride, int32_t M, int32_t N, float *out, int64_t out_stride, void *stream);

/* rover_gated_sum_backward: for out = add + mul * sigmoid(pre) and d_out [M, N], with s = sigmoid(pre) as the forward evaluates it:
 *   d_mul = d_out * s          d_pre = (d_out * mul) * (s * (1 - s))          (d_add is d_out itself and is not written)
 * Each output is optional (NULL).  mul and pre may have a row stride of 0 as in the forward; d_out, d_mul and d_pre are per row (stride
 * >= N): summing the rows of an output whose input was one shared row is the caller's job.  mul counts only for d_pre.  With neither
 * output the call returns ROVER_OK at once; otherwise the operand rules hold.  M = 0 launches nothing.  Allocates nothing, does not synchronise, capturable. */
ROVER_API int rover_gated_sum_backward(rover_ctx *ctx, const float *d_out, int64_t d_out_stride, const float *mul, int64_t mul_stride,
                                       const float *pre, int64_t pre_stride, int32_t M, int32_t N, float *d_mul, int64_t d_mul_stride,
                                       float *d_pre, int64_t d_pre_stride, void *stream);

/* ---- exteroception noise: the sensor model between the task's observation and a policy (learning/noise.py) ------------------------- */
/* The reference's authors tried Gaussian noise, dropout, a constant offset and zeroed columns on the observation (tasks/rover.py:326-329,
 * commented out) and carry is_evaluation_with_noise / max_noise_dev = 0.2; what follows is this project's definition.  The task's own
 * observation stays clean: the call maps in [M, F] to out [M, F] (f32 rows at a row stride in floats).
 * Columns [0, first) — the proprioceptive ones — are copied bit for bit.  For heightmap column c = col - first, 0 <= c < C = F - first,
 * global row g = row_offset + r, call counter t = step + *step_dev (mod 2^64; step_dev NULL: step alone) and column pair p = c / 2:
 *   w    = philox(counter = (g, t & 0xffffffff, t >> 32, 0x60000000 | p), key = (seed & 0xffffffff, seed >> 32))
 *   eps  = the head's Box-Muller pair from (w[0], w[1]) exactly as the rover_gauss_head comment writes it: eps[2 p] the cos branch,
 *          eps[2 p + 1] the sin branch
 *   u_c  = w[2] >> 8 for even c, w[3] >> 8 for odd c                                     (a 24-bit integer)
 *   e    = episode ? episode[r] : 0                                                       (int64, taken mod 2^64)
 *   wo   = philox(counter = (g, e & 0xffffffff, e >> 32, 0x70000000), key as above)
 *   eo   = the cos branch of the pair from (wo[0], wo[1])     (one draw per env and episode: the same for every column and every call)
 *   s    = row_scale ? row_scale[r] : 1.0f
 *   v    = (in[r, col] + (sigma_offset * s) * eo) + (sigma_point * s) * eps_c            f32, one rounding per written operation
 *   out[r, col] = u_c < thr ? drop_value : v,      thr = (uint32) llrint(dropout * 2^24), computed once on the host
 * (rover_obs_noise_threshold returns that thr: 0 for dropout 0 — nothing dropped —, 2^24 for 1 — everything.)
 * Streams: word 3 of the counter is 0 in the goal / yaw draws and 0x50000000 | pair in the action noise, so the four streams are disjoint
 * under one seed.  A value depends on (seed, t, g, c), on e and on the row's own inputs — not on M, not on a stride, not on how a batch is
 * sharded (a shard passes its env_offset as row_offset), not on eager execution against graph replay.  The library never writes
 * *step_dev or episode: the caller advances them with work enqueued on the same stream after the call, as for act().
 * A sigma of 0 switches its term off: the term is +0.0f and its draw is not made, whatever s is.  With sigma_point = sigma_offset = 0
 * and dropout = 0 the call therefore computes (in + 0.0f) + 0.0f: out equals in, except that -0.0f becomes +0.0f (a NaN stays a NaN).
 * sigma_point = 0 with dropout > 0 still takes u_c from words 2 and 3 of the same Philox call.  Everywhere else the results are the
 * written formula's, bit for bit, on both of the kernel's paths: a column pair moves as one 8-byte load and one 8-byte store when first
 * and both strides are even and both bases 8-byte aligned (the native obs: first 4, stride 1 750), as two scalars otherwise.
 * One launch (csrc/rover_noise.hip); plain vector loads and stores, no atomics.  The call allocates nothing, does not synchronise and can
 * be captured in a graph; one stream per ctx at a time.  M = 0 or F = 0: ROVER_OK, no launch.  out may be exactly in (same pointer and
 * stride): the in-place form, which leaves columns [0, first) alone.
 * ROVER_E_INVALID before any launch: a NULL descriptor; M < 0 or F < 0; first outside 0 .. F; C > 2^21; a negative or non-finite sigma;
 * dropout outside [0, 1] or NaN; a non-finite drop_value; row_offset < 0 or row_offset + M > 2^32; and, unless M = 0 or F = 0, the
 * operand rules: row_scale, episode and step_dev are optional, out and in may be the same array.  An empty call still wants a ctx. */
typedef struct {
    const float *in;        int64_t in_stride;     /* [M, F]                                                                     */
    float *out;             int64_t out_stride;    /* [M, F]; may be exactly in                                                   */
    int32_t M, F, first;                           /* first: the number of leading columns left alone, 0 .. F                      */
    float sigma_point, sigma_offset;               /* per-element and per-episode standard deviations, >= 0                        */
    double dropout;                                /* probability of a column reading drop_value, 0 .. 1                           */
    float drop_value;
    const float *row_scale;                        /* optional device [M]: scales both sigmas of its row                           */
    const int64_t *episode;                        /* optional device [M]: the row's episode count, keys the offset draw           */
    uint64_t seed, step;
    const uint64_t *step_dev;                      /* optional device [1], added to step when the kernel runs                      */
    int64_t row_offset;                            /* global row of row 0: >= 0, row_offset + M <= 2^32                            */
} rover_obs_noise_desc;
ROVER_API int rover_obs_noise(rover_ctx *ctx, const rover_obs_noise_desc *d, void *stream);
/* Host only (no ctx, no device): *thr = (uint32) llrint(dropout * 2^24); ROVER_E_INVALID for a NULL thr or dropout outside [0, 1]. */
ROVER_API int rover_obs_noise_threshold(double dropout, uint32_t *thr);

/* ---- line-of-sight occlusion: which heightmap columns a mast camera cannot see (learning/noise.py:HeightmapOcclusion) --------------- */
/* The task's heightmap is cast straight down from 3 cm above the ground, so it sees behind every rock; a camera on a mast does not.  The
 * reference has no camera model (tasks/utils/camera/rover_depth.py is a vestige of one); what follows is this project's definition.  The
 * task's own observation stays clean.  The library is built with -ffp-contract=off: every operation below is ONE f32 operation with one
 * IEEE rounding, in the written order; / and sqrtf are the correctly rounded ones (as cell_coord of rover_height.h relies on).
 * Configuration (rover_set_occlusion stores it in the ctx): camera[3], the camera in the body frame (forward, left, up; metres); step > 0,
 * the spacing of the samples along a sight line (metres); clearance, by how much the ground must rise above the sight line to hide
 * (metres); max_steps in 2 .. 4096, the most intervals a sight line is cut into; miss > 0, in observation units: a column at or beyond it
 * holds the clipped 11.0 m sentinel (clipObservations) and has no point to ask about.
 * Per call: row r, heightmap column c, 0 <= c < C = Ns + Nd; point j = c < Ns ? sparse_idx[c] : dense_idx[c - Ns]; body point b = the
 * three f64 coordinates of points[j] (rover_set_distribution), each rounded to f32 once on the host (column 0 is forward); pose
 * p = pos3[r], q = quat4[r] = (w, x, y, z), used as given and not normalised.
 *   r00 = 1 - 2 (y y + z z)   r01 = 2 (x y - w z)       r02 = 2 (x z + w y)
 *   r10 = 2 (x y + w z)       r11 = 1 - 2 (x x + z z)   r12 = 2 (y z - w x)
 *   r20 = 2 (x z - w y)       r21 = 2 (y z + w x)       r22 = 1 - 2 (x x + y y)
 *   rot(v)_i = (r_i0 v0 + r_i1 v1) + r_i2 v2
 *   Cam = p + rot(camera)      S = p + rot(b)      D = (-r02, -r12, -r22)        (the ray of camera.py:196-212: body ZYX rotation, rover "down")
 *   v = clean[r, first + c];   if !(|v| < miss): visible                          (a NaN is visible too)
 *   d = 2 v (exact);           T_i = S_i + d D_i                                  (the point the ray cast measured: obs = distance / 2)
 *   dx = Tx - Cam_x, dy = Ty - Cam_y, dz = Tz - Cam_z
 *   L = sqrtf(dx dx + dy dy);  u = ceilf(L / step);  n = u < (float) max_steps ? (int) u : max_steps    (a NaN u: max_steps);  n <= 1: visible
 *   for k = 1 .. n - 1:  t = (float) k / (float) n
 *        h = the heightfield at (Cam_x + t dx, Cam_y + t dy), read exactly as rover_sample_height reads it (clamp, round half to even,
 *            node, times vertical_scale; option cell_index_mode applies)
 *        hidden if  h > (Cam_z + t dz) + clearance                                (a NaN height never hides, nor does a NaN sight line)
 *   out[r, first + c] = hidden ? drop_value : in[r, first + c];   columns [0, first) are copied bit for bit when out != in
 * Three arrays, on purpose: clean is the task's clean observation and gives the geometry; in is what a visible column is copied from — it
 * may be clean itself, or the output of rover_obs_noise on it —; out may be exactly in (same pointer and stride), which leaves columns
 * [0, first) alone.  The composition is rover_obs_noise(clean -> x) followed by rover_obs_occlusion(clean, x -> x): a hidden column reads
 * exactly drop_value.
 * Optional outputs: hidden_u8 [M, C] at a row stride in bytes, 1 = hidden, 0 otherwise, every column written; target3 [M, C, 3] dense,
 * the point T — for a column that is visible by the miss test (no T exists) the three floats are LEFT UNWRITTEN.
 * The result depends on the row's own inputs only: not on M, a stride, how a batch is sharded (a shard passes its own slices of pos3 and
 * quat4), the order in which threads take columns, or eager execution against graph replay.
 * Two routes compute the same bits (option "occlusion_route"): 0 marches the columns in obs order and reads every sample's node; 1 takes
 * the columns in the order of rover_occlusion_order (far first, so that a wave's lanes march about equally long) and first asks a table
 * of the maxima of 8 x 8-node tiles: where tilemax <= (Cam_z + t dz) + clearance the node cannot hide (h <= tilemax) and is not read.
 * The test is conservative, so the mask is the plain march's by construction.  The default is 1.
 * One launch (csrc/rover_occlusion.hip); plain vector loads and stores, no atomics.  The call allocates nothing, does not synchronise and
 * can be captured in a graph.  M = 0 or F = 0: ROVER_OK, no launch.
 * ROVER_E_INVALID before any launch (the descriptor is checked before the ctx is looked at, as for rover_obs_noise): a NULL descriptor;
 * M < 0 or F < 0; first outside 0 .. F; a non-finite drop_value; and, unless M = 0 or F = 0, the operand rules: pos3, quat4, clean, in
 * and out must be given, hidden_u8 and target3 are optional, out may not overlap clean (nor pos3, quat4 or another output), and may
 * overlap in only by being exactly in.  An empty call still wants a ctx.
 * ROVER_E_STATE: no distribution; no heightfield; no rover_set_occlusion; F - first != Ns + Nd; the distribution or the heightfield was
 * set again after rover_set_occlusion (the message names rover_set_occlusion: call it again).
 * rover_set_occlusion owns what it derives — the columns' f32 body points, the column order and the tile-max table (one small reduction
 * launch over the heightfield; NaN nodes are ignored, as fmaxf ignores them) — under one validity key: the pair of counters that
 * rover_set_distribution and rover_set_heightfield advance.  It needs both set, may synchronise, and refuses with ROVER_E_INVALID a NULL
 * cfg, a non-finite field, step <= 0, max_steps outside 2 .. 4096 and miss <= 0 (all before the ctx is looked at). */
typedef struct {
    float camera[3];                               /* body frame: forward, left, up (m)                                            */
    float step;                                    /* sample spacing along the sight line (m), > 0                                 */
    float clearance;                               /* the ground hides when it is more than this above the sight line (m)          */
    int32_t max_steps;                             /* 2 .. 4096                                                                    */
    float miss;                                    /* observation units, > 0: |clean| >= miss has no point                         */
} rover_occlusion_cfg;
ROVER_API int rover_set_occlusion(rover_ctx *ctx, const rover_occlusion_cfg *cfg);
typedef struct {
    const float *pos3, *quat4;                     /* [M, 3], [M, 4] (w, x, y, z): the poses the observation was made from         */
    const float *clean;     int64_t clean_stride;  /* [M, F]: the clean observation (the geometry)                                 */
    const float *in;        int64_t in_stride;     /* [M, F]: what a visible column is copied from; may be clean                   */
    float *out;             int64_t out_stride;    /* [M, F]; may be exactly in                                                    */
    int32_t M, F, first;                           /* first: the number of leading columns left alone, 0 .. F                      */
    float drop_value;
    uint8_t *hidden_u8;     int64_t hidden_stride; /* optional [M, C] at a row stride in bytes: 1 = hidden                         */
    float *target3;                                /* optional [M, C, 3] dense: T (unwritten where the miss test said visible)     */
} rover_obs_occlusion_desc;
ROVER_API int rover_obs_occlusion(rover_ctx *ctx, const rover_obs_occlusion_desc *d, void *stream);
/* Host only (no ctx, no device): order[0 .. Ns + Nd) = the heightmap columns sorted by the horizontal distance of their body point from
 * the camera, far first, ties in column order (a stable sort).  The key of column c is (bx - camera[0])^2 + (by - camera[1])^2 in
 * double arithmetic on the f32-rounded coordinates.  ROVER_E_INVALID: a NULL points or order, P <= 0, Ns < 0 or Nd < 0, a NULL index list
 * with a count above 0, a NULL or non-finite camera, an index outside [0, P). */
ROVER_API int rover_occlusion_order(const double *points, int32_t P, const int64_t *sparse_idx, int32_t Ns, const int64_t *dense_idx,
                                    int32_t Nd, const float camera[3], int32_t *order);

/* ---- running standard scaler: skrl's RunningStandardScaler for states and values (learning/preprocess.py) ----------------------------- */
/* The reference's train.py imports skrl's RunningStandardScaler (omniisaacgymenvs/train.py); every skrl PPO recipe for Isaac tasks passes
 * it for states and values.  skrl is no dependency: the definition is restated here.  The state is the caller's, all float64 on the
 * device: mean [N] (skrl's running_mean, starts at 0), var [N] (running_variance, starts at 1) and count [1] (current_count, starts at 1:
 * one pseudo-sample).
 *
 * rover_scaler_update: a TRAIN call on x [M, N] (f32 rows at a row stride in floats).  Per column, with mb the mean of the M values
 * and vb their UNBIASED variance M2 / (M - 1) (torch.var), in f64, every line one rounding per operation in the written order:
 *     delta = mb - mean
 *     total = count + M
 *     m2    = (var * count + vb * M) + (((delta * delta) * count) * M) / total
 *     mean  = mean + (delta * M) / total
 *     var   = m2 / total
 *     count = total
 * Exactly two launches (csrc/rover_scaler.hip); the call allocates nothing, does not synchronise and can be captured in a graph; one
 * stream per ctx at a time.  rover_scaler_plan (host only, no ctx, a pure function of (M, N) — never of the device, so the same inputs
 * give the same bits on any machine) splits the rows into n_chunks chunks of rows_per_chunk rows (the last one shorter) and chooses
 *     ROVER_SCALER_NARROW for N <= 8:  rows_per_chunk = 16 384; the 256 threads of a workgroup split the chunk's rows (thread t takes
 *                                      rows t, t + 256, ...: at most 64), column by column, and add their sums in a fixed binary tree;
 *     ROVER_SCALER_WIDE   otherwise:   rows_per_chunk = 32 for M <= 8 192, else 128; a thread owns two neighbouring columns and walks
 *                                      the chunk's rows in order (one 8-byte load per row where x and its stride allow, two scalar loads
 *                                      otherwise: the same additions in the same order);
 *     scratch_bytes = 8 + 24 n_chunks N (caller-owned, 8-byte aligned; its contents mean nothing between calls).
 * Launch 1 leaves per chunk and column (count n, mean, M2) in f64 in scratch, from plain sums: S1 = sum x and S2 = sum x x with x widened
 *   to f64 (each product is exact), mean = S1 / n, M2 = max(S2 - (S1 S1) / n, 0) (a NaN stays a NaN).  Every x enters its sum through at
 *   most a = 136 additions, so with u = 2^-53 and g(k) = k u / (1 - k u):  |dS1| <= g(a) sum|x|,  |dS2| <= g(a) sum x^2,  and
 *   |dM2| <= 4 g(a + 3) sum x^2 per chunk (S1^2 / n <= sum x^2).  It also copies *count into the scratch header.
 * Launch 2 merges the chunks IN CHUNK ORDER in two levels (Chan: tot = n + nk, d = mean_k - mean, f = nk / tot, mean += d f,
 *   M2 = (M2 + M2_k) + (d d)(n f), n = tot — at most 10 roundings per merge, each relative to a quantity bounded by sum x^2, resp.
 *   sum|x| / n for the mean): the chunks form 8 runs of ceil(n_chunks / 8) consecutive chunks (the last runs shorter or empty), one thread
 *   per column and run merges its run's chunks in order, then one thread per column merges the 8 runs in order, empty ones passed over.
 *   It then folds (M, mb, vb = M2 / (M - 1)) into the state as written above with the count from
 *   the header, and writes *count.  Over C chunks:  |d mb| <= (g(a + 1) + 4 C u) sum|x| / M,  |d M2| <= (4 g(a + 3) + 10 C u) sum x^2.
 * skip_if: optional device int32[1], read when launch 2 runs; nonzero: mean, var and count stay bit-unchanged (the device-side KL stop
 * of learning/ppo.py hands the optimiser's `stopped` latch here).  No floating-point atomics: the same inputs give the same bits on
 * every run, whatever the alignment or the row stride of x.
 *
 * rover_scaler_apply: one launch, y [M, N] from x [M, N] and the statistics as they are on the device when the kernel runs, in f32,
 * one rounding per operation in this order, with m = f32(mean), s = sqrtf(f32(var)), e = f32(epsilon), c = f32(clip):
 *     forward:   y = clamp((x - m) / (s + e), -c, +c)
 *     inverse:   y = s * clamp(x, -c, +c) + m
 * clamp is torch.clamp: a NaN stays a NaN in both directions; +-Inf clamps to +-c.  y may be exactly x (same pointer and stride: in
 * place); any other overlap is refused.  M = 0: ROVER_OK, no launch.  Allocates nothing, does not synchronise, capturable.
 *
 * ROVER_E_INVALID before any launch: a NULL descriptor; N outside 1 .. 4096; M < 0 or M N >= 2^31; update with M < 2 (skrl's vb would
 * be a NaN: a documented deviation); scratch_bytes below the plan's; a negative or non-finite epsilon or clip; and the operand rules.
 * Update: scratch is a written extent of scratch_bytes bytes; mean, var and count are state; those four are 8-byte aligned; skip_if is
 * optional and 4-byte aligned.  Apply: mean and var (8-byte aligned, required even for M = 0) are only read but stand clear of x, y
 * and each other like state; x and y count for M > 0 and may be the same array; M = 0 still wants a ctx. */
#define ROVER_SCALER_WIDE 0
#define ROVER_SCALER_NARROW 1
typedef struct {
    int32_t route;                                 /* ROVER_SCALER_WIDE / ROVER_SCALER_NARROW                                       */
    int32_t rows_per_chunk, n_chunks;
    int64_t scratch_bytes;
} rover_scaler_plan_desc;
ROVER_API int rover_scaler_plan(int32_t M, int32_t N, rover_scaler_plan_desc *plan);
typedef struct {
    const float *x;         int64_t x_stride;      /* [M, N]                                                                        */
    int32_t M, N;
    double *mean, *var, *count;                    /* device [N], [N], [1]: read and written by launch 2                            */
    void *scratch;          int64_t scratch_bytes; /* device, >= the plan's scratch_bytes                                           */
    const int32_t *skip_if;                        /* optional device [1]                                                           */
} rover_scaler_update_desc;
ROVER_API int rover_scaler_update(rover_ctx *ctx, const rover_scaler_update_desc *d, void *stream);
typedef struct {
    const float *x;         int64_t x_stride;      /* [M, N]                                                                        */
    float *y;               int64_t y_stride;      /* [M, N]; may be exactly x                                                      */
    int32_t M, N;
    const double *mean, *var;                      /* device [N] each                                                               */
    double epsilon, clip;                          /* >= 0, finite; rounded to f32 once                                             */
    int32_t inverse;                               /* 0: forward, else inverse                                                      */
} rover_scaler_apply_desc;
ROVER_API int rover_scaler_apply(rover_ctx *ctx, const rover_scaler_apply_desc *d, void *stream);

/* ---- terrain-following motion model: what moves the rovers between two steps (vec_env.TerrainSim) ------------------------------------ */
/* PhysX is out of scope; this is the project's own definition of a deterministic, stateless, kinematic pose feeder that keeps the six
 * wheels on the heightfield of rover_set_heightfield.  f32 on the device, one rounding per written operation, one thread per env.
 * Wheel layout (kinematics.py:20-25, order FL, FR, ML, MR, RL, RR), as (right r_i, forward f_i):
 *   (-0.385, 0.438) (0.385, 0.438) (-0.447, 0) (0.447, 0) (-0.385, -0.411) (0.385, -0.411);   body coordinates a_i = f_i, b_i = -r_i (left).
 * Body forward is world +x at yaw 0.  Each of `substeps` sub-steps of length dt, on the pose (x, y, z; quaternion w, qx, qy, qz):
 *   1. v = lin[e * cmd_stride] * max_lin,  w = ang[e * cmd_stride] * max_ang;  v_eff = |v / w| > 0.45f ? v : 0    (turn on the spot,
 *      kinematics.py:34-39: w = 0 with v != 0 keeps v, v = w = 0 gives 0)
 *   2. yaw0 = atan2(2 (w qz + qx qy), 1 - 2 (qy^2 + qz^2))   (the yaw of tensor_quat_to_eul: valid for a tilted body and for the reset
 *      kernel's quaternion);   yaw1 = yaw0 + w dt,  c = cos(yaw1),  s = sin(yaw1)
 *   3. x1 = x + (v_eff c) dt,   y1 = y + (v_eff s) dt
 *   4. wheel contact i at ((x1 + f_i c) + r_i s, (y1 + f_i s) - r_i c);  z_i = the heightfield there, exactly as rover_sample_height
 *      reads it (clamp, round half to even, lookup, times vertical_scale; option cell_index_mode applies)
 *   5. the least-squares plane z = z_c + p a + q b through the six samples: (z_c, p, q) = C z with the constant C [3][6] =
 *      pinv([1, a_i, b_i]) (rover_motion_plane_fit), each row summed from i = 0 upwards
 *   6. pitch = -atan(p),  roll = atan(q cos(pitch)) — the one roll for which the body's y axis lies in the plane —, yaw = yaw1, turned
 *      into a quaternion by the ZYX formula on the half angles:  w = (cr cp) cy + (sr sp) sy,  qx = (sr cp) cy - (cr sp) sy,
 *      qy = (cr sp) cy + (sr cp) sy,  qz = (cr cp) sy - (sr sp) cy;   tensor_quat_to_eul of it is (roll, pitch, yaw1) up to rounding
 *      and the wrap of yaw
 *   7. z1 = z_c + ride_height
 * pos3 and quat4 are updated IN PLACE (the step kernels borrow the same pointers); between sub-steps the pose stays in registers, and
 * `substeps` = n gives the bits of n calls with `substeps` = 1.  After the last sub-step, where the joint quadruple is given, all 13
 * columns are copied: joint_pos13 <- joint_pos_targets13, joint_vel13 <- joint_vel_targets13 (ideal actuators).
 * One launch of ceil(E / 256) workgroups (csrc/rover_motion.hip), plain vector loads and stores, no atomics, no LDS.  The call
 * allocates nothing, does not synchronise and can be captured in a graph.  E = 0: ROVER_OK, no launch.
 * ROVER_E_INVALID before any launch (the descriptor is checked before the ctx is looked at, as for rover_obs_noise): a NULL descriptor;
 * E < 0; substeps < 1; cmd_stride < 1; dt not finite or not > 0; a NULL pos3, quat4, lin or ang with E > 0; a joint quadruple given
 * only in part.  ROVER_E_STATE: no heightfield (rover_set_heightfield). */
typedef struct {
    float *pos3, *quat4;                           /* [E, 3], [E, 4] (w, x, y, z): read and written in place                       */
    const float *lin, *ang;                        /* env e's commands at [e * cmd_stride]                                         */
    int32_t cmd_stride, E, substeps;               /* cmd_stride 3: column 0 of the task's [E, 3] histories, newest first          */
    float dt, max_lin, max_ang, ride_height;
    const float *joint_pos_targets13, *joint_vel_targets13;      /* optional [E, 13]: all four or none                              */
    float *joint_pos13, *joint_vel13;
} rover_motion_desc;
ROVER_API int rover_motion_step(rover_ctx *ctx, const rover_motion_desc *d, void *stream);
/* Host only (no ctx, no device): the 18 floats of C, row-major (z_c's row, p's, q's), computed in double and rounded to f32 once. */
ROVER_API int rover_motion_plane_fit(float out[18]);

/* ---- rocker-bogie posture: the motion model's opt-in second mode (TerrainSim(suspension="bogie")) -------------------------------------- */
/* The plane of rover_motion_step leaves wheels above bumps or sunk into them; a rocker-bogie keeps all six down and takes up the
 * difference in its three passive joints — joint columns 0, 1, 2: FL_Boogie, FR_Boogie, R_Boogie.  This mode solves that posture and
 * writes the three angles into the joint state, where the step kernels read them: the uprightness penalty (rover.py:476, 492) and the
 * suspension transform of the 24 wheel rays (rock_detect.py:263-277).  Again this project's own definition: f32, one rounding per
 * written operation, one thread per env, stateless.  Each of `substeps` sub-steps of length dt:
 *   1.-3. commands, heading and position exactly as steps 1-3 of rover_motion_step
 *   4. wheel contacts at the layout of the wheel rays, not of kinematics.py: (a_i, b_i) = (forward, left) of the wheel frame's origin
 *      with all joints at 0 (T0 + T1 of rock_detect.py:201-215), in the order FL, FR, CL, CR, RL, RR:
 *        (0.439, 0.385) (0.439, -0.385) (0.007, 0.447) (0.007, -0.447) (-0.440, 0.385) (-0.440, -0.385);   every origin's body z is -0.167.
 *      Contact i at ((x1 + a_i c) - b_i s, (y1 + a_i s) + b_i c): sampled at yaw only — the posture does not move the sample points —;
 *      z_i = the heightfield there as in step 4 of rover_motion_step; all six loads are issued before the first is used
 *   5. posture.  Unknowns u = (z_c, roll, pitch, j0, j1, j2).  Targets t_i = z_i + (ride_height - 0.167f): flat ground at height h gives
 *      z = h + ride_height, as the plane mode does.  F(u)_i is the world z of wheel i's frame origin through the reference's own chain
 *      with zero steering.  With T0_i = (x0, y0, -0.197) = ((0.286, +-0.385), (-0.146, +-0.447), (-0.440, +-0.385)), T1 = (0.153, 0, 0.03)
 *      for i < 4 and (0, 0, 0.03) for the rear pair, susY = (-j0, j1, -j0, j1) for i < 4 and susX = -j2 for the rear pair:
 *        i < 4:   bx = (0.153 + x0 cos susY) - sin susY * -0.197,   by = y0,   bz = (0.03 + x0 sin susY) + cos susY * -0.197
 *        i >= 4:  bx = x0,   by = y0 cos susX + -0.197 sin susX,   bz = 0.03 + (-0.197 cos susX - y0 sin susX)
 *      (the chain's factors cos 0 = 1 and sin 0 = 0 of the angle a wheel does not have are left out), and through the third row of the
 *      ZYX body rotation:   F_i = (z_c - bx sin pitch) + cos pitch * (bz cos roll + by sin roll).
 *      Chord iteration from u = 0, `iters` times:   r_i = t_i - F(u)_i,   u_n <- u_n + sum_i D[n][i] r_i, each row summed from i = 0
 *      upwards.  D [6][6] = inv(J), J = dF/du at u = 0 — rows (1, b_i, -a_i, then -x0 in column 3 for FL and CL, +x0 in column 4 for FR
 *      and CR, y0 in column 5 for RL and RR), condition number 10.6 — in double on the host, each entry rounded to f32 once
 *      (rover_motion_bogie_fit).  The error contracts by the size of the angles per iteration: 4 iterations leave less than 1e-6 m at
 *      0.3 rad.  After the last iteration the joint angles are clamped to [-max_bogie, max_bogie]; the body pose is NOT re-solved, so a
 *      clamped env's pose is the unclamped solve's.  max_bogie's default of 0.6 rad is this project's choice: the repository holds no
 *      joint limits for the asset.
 *   6. (roll, pitch, yaw1) to the quaternion by the ZYX half-angle formula of step 6 of rover_motion_step; no atan, the angles are the
 *      unknowns themselves
 *   7. z1 = z_c;  pos3 and quat4 are written in place
 * `substeps` = n gives the bits of n calls with `substeps` = 1 (every sub-step's solve starts from u = 0).  On a planar heightfield
 * z = h + p a + q b the three joints are 0 to rounding and the body lies in the plane in this sense: -sin pitch = p and
 * cos pitch sin roll = q, the body's x and y axes rise by p and q per metre.  Because the contacts are sampled at yaw only, that is
 * the plane over the body's own horizontal coordinates; against the world plane's normal (tan pitch = -p) the body's z axis is off by
 * a term of third order in the slope, 0.014 rad at p = 0.3.  The iteration converges while the wheel-height differences stay near
 * 0.1 m (angles up to about 0.3 rad); on a step of several decimetres under one wheel it does not, the angles it returns are finite
 * but meaningless, and the joints sit at the clamp.
 * Joint state, after the last sub-step, where the joint quadruple is given: joint_vel13 <- joint_vel_targets13, all 13 columns (the
 * passive joints' velocity is not modelled); joint_pos13 <- joint_pos_targets13 in columns 3-12 and the last solve's clamped (j0, j1, j2)
 * in columns 0-2, whatever the targets hold there.  The workgroup copies all 13 columns of its rows cooperatively, as in
 * rover_motion_step; a workgroup BARRIER follows, and then each env's own thread overwrites columns 0-2 — the copy does not skip them.
 * One launch of ceil(E / 256) workgroups (csrc/rover_motion.hip), no LDS, no atomics.  Enqueues only, allocates nothing, capturable.
 * E = 0: ROVER_OK, no launch.  ROVER_E_INVALID before any launch, all decided before the ctx is looked at: every refusal of
 * rover_motion_step; a NULL params; iters outside 1 .. ROVER_BOGIE_MAX_ITERS; max_bogie not finite or not > 0.  ROVER_E_STATE: no
 * heightfield.  rover_motion_step, rover_motion_desc and rover_motion_plane_fit are unchanged by this mode. */
#define ROVER_BOGIE_MAX_ITERS 8
typedef struct {
    int32_t iters;                                 /* 1 .. 8; 4 is the binding's default                                           */
    float max_bogie;                               /* rad, finite and > 0; 0.6 is the binding's default                            */
} rover_bogie_params;
ROVER_API int rover_motion_step_bogie(rover_ctx *ctx, const rover_motion_desc *d, const rover_bogie_params *p, void *stream);
/* Host only (no ctx, no device): the 36 floats of D, row-major (z_c's row, roll's, pitch's, j0's, j1's, j2's). */
ROVER_API int rover_motion_bogie_fit(float out[36]);

/* ---- wheel-level drive: the motion model's opt-in third mode (TerrainSim(drive="wheels")); composes with both postures ---------------- */
/* The two modes above move the body by the policy's command itself and copy the joint targets into the joint state.  This mode closes
 * the chain the reference closes in PhysX — action -> Ackermann (rover_pre_physics_step) -> joint drives -> wheels on the ground -> body
 * motion — kinematically: the actuated joints follow their targets at a limited rate, and the body moves by the rigid motion that fits
 * the six wheels' velocity vectors best.  lin, ang, cmd_stride, max_lin and max_ang of the descriptor are NOT read (NULL / 0 are fine):
 * the joint targets are the command.  Again this project's own definition: f32, one rounding per written operation, one thread per env.
 * Wheel layout and order as in rover_motion_step (FL FR ML MR RL RR; a_i = f_i forward, b_i = -r_i left).  Joint columns, as
 * pre_physics_step writes them:   steering angle d_i: FL 4, FR 6, RL 7, RR 8 (ML, MR do not steer: d = 0);   wheel speed o_i: FL 9, FR 10,
 * ML 3, MR 5, RL 11, RR 12.  Steering angles are taken in Ackermann's own convention, counter-clockwise from body forward, exactly as
 * written into the targets — no sign flips.  (rock_detect.py:248 reads RL as -j7 when it places the wheel rays; that is the rays'
 * business and stays as it is.)
 * Each of `substeps` sub-steps of length dt:
 *   1. actuators.  step_s = steer_rate dt and step_w = wheel_accel dt, each computed once.  Every steered column, with D = target - d:
 *      d <- |D| > step_s ? d + copysign(step_s, D) : target;   every drive column the same with step_w on the joint velocity.  A state
 *      lands on its target exactly and never passes it (|D| > step and rounding is monotone); +inf rates are ideal actuators; a NaN
 *      target fails the comparison and is taken as it is, so it reaches that env's pose and no other's.  The state is the caller's
 *      joint_pos13 / joint_vel13: there is no hidden state, the call is stateless.
 *   2. wheel velocity vectors:  s_i = wheel_radius o_i;   t_2i = s_i cos d_i,  t_2i+1 = s_i sin d_i for the four steered wheels,
 *      t_2i = s_i,  t_2i+1 = 0 for ML and MR.
 *   3. body twist.  A rigid motion (vx, vy, w) gives wheel i the velocity u_i = (vx - w b_i, vy + w a_i); minimising sum |u_i - t_i|^2 is
 *      linear:  (vx, vy, w) = P t,  P [3][12] = pinv(M),  M's rows (1, 0, -b_i), (0, 1, a_i)  (condition number 1.87), computed in double
 *      on the host, each entry rounded to f32 once (rover_motion_drive_fit); each row is summed from column 0 upwards, all 12 columns.
 *   4. slip (optional output slip [E]), of the LAST sub-step:  q_i = (u_ix - t_2i)^2 + (u_iy - t_2i+1)^2 with u_ix = vx + w r_i and
 *      u_iy = vy + w f_i,  slip = sqrt((q_0 + q_1 + ... + q_5) / 6) in m/s: 0 when the wheels agree with one rigid motion, positive while
 *      the steering lags.  Slip is reported only; it does not change the motion.
 *   5. yaw0 as step 2 of rover_motion_step;   yaw1 = yaw0 + w dt,  c = cos(yaw1),  s = sin(yaw1);
 *      x1 = x + ((vx c) - (vy s)) dt,   y1 = y + ((vx s) + (vy c)) dt.   No turn-on-the-spot rule here: Ackermann applied it to the targets.
 *   6. posture: steps 4-7 of rover_motion_step (bogie params NULL) or steps 4-7 of rover_motion_step_bogie, by the same device functions:
 *      the same (x1, y1, yaw1) gives the bits those modes give.
 * After the last sub-step the steered columns of joint_pos13 and the drive columns of joint_vel13 hold the new states; every other column
 * follows the posture mode's rule (the targets' copy; with the bogie, columns 0-2 of joint_pos13 are the last solve's clamped angles).
 * `substeps` = n gives the bits of n calls with `substeps` = 1.  A reset needs nothing new: rover_reset_envs zeroes a reset env's joint
 * state, so a respawned rover starts at rest and ramps up.
 * wheel_radius is the length that turns rad/s into m/s.  kinematics.py:18,61 divides the ground speed by wheel_diameter = 0.2, so 0.2 (the
 * binding's default) moves the rover as far as the command modes do; the asset's physical radius is 0.1, which halves every speed, as
 * the reference's rover in PhysX does.  The repository holds no actuator limits for the asset: the binding's rates default to +inf.
 * One launch of ceil(E / 256) workgroups (csrc/rover_motion.hip); a workgroup stages its rows of the four joint arrays in LDS (53 248
 * bytes), no atomics.  Enqueues only, allocates nothing, capturable.  E = 0: ROVER_OK, no launch.  ROVER_E_INVALID before any launch, all
 * decided before the ctx is looked at: a NULL descriptor; E < 0; substeps < 1; dt not finite or not > 0; a NULL pos3 or quat4 with
 * E > 0; a joint quadruple given only in part, or not at all with E > 0; NULL drive params; wheel_radius not finite or not > 0; steer_rate
 * or wheel_accel NaN or not > 0 (+inf is valid); bogie params given with iters outside 1 .. ROVER_BOGIE_MAX_ITERS or max_bogie not finite
 * or not > 0.  ROVER_E_STATE: no heightfield.  The two modes above and their structs are unchanged by this one. */
typedef struct {
    float wheel_radius, steer_rate, wheel_accel;   /* m (finite, > 0), rad/s and rad/s^2 (> 0, +inf: ideal)                         */
    float *slip;                                   /* optional [E]: the last sub-step's slip, m/s                                  */
} rover_drive_params;
ROVER_API int rover_motion_step_drive(rover_ctx *ctx, const rover_motion_desc *d, const rover_drive_params *p,
                                      const rover_bogie_params *bogie /* NULL: the plane's posture */, void *stream);
/* Host only (no ctx, no device): the 36 floats of P, row-major (vx's row, vy's, w's); column 2i is wheel i's x component, 2i+1 its y. */
ROVER_API int rover_motion_drive_fit(float out[36]);

/* ---- episode statistics on the device (learning/tracking.py:EpisodeTracker) ----------------------------------------------------------- */
/* What skrl's agent writes every write_interval steps (instantaneous reward, total reward and length of the episodes in a deque of the
 * last W, each as max / min / mean), the exact totals of a reporting interval and the sums of up to 16 reward components, kept on the
 * device: one call per env step, at most two launches, no host read.  All state is the caller's device memory; the library keeps none.
 *
 * Inputs of one call: rewards [E] f32 (finite by contract); done [E] with elements of done_size = 1 byte (bool / uint8) or 8 bytes
 * (int64, the task's reset_buf), non-zero = the episode ended with this step; K component columns, each [E] of kind ROVER_TRACK_F32 or
 * ROVER_TRACK_I64, every element converted to f64 (one rounding for |i64| > 2^53) before it is summed.
 * State: per env cum_reward [E] f32 and cum_steps [E] i32; the window ring_ret [W] f32, ring_len [W] i32, ring_count (one i64: the
 * episodes ever appended); the interval record (rover_track_record below).  A fresh record is all zero except the minima, which hold
 * +inf / INT32_MAX, and the maxima, which hold -inf / INT32_MIN: a constant the caller writes.
 * One call, in this order:
 *   1. per env:  c = cum_reward[e] + rewards[e]  (one f32 add),  n = cum_steps[e] + 1;  done[e]: (c, n) is a finished episode and
 *      cum_reward[e] = 0, cum_steps[e] = 0;  otherwise cum_reward[e] = c, cum_steps[e] = n
 *   2. ring:  this call's finished episodes, in ascending env order, are appended: entry j goes to slot (ring_count + j) mod W (only
 *      the last min(n_finished, W) of them are written); then ring_count += n_finished
 *   3. record:  calls += 1;  inst_min / inst_max / inst_sum take every rewards[e];  ep_count += n_finished and the ep_* fields take every
 *      finished (c, n) (ep_ret_sumsq the f64 product c c, which is exact);  comp_sum[k] takes every element of column k;  and if
 *      ring_count > 0:  win_calls += 1, win_ret_mean_sum += (the f64 sum of the min(ring_count, W) valid slots) / their number,
 *      win_ret_min / win_ret_max take the ring's min / max, and the same three for the lengths (their sum is an exact integer)
 * Arithmetic: every f32 value (cum_reward, ring entries, each min / max) and every integer is exact — a restatement in float32 gives the
 * same bits (tests/track_ref.py); in a minimum or maximum -0 orders below +0.  The f64 sums are formed in a fixed order that depends on
 * E, W and K alone: the same inputs give the same bits on every run.  No floating-point atomics, no atomics at all.
 * Launches (csrc/rover_track.hip): an update kernel of ceil(E / 256) workgroups (step 1, the workgroup's finished pairs compacted in env
 * order into the scratch, one partial record per workgroup) and a one-workgroup merge kernel (steps 2 and 3); E = 0 launches the merge
 * kernel alone and is a counted call with no envs: calls += 1, the inst_*, ep_* and comp_sum fields stay, the win_* fields take the
 * ring as in every call.  The call allocates nothing, does not synchronise and can be captured in a graph.
 * ROVER_E_INVALID before any launch (the descriptor is checked before the ctx is looked at, as for rover_motion_step): a NULL
 * descriptor; E < 0; W outside 1 .. 1024; K outside 0 .. 16; done_size other than 1 or 8; a comp_kind below K other than the two kinds;
 * a NULL ring_ret, ring_len, ring_count or record; with E > 0 a NULL rewards, done, cum_reward, cum_steps or scratch, or a NULL comp
 * below K; scratch_bytes below what rover_track_sizes reports. */
#define ROVER_TRACK_MAX_COMPONENTS 16
#define ROVER_TRACK_MAX_WINDOW 1024
#define ROVER_TRACK_F32 0
#define ROVER_TRACK_I64 1
typedef struct {
    int64_t calls;
    double inst_sum;                               /* over every env of every call                                                 */
    int64_t ep_count;
    double ep_ret_sum, ep_ret_sumsq;
    int64_t ep_len_sum;
    int64_t win_calls;                             /* the calls at whose end the ring was not empty                                */
    double win_ret_mean_sum, win_len_mean_sum;     /* over those calls, the ring's mean return / length                            */
    double comp_sum[ROVER_TRACK_MAX_COMPONENTS];   /* over every env of every call                                                 */
    float inst_min, inst_max;
    float ep_ret_min, ep_ret_max;
    int32_t ep_len_min, ep_len_max;
    float win_ret_min, win_ret_max;                /* over those calls, the ring's min / max                                       */
    int32_t win_len_min, win_len_max;
} rover_track_record;                              /* 240 bytes */
typedef struct {
    const float *rewards;                          /* [E]                                                                          */
    const void *done;                              /* [E] elements of done_size bytes                                              */
    int32_t done_size, E, W, K;
    const void *comp[ROVER_TRACK_MAX_COMPONENTS];  /* K columns [E]                                                                */
    int32_t comp_kind[ROVER_TRACK_MAX_COMPONENTS];
    float *cum_reward;                             /* [E]                                                                          */
    int32_t *cum_steps;                            /* [E]                                                                          */
    float *ring_ret;                               /* [W]                                                                          */
    int32_t *ring_len;                             /* [W]                                                                          */
    int64_t *ring_count;
    rover_track_record *record;
    void *scratch;                                 /* scratch_bytes of rover_track_sizes, 8-byte aligned; only this call's         */
    int64_t scratch_bytes;
} rover_track_desc;
typedef struct {
    int32_t workgroup;                             /* envs per update workgroup (256)                                              */
    int32_t n_partials;                            /* ceil(E / workgroup)                                                          */
    int64_t partial_bytes;                         /* one workgroup's partial record                                               */
    int64_t finished_slots;                        /* n_partials * workgroup (return, length) pairs of 8 bytes                     */
    int64_t scratch_bytes;                         /* n_partials * partial_bytes + 8 * finished_slots                              */
} rover_track_sizes_out;
ROVER_API int rover_episode_track(rover_ctx *ctx, const rover_track_desc *d, void *stream);
/* Host only (no ctx, no device).  ROVER_E_INVALID: a NULL out, E < 0, W outside 1 .. 1024, K outside 0 .. 16. */
ROVER_API int rover_track_sizes(int32_t E, int32_t W, int32_t K, rover_track_sizes_out *out);

/* ---- tuning knobs ------------------------------------------------------------------------------------- */
/* name = "raycast_variant": 0 = auto; 1 = one half-wave per ray in env order, every cell block streamed from HBM;
 *        2 = rays counting-sorted by (map, cell), one wave per run of sorted rays, the cell's triangles held in registers
 *        (needs K <= 256 on both maps); 3 = culled: the sorted rays of 2, but a conservative bounding-sphere + normal test
 *        (16 B per triangle, built at rover_set_knn_map) first proves for most (ray, triangle) pairs that ray_casting.py:59
 *        rejects them, and only the remaining candidates get the exact arithmetic (csrc/rover_cull.hip) — in f32 or, with
 *        ray_precision = 2, in the reference's as-shipped fp16 arithmetic (its own, wider proof margins).
 *        4 = staged: the proof of 3 on per-cell record rows ordered by a distance bound (16 suffix levels per cell: a ray tests only the
 *        prefix it cannot clear as a group; 16 B per pair for the sphere test, 8 B per pair — f32 proof — for the normal test), one lane
 *        per (ray, chunk of 8 pairs), then the same exact phase.
 *        All give bit-identical results.  auto: fp32 arithmetic (ray_precision 0, 1) — 4 from 24 576 rays per step, 1 below;
 *        ray_precision = 2 — 2 up to 24 576 rays per step; above that 4: in env order below 98 304 rays per step, behind the sort beyond
 *        (on an irregular terrain mesh — fewer than half of its cells with a usable far bound — 4 from two heightmap rays per terrain cell, 3 below).
 * name = "lane_env_order" (variant 4): 1 = no sort, the ray slots in env order; 0 = rays sorted by (map, cell); -1 (default) = auto: env
 *        order while a step's heightmap rays are fewer than 1.5 per terrain cell and the rovers fewer than one per 64 cells (ray_precision
 *        2: below 98 304 rays per step).
 * name = "lane_rocks" (variant 4, sorted): 1 = the rock rays through the staged kernel too (one ray-cast launch), 0 = through the culled one
 *        (3); -1 (default) = auto: 1.
 * name = "lane_box" (variant 4, fp32 arithmetic): the form of the sphere test's records in the staged tables the NEXT rover_set_knn_map
 *        calls build.  0 = two bounding spheres per pair of triangles; 1 = one axis-aligned box per pair, tested on the three axes d x e_i;
 *        -1 (default) = auto: boxes for a map in which at least three quarters of the pairs fill their box (a regular grid mesh), spheres
 *        for any other (a decimated mesh).  One form per map; results do not depend on it (rover_info.lane_box reports it).
 * name = "lane_pair_rows" (variant 4, both arithmetics): the rows of the staged tables the NEXT rover_set_knn_map calls build.  0 = one row
 *        per cell; 1 = one row per two cells (ix, 2j), (ix, 2j + 1), holding the union of their triangles about the midpoint of their
 *        centres — where every union fits a row of 128 pairs, else the map keeps one row per cell; -1 (default) = auto: the terrain map
 *        only (nearly all of its cells hold rays, and two neighbours' rays share a wave: a row is read once for both; a rock ray streams its
 *        row alone).  Results do not depend on it (rover_info.lane_pair_rows reports it).
 * name = "lane_rebase" (variant 4, both arithmetics): how the staged kernel measures a steep ray against a row's suffix bounds.  0 = from
 *        the ray's origin; 1 (default) = from the point where the ray's line crosses the row's own height, so that the origin's height
 *        above the ground no longer widens the bound.  Read at every launch; no table and no plan depends on it, nor do the results.
 * name = "occlusion_route" (rover_obs_occlusion): 0 = the plain march (columns in obs order, every sample's node read); 1 (default) = the
 *        columns in rover_occlusion_order and the tile-max table in front of the node reads.  Read at every call; results do not depend on it.
 * name = "ray_precision": 0 (default) = the reference's fp32 mode, which the parity tests pin.
 *        1 = every ray origin / direction rounded to fp16 before the cell lookup and the ray maths, like the reference AS
 *        SHIPPED (Camera.dtype = float16: camera.py:55,212; rock_detect.py:319,371); f32 arithmetic after that.
 *        2 = AS SHIPPED: (1) plus every operation of ray_casting.py:31-59 rounded to fp16 the way ATen's Half kernels do,
 *        and fp16 collision thresholds (rover.py:667-668).  Bit-identical to the as-shipped reference on ray origins,
 *        distances, collision mask and done flags (ray-cast variants 2 and 3).
 * name = "bin_low_bits": width of the low digit of the ray bucket sort (2^bits map cells per bucket), 8..12, or 0 (default) = chosen by
 *        the library: 10, raised while that gives more than 4 096 buckets, lowered (to 8 at most) when that lets a sort entry fit one
 *        dword (num_envs x padded rays per env <= 2^(32 - bits)).  Results do not depend on it.
 * name = "raycast_early_out": 1 (default) = the binned kernel drops a whole packed pair of triangles per lane (the far half
 *        of a cell's K-nearest list; on the rocks map also the near half) when a conservative test on the numerators shows that
 *        every triangle of it fails the barycentric test; results are bit-identical with 0 (A/B and tests).
 * name = "cell_index_mode": how `(xy - shift) / 0.1` (camera.py:241, rock_detect.py:381, rover.py:590; a Python-float divisor)
 *        is evaluated.  0 = cpu_div (default): a correctly rounded division, what ATen's CPU kernel does and what the golden
 *        vectors (captured from the reference on CPU) pin.  1 = cuda_rcp: multiplication by 1.0f / 0.1f = 10.0f, what ATen's
 *        CUDA kernel does ("a * reciprocal(b)" for a CPU-scalar divisor) — the device the reference actually runs on.  The
 *        two differ only for coordinates within an ulp of a .5 tie of the cell grid (tests/test_oracle_golden.py).
 * name = "cull_queue_mb": most MiB the candidate queue of the culled ray cast may take (default 1536).  A wave of a launch owns a
 *        region of 1 024 entries (8 KB; a run that finds more finishes them and scans on), so a launch needs 8 KB per run of 64
 *        sorted rays: 712 MB at 65 536 envs x 63 rays.  Past the budget a step's ray cast is cut into several launches that
 *        re-use the regions (each extra launch costs ~25 us); an allocation failure is an error (ROVER_E_NOMEM), never a
 *        silent change of kernel.
 * name = "staged_tables": which proofs' tables of the staged ray cast (variant 4) the NEXT rover_set_knn_map calls build — bit 0 the f32
 *        proof (ray_precision 0 / 1), bit 1 the as-shipped fp16 proof (ray_precision 2); default 3.  About 4.3 KB per cell, map and proof
 *        at K = 200 (1.56 GB at 600 x 600 cells).  Tables that are not asked for, or that do not fit (the allocation failure is absorbed:
 *        the culled kernel, variant 3, then runs), leave variant 4 unavailable for that arithmetic: the auto choice never picks it, and
 *        asking for it by name ("raycast_variant" 4) is an error (ROVER_E_STATE / ROVER_E_NOMEM), never a silent change of kernel.
 * name = "raycast_run": rays per wave of the launches over the sorted list (variants 2, 3, 4) and — capped at 64 — slots per wave of
 *        variant 4 in env order; 1..4096, variants 3 and 4 cap it at 64.  0 (default) = auto, from r = rays per step / 65 536: variant 2
 *        r clamped to [4, 32]; variant 3 8 / 16 / 32 / 64 from r = 0 / 3 / 6 / 20 (regular terrain mesh, f32 arithmetic) or 0 / 12 /
 *        24 / 48 (irregular mesh, or ray_precision 2); variant 4 behind the sort 32, 64 from r = 12; in env order 16, 32 from 2^17
 *        padded ray slots, 64 from 2^20.  Results do not depend on it.
 * Every name above but "ray_precision" and "cell_index_mode" that has a ROVER_<NAME> environment variable (ROVER_RAYCAST_VARIANT,
 * ROVER_RAYCAST_RUN, ROVER_LANE_ENV_ORDER, ROVER_LANE_ROCKS, ROVER_LANE_BOX, ROVER_LANE_PAIR_ROWS, ROVER_LANE_REBASE, ROVER_BIN_LOW_BITS, ROVER_CULL_QUEUE_MB) takes its start value from it at
 * rover_create; a value outside the option's range (and 0 = auto) is ignored there. */
ROVER_API int rover_set_option(rover_ctx *ctx, const char *name, int64_t value);

/* ---- introspection (bench / roofline) ---------------------------------------------------------------- */
typedef struct {
    int32_t P, Ns, Nd, rays_per_env_padded;
    int32_t K[2], K8[2], X[2], Y[2];
    uint64_t table_bytes[2];       /* re-packed per-cell fp16 tables + cull tables */
    uint64_t workspace_bytes;
    int32_t raycast_variant;       /* the variant the next step will run: 1 env order, 2 binned, 3 culled, 4 staged (csrc/rover_cull.hip) */
    int32_t cell_index_mode;       /* option "cell_index_mode" in force: 0 cpu_div, 1 cuda_rcp (tests pin the mode a fixture was captured with) */
    int32_t ray_precision;         /* option "ray_precision" in force */
    int32_t raycast_sorted;        /* 1: the step sorts the rays by (map, cell) bin; 0: the ray cast walks the slots in env order */
    int32_t raycast_rocks_staged;  /* variant 4: 1 = the rocks part of the sorted list runs on the staged kernel too, 0 = on the culled one */
    int32_t lane_box[2];           /* per map: 1 = the staged tables of the fp32 arithmetic hold one box per pair of triangles, 0 = two spheres ("lane_box") */
    int32_t lane_pair_rows[2];     /* per map: 1 = the staged tables hold one row per two cells that neighbour in iy, 0 = one per cell ("lane_pair_rows") */
} rover_info;
ROVER_API int rover_get_info(const rover_ctx *ctx, rover_info *info);
/* The whole ray-cast plan in force (what the next step's ray cast will run) and the other host-side values that select a code path of
 * a step — host only: copies what the ctx already holds, launches nothing, does not synchronise.  Tests assert it field by field, so
 * that they know which kernel instantiation and traversal they exercised. */
typedef struct {
    int32_t variant;               /* 0: a map is missing; 1 env-order kernel, 2 binned, 3 culled, 4 staged */
    int32_t proof;                 /* the proof tables in force: 1 for the as-shipped fp16 arithmetic (ray_precision 2), else 0 */
    int32_t sorted;                /* the bucket sort by (map, cell) runs before the ray cast */
    int32_t env_order;             /* variant 4 over the ray slots in env order, one launch */
    int32_t rocks_staged;          /* variant 4: the rocks part on the staged kernel too (0: the culled kernel casts it, a second launch) */
    int32_t run;                   /* rays per wave of the sorted launches */
    int32_t env_run;               /* slots per wave of the staged kernel in env order (0 unless env_order) */
    int32_t lazy_far;              /* culled kernel: a bin's far records fetched only when a ray needs them */
    int32_t skip_clear;            /* culled kernel: rays that clear their whole cell left out of the scan */
    int32_t cull_launches;         /* launches the queue budget ("cull_queue_mb") cuts a culled ray cast over the whole ray set into
                                      (rover_cull_info.launches_per_step); 0: no candidate queue (variants 1, 2, or nothing to plan yet) */
    int32_t low_bits;              /* width of the low digit of the bucket sort in force ("bin_low_bits") */
    int32_t sort_entry_dwords;     /* 1: a sort entry is low bin bits | slot id in one dword, 2: (bin, slot); 0: the step does not sort */
    int32_t hist_fused;            /* 1: prep_rays_kernel counts the sort's coarse buckets itself (one launch less); 0 also when the step does not sort */
} rover_raycast_plan;
ROVER_API int rover_get_raycast_plan(const rover_ctx *ctx, rover_raycast_plan *out);
/* The same plan without a ctx and without a device, from the shapes and options alone (as rover_linear_route answers for a layer):
 * what rover_get_raycast_plan reports on a ctx with these inputs.  The options are the fields below, named as rover_set_option names
 * them and checked as it checks them — no environment variable is read; zero-initialise, then set lane_env_order = lane_rocks =
 * cull_lazy = -1 and cull_queue_mb = 1536 for the defaults.  Per map (terrain, rocks): X, Y and K8 as rover_get_info reports them,
 * cells_with_far_bound as rover_get_cull_info does, and which tables rover_set_knn_map built (the culled kernel's: K8 <= 256; the
 * staged kernel's per proof: option "staged_tables").  ROVER_E_INVALID (rover_last_error(NULL)) for a value no ctx could hold. */
typedef struct {
    int32_t num_envs, P, have_dist;    /* P: heightmap rays per env (0 with have_dist = 0: no rover_set_distribution yet) */
    int32_t ray_precision, raycast_variant, raycast_run, lane_env_order, lane_rocks, bin_low_bits;
    int32_t cull_lazy;                 /* ROVER_CULL_LAZY: < 0 auto, 0 / else force the culled kernel's on-demand far records */
    int64_t cull_queue_mb;
    int32_t map_present[2], X[2], Y[2], K8[2];
    int64_t cells_with_far_bound[2];
    int32_t has_cull_tables[2];
    int32_t has_staged_tables[2][2];   /* [map][proof]: 0 the f32 proof, 1 the as-shipped fp16 one */
} rover_plan_query;
ROVER_API int rover_plan_raycast(const rover_plan_query *query, rover_raycast_plan *out);
/* Diagnostics of the culled ray cast (variant 3, csrc/rover_cull.hip).  Per map: how many triangles its conservative
 * rejection test can never reject (slivers, non-finite vertices: stored with a zero normal = "always a candidate") and how
 * many cells have no normal cone (their rays run both tests on every pair).  Of the LAST culled launch on this ctx: rays
 * scanned, (ray, lane-pair) candidates handed to the exact arithmetic (camera.py:84-117 evaluated K per ray), rays that ran
 * both tests, (map, cell) bins walked.  Synchronises the device (a test / bench call, not a step call). */
typedef struct {
    int64_t triangles[2];
    int64_t always_candidate_triangles[2];
    int64_t cells_without_cone[2];
    uint64_t rays, candidate_pairs, rays_both_tests, bins;
    uint64_t max_pairs_per_run;    /* most queue entries any one run of sorted rays produced */
    uint64_t queue_bytes;          /* size of the candidate queue allocation */
    uint64_t launches_per_step;    /* 1, unless the queue budget ("cull_queue_mb") forces a step's ray cast into slices */
    uint64_t rays_far_skipped;     /* rays whose scan skipped the farther half of their cell's triangles (proved clear as a group) */
    int64_t cells_with_far_bound[2];  /* per map: cells whose far bound is wide enough to hold for a usual ray (f32 proof tables) */
    uint64_t far_records_on_demand;   /* 1: the scan kernel in use fetches a bin's far records only when one of its rays tests them, and does not scan rays that clear their whole cell (rays_not_scanned) */
    uint64_t rays_not_scanned;        /* rays that cleared BOTH halves of their cell's triangles as groups (no candidate: the distance is the miss value) */
    uint64_t lane_items, lane_flushes;   /* staged ray cast (variant 4): (ray, chunk of 8 pairs) items tested, exact-phase rounds of runs (saturating at 63 per wave) */
} rover_cull_info;
ROVER_API int rover_get_cull_info(rover_ctx *ctx, rover_cull_info *out);
/* In-situ kernel timing: when enabled, rover_step / rover_get_observations bracket the ray-cast launch with
 * hipEvents on the caller's stream (ring of 256 pairs).  rover_get_profile synchronises those events and
 * returns the summed ray-cast time and the number of TIMED launches since the last rover_set_profiling(ctx, n > 0).
 * enable = n > 1 times every n-th launch only (the first one included): an event pair costs the stream ~12 us around
 * the kernel it brackets (two 6 us bubbles on MI355X), which a caller timing its own steps may not want in each of them. */
typedef struct { double raycast_ms; int32_t launches; uint64_t pairs_per_launch; } rover_profile;
ROVER_API int rover_set_profiling(rover_ctx *ctx, int32_t enable);
ROVER_API int rover_get_profile(rover_ctx *ctx, rover_profile *out);
/* Launch ONLY the ray-cast kernel on the ray records left by the last step (for hipEvent timing of the
 * roofline kernel in isolation; results are rewritten identically). */
ROVER_API int rover_replay_raycast(rover_ctx *ctx, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_STEP_H */
