// rover_capi_sim.cpp — the sensor, simulation and statistics calls of the C-ABI layer (include/rover_step.h): observation noise, occlusion,
// the running scalers, the motion model, episode tracking.  Of the env state they only read the heightfield and the ray distribution:
// the only ctx member this unit writes is c->occ (rover_set_occlusion).
#include "../../include/rover_step.h"
#include "rover_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

extern "C" {

// Validates the whole descriptor before the ctx is looked at (a NULL ctx reports through rover_last_error(NULL)): the refusals can be
// checked without a device.
int rover_obs_noise(rover_ctx* c, const rover_obs_noise_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "obs_noise: null descriptor");
    if (d->M < 0 || d->F < 0) return fail(c, ROVER_E_INVALID, "obs_noise: M = %d or F = %d is negative", d->M, d->F);
    if (d->first < 0 || d->first > d->F) return fail(c, ROVER_E_INVALID, "obs_noise: first = %d outside 0 .. F = %d", d->first, d->F);
    if (d->F - d->first > (1 << 21)) return fail(c, ROVER_E_INVALID, "obs_noise: %d heightmap columns, more than 2^21", d->F - d->first);
    if (!(d->sigma_point >= 0.0f) || !std::isfinite(d->sigma_point) || !(d->sigma_offset >= 0.0f) || !std::isfinite(d->sigma_offset))
        return fail(c, ROVER_E_INVALID, "obs_noise: sigma_point = %g or sigma_offset = %g is negative or not finite", (double)d->sigma_point, (double)d->sigma_offset);
    if (!(d->dropout >= 0.0 && d->dropout <= 1.0)) return fail(c, ROVER_E_INVALID, "obs_noise: dropout = %g outside [0, 1]", d->dropout);
    if (!std::isfinite(d->drop_value)) return fail(c, ROVER_E_INVALID, "obs_noise: drop_value is not finite");
    if (d->row_offset < 0 || d->row_offset + (int64_t)d->M > (int64_t)1 << 32)
        return fail(c, ROVER_E_INVALID, "obs_noise: row_offset = %lld is negative or row_offset + M passes 2^32", (long long)d->row_offset);
    const bool empty = d->M == 0 || d->F == 0;
    if (!empty) {
        Operands ops("obs_noise");
        ops.read("in", d->in, d->in_stride, d->M, d->F, 4).written("out", d->out, d->out_stride, d->M, d->F, 4)
            .read("row_scale", d->row_scale, d->M, 1, d->M, 4, OP_OPTIONAL).read("episode", d->episode, d->M, 1, d->M, 8, OP_OPTIONAL)
            .read("step_dev", d->step_dev, 1, 1, 1, 8, OP_OPTIONAL)
            .same_array("out", "in");
        if (int e = check_operands(c, ops, false)) return e;
    }
    if (!c) return fail(nullptr, ROVER_E_INVALID, "obs_noise: null ctx");
    if (empty) return ROVER_OK;
    USE_DEVICE(c);
    ObsNoiseArgs a{};
    a.in = d->in; a.in_stride = d->in_stride; a.out = d->out; a.out_stride = d->out_stride;
    a.M = d->M; a.F = d->F; a.first = d->first;
    a.sigma_point = d->sigma_point; a.sigma_offset = d->sigma_offset; a.drop_value = d->drop_value;
    (void)rover_obs_noise_threshold(d->dropout, &a.thr);
    a.row_scale = d->row_scale; a.episode = d->episode;
    a.seed = d->seed; a.step = d->step; a.step_dev = d->step_dev; a.row_offset = d->row_offset;
    HIP_TRY(c, launch_obs_noise(a, (hipStream_t)stream));
    return ROVER_OK;
}

// Host only: the dropout threshold rover_obs_noise compares a column's 24-bit word with
int rover_obs_noise_threshold(double dropout, uint32_t* thr) {
    if (!thr || !(dropout >= 0.0 && dropout <= 1.0)) return fail(nullptr, ROVER_E_INVALID, "obs_noise_threshold: null argument or dropout = %g outside [0, 1]", dropout);
    *thr = (uint32_t)llrint(dropout * 16777216.0);
    return ROVER_OK;
}

// Host only: the heightmap columns far first by the horizontal distance of their body point from the camera, ties in column order
int rover_occlusion_order(const double* points, int32_t P, const int64_t* sparse_idx, int32_t Ns, const int64_t* dense_idx, int32_t Nd,
                          const float camera[3], int32_t* order) {
    if (!points || !order || !camera || P <= 0 || Ns < 0 || Nd < 0 || (Ns > 0 && !sparse_idx) || (Nd > 0 && !dense_idx))
        return fail(nullptr, ROVER_E_INVALID, "occlusion_order: null argument or bad counts (P=%d Ns=%d Nd=%d)", P, Ns, Nd);
    if (!std::isfinite(camera[0]) || !std::isfinite(camera[1]) || !std::isfinite(camera[2]))
        return fail(nullptr, ROVER_E_INVALID, "occlusion_order: the camera is not finite");
    const int32_t C = Ns + Nd;
    std::vector<double> key((size_t)C);
    for (int32_t c = 0; c < C; ++c) {
        const int64_t j = c < Ns ? sparse_idx[c] : dense_idx[c - Ns];
        if (j < 0 || j >= P) return fail(nullptr, ROVER_E_INVALID, "occlusion_order: index %lld outside [0,%d)", (long long)j, P);
        const double ax = (double)(float)points[3 * j] - (double)camera[0], ay = (double)(float)points[3 * j + 1] - (double)camera[1];
        const double k = ax * ax + ay * ay;
        key[(size_t)c] = k == k ? k : -1.0;        // a NaN point goes last
    }
    for (int32_t c = 0; c < C; ++c) order[c] = c;
    std::stable_sort(order, order + C, [&](int32_t a, int32_t b) { return key[(size_t)a] > key[(size_t)b]; });
    return ROVER_OK;
}

// The cfg is validated before the ctx is looked at.  Builds the three derived tables whole, then moves them into the ctx in one assignment
// (a failure half way leaves the previous configuration in force).
int rover_set_occlusion(rover_ctx* c, const rover_occlusion_cfg* cfg) {
    if (!cfg) return fail(c, ROVER_E_INVALID, "set_occlusion: null cfg");
    if (!std::isfinite(cfg->camera[0]) || !std::isfinite(cfg->camera[1]) || !std::isfinite(cfg->camera[2]) || !std::isfinite(cfg->step) ||
        !std::isfinite(cfg->clearance) || !std::isfinite(cfg->miss))
        return fail(c, ROVER_E_INVALID, "set_occlusion: camera, step, clearance and miss must be finite");
    if (!(cfg->step > 0.0f)) return fail(c, ROVER_E_INVALID, "set_occlusion: step = %g is not > 0", (double)cfg->step);
    if (cfg->max_steps < 2 || cfg->max_steps > 4096) return fail(c, ROVER_E_INVALID, "set_occlusion: max_steps = %d outside 2 .. 4096", cfg->max_steps);
    if (!(cfg->miss > 0.0f)) return fail(c, ROVER_E_INVALID, "set_occlusion: miss = %g is not > 0", (double)cfg->miss);
    if (!c) return fail(nullptr, ROVER_E_INVALID, "set_occlusion: null ctx");
    if (!c->have_dist) return fail(c, ROVER_E_STATE, "set_occlusion: rover_set_distribution first");
    if (!c->have_hf) return fail(c, ROVER_E_STATE, "set_occlusion: rover_set_heightfield first");
    USE_DEVICE(c);
    const int32_t C = c->Ns + c->Nd;
    std::vector<double> pts((size_t)c->P * 3);
    std::vector<int32_t> idx((size_t)C);
    HIP_TRY(c, hipMemcpy(pts.data(), c->d_dist.get(), pts.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (C) HIP_TRY(c, hipMemcpy(idx.data(), c->d_obs_idx.get(), idx.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int64_t> idx64(idx.begin(), idx.end());
    std::vector<float> body((size_t)C * 3);
    for (int32_t k = 0; k < C; ++k)
        for (int i = 0; i < 3; ++i) body[(size_t)3 * k + i] = (float)pts[(size_t)3 * idx[(size_t)k] + i];
    std::vector<int32_t> order((size_t)C);
    if (int e = rover_occlusion_order(pts.data(), c->P, idx64.data(), c->Ns, idx64.data() + c->Ns, c->Nd, cfg->camera, order.data()))
        return fail(c, e, "set_occlusion: %s", rover_last_error(nullptr));
    OcclusionTables t;
    t.cfg = *cfg;
    t.TN0 = (c->hf.N0 + OCC_TILE - 1) / OCC_TILE; t.TN1 = (c->hf.N1 + OCC_TILE - 1) / OCC_TILE;
    HIP_TRY(c, t.body3.alloc(body.size() + 1));
    HIP_TRY(c, t.order.alloc(order.size() + 1));
    HIP_TRY(c, t.tilemax.alloc((size_t)t.TN0 * t.TN1));
    if (C) HIP_TRY(c, hipMemcpy(t.body3.get(), body.data(), body.size() * sizeof(float), hipMemcpyHostToDevice));
    if (C) HIP_TRY(c, hipMemcpy(t.order.get(), order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, launch_occlusion_tiles(c->hf, t.tilemax.get(), t.TN0, t.TN1, nullptr));
    HIP_TRY(c, hipStreamSynchronize(nullptr));
    t.dist_gen = c->dist_gen; t.hf_gen = c->hf_gen;
    t.set = true;
    c->occ = std::move(t);
    return ROVER_OK;
}

// The descriptor is validated before the ctx is looked at, as for rover_obs_noise
int rover_obs_occlusion(rover_ctx* c, const rover_obs_occlusion_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "obs_occlusion: null descriptor");
    if (d->M < 0 || d->F < 0) return fail(c, ROVER_E_INVALID, "obs_occlusion: M = %d or F = %d is negative", d->M, d->F);
    if (d->first < 0 || d->first > d->F) return fail(c, ROVER_E_INVALID, "obs_occlusion: first = %d outside 0 .. F = %d", d->first, d->F);
    if (!std::isfinite(d->drop_value)) return fail(c, ROVER_E_INVALID, "obs_occlusion: drop_value is not finite");
    const bool empty = d->M == 0 || d->F == 0;
    const int64_t C = (int64_t)d->F - d->first;
    if (!empty) {
        Operands ops("obs_occlusion");
        ops.read("pos3", d->pos3, 3, d->M, 3, 4).read("quat4", d->quat4, 4, d->M, 4, 4)
            .read("clean", d->clean, d->clean_stride, d->M, d->F, 4).read("in", d->in, d->in_stride, d->M, d->F, 4)
            .written("out", d->out, d->out_stride, d->M, d->F, 4)
            .written("hidden_u8", d->hidden_u8, d->hidden_stride, d->M, C, 1, OP_OPTIONAL).written("target3", d->target3, 3 * C, d->M, 3 * C, 4, OP_OPTIONAL)
            .same_array("out", "in");
        if (int e = check_operands(c, ops, false)) return e;
    }
    if (!c) return fail(nullptr, ROVER_E_INVALID, "obs_occlusion: null ctx");
    if (!c->have_dist) return fail(c, ROVER_E_STATE, "obs_occlusion: rover_set_distribution first");
    if (!c->have_hf) return fail(c, ROVER_E_STATE, "obs_occlusion: rover_set_heightfield first");
    if (!c->occ.set) return fail(c, ROVER_E_STATE, "obs_occlusion: rover_set_occlusion first");
    if (c->occ.dist_gen != c->dist_gen || c->occ.hf_gen != c->hf_gen)
        return fail(c, ROVER_E_STATE, "obs_occlusion: the %s was set again after rover_set_occlusion: call rover_set_occlusion again",
                    c->occ.dist_gen != c->dist_gen ? "distribution" : "heightfield");
    if (C != (int64_t)c->Ns + c->Nd)
        return fail(c, ROVER_E_STATE, "obs_occlusion: F - first = %lld columns, the distribution has Ns + Nd = %d", (long long)C, c->Ns + c->Nd);
    if (empty) return ROVER_OK;
    USE_DEVICE(c);
    const OcclusionTables& t = c->occ;
    OcclusionArgs a{};
    a.h = c->hf;
    a.tilemax = t.tilemax.get(); a.TN0 = t.TN0; a.TN1 = t.TN1;
    a.body3 = t.body3.get(); a.order = t.order.get();
    a.pos3 = d->pos3; a.quat4 = d->quat4;
    a.clean = d->clean; a.clean_stride = d->clean_stride; a.in = d->in; a.in_stride = d->in_stride; a.out = d->out; a.out_stride = d->out_stride;
    a.hidden = d->hidden_u8; a.hidden_stride = d->hidden_stride; a.target3 = d->target3;
    a.M = d->M; a.F = d->F; a.first = d->first;
    for (int i = 0; i < 3; ++i) a.camera[i] = t.cfg.camera[i];
    a.step = t.cfg.step; a.clearance = t.cfg.clearance; a.miss = t.cfg.miss; a.drop_value = d->drop_value;
    a.max_steps = t.cfg.max_steps; a.route = c->occlusion_route;
    HIP_TRY(c, launch_obs_occlusion(a, (hipStream_t)stream));
    return ROVER_OK;
}

// Host only, a pure function of (M, N): the route, the chunking and the scratch of rover_scaler_update
int rover_scaler_plan(int32_t M, int32_t N, rover_scaler_plan_desc* plan) {
    if (!plan) return fail(nullptr, ROVER_E_INVALID, "scaler_plan: null plan");
    if (N < 1 || N > 4096) return fail(nullptr, ROVER_E_INVALID, "scaler_plan: N = %d outside 1 .. 4096", N);
    if (M < 0 || (int64_t)M * N >= (int64_t)1 << 31) return fail(nullptr, ROVER_E_INVALID, "scaler_plan: M = %d is negative or M N >= 2^31", M);
    const bool narrow = (uint32_t)N <= SCALER_NARROW_MAX_N;
    plan->route = narrow ? ROVER_SCALER_NARROW : ROVER_SCALER_WIDE;
    plan->rows_per_chunk = narrow ? 16384 : (M <= 8192 ? 32 : 128);
    plan->n_chunks = (int32_t)(((int64_t)M + plan->rows_per_chunk - 1) / plan->rows_per_chunk);
    plan->scratch_bytes = 8 + (int64_t)24 * plan->n_chunks * N;
    return ROVER_OK;
}

// The descriptor is validated before the ctx is looked at, as for rover_obs_noise
int rover_scaler_update(rover_ctx* c, const rover_scaler_update_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "scaler_update: null descriptor");
    rover_scaler_plan_desc plan;
    if (d->N < 1 || d->N > 4096) return fail(c, ROVER_E_INVALID, "scaler_update: N = %d outside 1 .. 4096", d->N);
    if (d->M < 0 || (int64_t)d->M * d->N >= (int64_t)1 << 31) return fail(c, ROVER_E_INVALID, "scaler_update: M = %d is negative or M N >= 2^31", d->M);
    if (d->M < 2) return fail(c, ROVER_E_INVALID, "scaler_update: M = %d rows, a train call needs at least 2 (the unbiased variance of one row is undefined)", d->M);
    (void)rover_scaler_plan(d->M, d->N, &plan);
    if (d->scratch_bytes < plan.scratch_bytes)
        return fail(c, ROVER_E_INVALID, "scaler_update: scratch of %lld bytes, the plan needs %lld", (long long)d->scratch_bytes, (long long)plan.scratch_bytes);
    Operands ops("scaler_update");
    ops.read("x", d->x, d->x_stride, d->M, d->N, 4).written("scratch", d->scratch, 0, 1, d->scratch_bytes, 1, OP_BYTES, 8)
        .state("mean", d->mean, d->N, 1, d->N, 8, 0, 8).state("var", d->var, d->N, 1, d->N, 8, 0, 8).state("count", d->count, 1, 1, 1, 8, 0, 8)
        .read("skip_if", d->skip_if, 1, 1, 1, 4, OP_OPTIONAL, 4);
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    ScalerUpdateArgs a{};
    a.x = d->x; a.x_stride = d->x_stride;
    a.M = (uint32_t)d->M; a.N = (uint32_t)d->N; a.rows_per_chunk = (uint32_t)plan.rows_per_chunk; a.n_chunks = (uint32_t)plan.n_chunks;
    a.partials = (double*)d->scratch + 1;
    a.mean = d->mean; a.var = d->var; a.count = d->count; a.skip_if = d->skip_if;
    HIP_TRY(c, launch_scaler_update(a, plan.route == ROVER_SCALER_NARROW ? SCALER_ROUTE_NARROW : SCALER_ROUTE_WIDE, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_scaler_apply(rover_ctx* c, const rover_scaler_apply_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "scaler_apply: null descriptor");
    if (d->N < 1 || d->N > 4096) return fail(c, ROVER_E_INVALID, "scaler_apply: N = %d outside 1 .. 4096", d->N);
    if (d->M < 0 || (int64_t)d->M * d->N >= (int64_t)1 << 31) return fail(c, ROVER_E_INVALID, "scaler_apply: M = %d is negative or M N >= 2^31", d->M);
    if (!(d->epsilon >= 0.0) || !std::isfinite(d->epsilon) || !(d->clip >= 0.0) || !std::isfinite(d->clip))
        return fail(c, ROVER_E_INVALID, "scaler_apply: epsilon = %g or clip = %g is negative or not finite", d->epsilon, d->clip);
    Operands ops("scaler_apply");
    if (d->M > 0) ops.read("x", d->x, d->x_stride, d->M, d->N, 4).written("y", d->y, d->y_stride, d->M, d->N, 4).same_array("y", "x");
    ops.state("mean", d->mean, d->N, 1, d->N, 8, 0, 8).state("var", d->var, d->N, 1, d->N, 8, 0, 8);      // only read here, but clear of x and y too
    if (int e = check_operands(c, ops)) return e;
    if (d->M == 0) return ROVER_OK;
    USE_DEVICE(c);
    ScalerApplyArgs a{d->x, d->x_stride, d->y, d->y_stride, (uint32_t)d->M, (uint32_t)d->N, d->mean, d->var, (float)d->epsilon, (float)d->clip};
    HIP_TRY(c, launch_scaler_apply(a, d->inverse != 0, (hipStream_t)stream));
    return ROVER_OK;
}

// The checks that the three motion entry points share, in two parts: the descriptor's own, which need no ctx ...  `commands`: the mode
// reads lin, ang and cmd_stride (rover_motion_step_drive does not)
static int motion_check_desc(rover_ctx* c, const rover_motion_desc* d, const char* what, bool commands = true) {
    if (!d) return fail(c, ROVER_E_INVALID, "%s: null descriptor", what);
    if (commands) {
        if (d->E < 0 || d->substeps < 1 || d->cmd_stride < 1)
            return fail(c, ROVER_E_INVALID, "%s: E = %d is negative, substeps = %d or cmd_stride = %d is below 1", what, d->E, d->substeps, d->cmd_stride);
    } else if (d->E < 0 || d->substeps < 1) {
        return fail(c, ROVER_E_INVALID, "%s: E = %d is negative or substeps = %d is below 1", what, d->E, d->substeps);
    }
    if (!std::isfinite(d->dt) || !(d->dt > 0.0f)) return fail(c, ROVER_E_INVALID, "%s: dt = %g is not finite or not > 0", what, (double)d->dt);
    if (commands) {
        if (d->E > 0 && (!d->pos3 || !d->quat4 || !d->lin || !d->ang)) return fail(c, ROVER_E_INVALID, "%s: pos3, quat4, lin and ang must be given", what);
    } else if (d->E > 0 && (!d->pos3 || !d->quat4)) {
        return fail(c, ROVER_E_INVALID, "%s: pos3 and quat4 must be given", what);
    }
    const int n_joint = (d->joint_pos_targets13 != nullptr) + (d->joint_vel_targets13 != nullptr) + (d->joint_pos13 != nullptr) + (d->joint_vel13 != nullptr);
    if (n_joint != 0 && n_joint != 4)
        return fail(c, ROVER_E_INVALID, "%s: joint_pos_targets13, joint_vel_targets13, joint_pos13 and joint_vel13 go together (%d of 4 given)", what, n_joint);
    return ROVER_OK;
}

// ... and the ctx's, after which the kernel's arguments are filled in
static int motion_check_ctx(rover_ctx* c, const rover_motion_desc* d, const char* what, MotionArgs& a) {
    if (!c) return fail(nullptr, ROVER_E_INVALID, "%s: null ctx", what);
    if (!c->have_hf) return fail(c, ROVER_E_STATE, "%s: rover_set_heightfield first", what);
    a.h = c->hf;
    a.pos3 = d->pos3; a.quat4 = d->quat4; a.lin = d->lin; a.ang = d->ang;
    a.cmd_stride = d->cmd_stride; a.E = (uint32_t)d->E; a.substeps = d->substeps;
    a.dt = d->dt; a.max_lin = d->max_lin; a.max_ang = d->max_ang; a.ride_height = d->ride_height;
    a.joint_pos_targets13 = d->joint_pos_targets13; a.joint_vel_targets13 = d->joint_vel_targets13;
    a.joint_pos13 = d->joint_pos13; a.joint_vel13 = d->joint_vel13;
    return ROVER_OK;
}

// The descriptor is validated before the ctx is looked at, as for rover_obs_noise
int rover_motion_step(rover_ctx* c, const rover_motion_desc* d, void* stream) {
    const char* what = "motion_step";
    if (int e = motion_check_desc(c, d, what)) return e;
    MotionArgs a{};
    if (int e = motion_check_ctx(c, d, what, a)) return e;
    if (d->E == 0) return ROVER_OK;
    USE_DEVICE(c);
    motion_plane_fit(a.fit);
    HIP_TRY(c, launch_motion(a, (hipStream_t)stream));
    return ROVER_OK;
}

static int bogie_check_params(rover_ctx* c, const rover_bogie_params* p, const char* what) {
    if (p->iters < 1 || p->iters > ROVER_BOGIE_MAX_ITERS)
        return fail(c, ROVER_E_INVALID, "%s: iters = %d is outside 1 .. %d", what, p->iters, ROVER_BOGIE_MAX_ITERS);
    if (!std::isfinite(p->max_bogie) || !(p->max_bogie > 0.0f))
        return fail(c, ROVER_E_INVALID, "%s: max_bogie = %g is not finite or not > 0", what, (double)p->max_bogie);
    return ROVER_OK;
}

// The rocker-bogie posture mode: rover_motion_step's refusals and the two parameters', all before the ctx is looked at
int rover_motion_step_bogie(rover_ctx* c, const rover_motion_desc* d, const rover_bogie_params* p, void* stream) {
    const char* what = "motion_step_bogie";
    if (int e = motion_check_desc(c, d, what)) return e;
    if (!p) return fail(c, ROVER_E_INVALID, "%s: null parameters", what);
    if (int e = bogie_check_params(c, p, what)) return e;
    MotionArgs a{};
    if (int e = motion_check_ctx(c, d, what, a)) return e;
    if (d->E == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_motion_bogie(a, p->iters, p->max_bogie, (hipStream_t)stream));
    return ROVER_OK;
}

// The wheel-level drive mode: the refusals of the other two modes that still apply (the commands are not read), the drive parameters'
// and, where given, the bogie parameters', all before the ctx is looked at
int rover_motion_step_drive(rover_ctx* c, const rover_motion_desc* d, const rover_drive_params* p, const rover_bogie_params* b, void* stream) {
    const char* what = "motion_step_drive";
    if (int e = motion_check_desc(c, d, what, false)) return e;
    if (d->E > 0 && !d->joint_pos13)           // given in part is refused above
        return fail(c, ROVER_E_INVALID, "%s: joint_pos_targets13, joint_vel_targets13, joint_pos13 and joint_vel13 must be given", what);
    if (!p) return fail(c, ROVER_E_INVALID, "%s: null parameters", what);
    if (!std::isfinite(p->wheel_radius) || !(p->wheel_radius > 0.0f))
        return fail(c, ROVER_E_INVALID, "%s: wheel_radius = %g is not finite or not > 0", what, (double)p->wheel_radius);
    if (!(p->steer_rate > 0.0f) || !(p->wheel_accel > 0.0f))
        return fail(c, ROVER_E_INVALID, "%s: steer_rate = %g or wheel_accel = %g is NaN or not > 0", what, (double)p->steer_rate, (double)p->wheel_accel);
    if (b)
        if (int e = bogie_check_params(c, b, what)) return e;
    MotionArgs a{};
    if (int e = motion_check_ctx(c, d, what, a)) return e;
    if (d->E == 0) return ROVER_OK;
    USE_DEVICE(c);
    DriveArgs g{p->wheel_radius, p->steer_rate, p->wheel_accel, p->slip, b != nullptr, b ? b->iters : 0, b ? b->max_bogie : 0.0f};
    if (!b) motion_plane_fit(a.fit);
    HIP_TRY(c, launch_motion_drive(a, g, (hipStream_t)stream));
    return ROVER_OK;
}

// Host only: the constant of the drive mode's twist fit
int rover_motion_drive_fit(float out[36]) {
    if (!out) return fail(nullptr, ROVER_E_INVALID, "motion_drive_fit: null argument");
    float fit[3][2 * MOTION_WHEELS];
    motion_drive_fit(fit);
    memcpy(out, fit, sizeof fit);
    return ROVER_OK;
}

// Host only: the constant of the posture solve
int rover_motion_bogie_fit(float out[36]) {
    if (!out) return fail(nullptr, ROVER_E_INVALID, "motion_bogie_fit: null argument");
    float inv[MOTION_WHEELS][MOTION_WHEELS];
    motion_bogie_fit(inv);
    memcpy(out, inv, sizeof inv);
    return ROVER_OK;
}

// Host only: the constant of the motion model's plane fit
int rover_motion_plane_fit(float out[18]) {
    if (!out) return fail(nullptr, ROVER_E_INVALID, "motion_plane_fit: null argument");
    float fit[3][MOTION_WHEELS];
    motion_plane_fit(fit);
    memcpy(out, fit, sizeof fit);
    return ROVER_OK;
}

static bool track_shape_ok(int32_t E, int32_t W, int32_t K) {
    return E >= 0 && W >= 1 && W <= ROVER_TRACK_MAX_WINDOW && K >= 0 && K <= ROVER_TRACK_MAX_COMPONENTS;
}

// Host only: what the descriptor's scratch must cover
int rover_track_sizes(int32_t E, int32_t W, int32_t K, rover_track_sizes_out* out) {
    if (!out) return fail(nullptr, ROVER_E_INVALID, "track_sizes: null argument");
    if (!track_shape_ok(E, W, K))
        return fail(nullptr, ROVER_E_INVALID, "track_sizes: E = %d is negative, W = %d is outside 1 .. %d or K = %d is outside 0 .. %d", E, W,
                    ROVER_TRACK_MAX_WINDOW, K, ROVER_TRACK_MAX_COMPONENTS);
    out->workgroup = TRACK_BLOCK;
    out->n_partials = (int32_t)track_partials((uint32_t)E);
    out->partial_bytes = (int64_t)track_partial_bytes();
    out->finished_slots = (int64_t)out->n_partials * TRACK_BLOCK;
    out->scratch_bytes = (int64_t)track_scratch_bytes((uint32_t)E);
    return ROVER_OK;
}

// The descriptor is validated before the ctx is looked at, as for rover_motion_step
int rover_episode_track(rover_ctx* c, const rover_track_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "episode_track: null descriptor");
    if (!track_shape_ok(d->E, d->W, d->K))
        return fail(c, ROVER_E_INVALID, "episode_track: E = %d is negative, W = %d is outside 1 .. %d or K = %d is outside 0 .. %d", d->E, d->W,
                    ROVER_TRACK_MAX_WINDOW, d->K, ROVER_TRACK_MAX_COMPONENTS);
    if (d->done_size != 1 && d->done_size != 8) return fail(c, ROVER_E_INVALID, "episode_track: done_size = %d is neither 1 nor 8", d->done_size);
    for (int32_t k = 0; k < d->K; ++k)
        if (d->comp_kind[k] != ROVER_TRACK_F32 && d->comp_kind[k] != ROVER_TRACK_I64)
            return fail(c, ROVER_E_INVALID, "episode_track: comp_kind[%d] = %d is neither ROVER_TRACK_F32 nor ROVER_TRACK_I64", k, d->comp_kind[k]);
    if (!d->ring_ret || !d->ring_len || !d->ring_count || !d->record)
        return fail(c, ROVER_E_INVALID, "episode_track: ring_ret, ring_len, ring_count and record must be given");
    if (d->E > 0) {
        if (!d->rewards || !d->done || !d->cum_reward || !d->cum_steps || !d->scratch)
            return fail(c, ROVER_E_INVALID, "episode_track: rewards, done, cum_reward, cum_steps and scratch must be given");
        for (int32_t k = 0; k < d->K; ++k)
            if (!d->comp[k]) return fail(c, ROVER_E_INVALID, "episode_track: comp[%d] is NULL (K = %d)", k, d->K);
        if (((uintptr_t)d->scratch & 7u) != 0) return fail(c, ROVER_E_INVALID, "episode_track: scratch is not 8-byte aligned");
        if (d->scratch_bytes < (int64_t)track_scratch_bytes((uint32_t)d->E))
            return fail(c, ROVER_E_INVALID, "episode_track: scratch_bytes = %lld is below the %llu of rover_track_sizes", (long long)d->scratch_bytes,
                        (unsigned long long)track_scratch_bytes((uint32_t)d->E));
    }
    if (!c) return fail(nullptr, ROVER_E_INVALID, "episode_track: null ctx");
    USE_DEVICE(c);
    TrackArgs a{};
    a.rewards = d->rewards; a.done = d->done; a.done8 = d->done_size == 8;
    a.E = (uint32_t)d->E; a.W = (uint32_t)d->W; a.K = (uint32_t)d->K;
    for (int32_t k = 0; k < d->K; ++k) {
        a.comp[k] = d->comp[k];
        if (d->comp_kind[k] == ROVER_TRACK_I64) a.comp_i64 |= 1u << k;
    }
    a.cum_reward = d->cum_reward; a.cum_steps = d->cum_steps;
    a.ring_ret = d->ring_ret; a.ring_len = d->ring_len; a.ring_count = d->ring_count;
    a.record = d->record; a.scratch = d->scratch;
    HIP_TRY(c, launch_track(a, (hipStream_t)stream));
    return ROVER_OK;
}

}  // extern "C"
