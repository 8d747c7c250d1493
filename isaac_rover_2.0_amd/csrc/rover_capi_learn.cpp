// rover_capi_learn.cpp — the learning kernels' entry points of the C-ABI layer (include/rover_step.h): linear, chain, Gaussian head, GAE,
// the backward, the PPO loss, the optimiser, the GRU, the gated sum, and their host-only route queries.
// A learning call never touches env state: of the ctx this unit uses only the device number (through USE_DEVICE), the error string
// (through fail) and the `learn` member (mlp_scratch_reserve, which takes the ctx, counts as part of it) — a search of this file for
// the ctx arrow finds nothing but that member.
#include "../../include/rover_step.h"
#include "rover_ctx.h"
#include "rover_bf16.h"
#include "rover_philox.h"

#include <cmath>
#include <cstdio>

extern "C" {

// the f32 and the bf16 layer differ in the launch alone (launch_linear_act: rover_mlp.hip; launch_linear_bf16: rover_bf16_tile.hip)
static int linear_forward_run(rover_ctx* c, const char* what, hipError_t (*launch)(const LinearArgs&, hipStream_t), const float* x, int64_t x_stride,
                              int32_t M, int32_t K, const float* weight, const float* bias, int32_t N, int32_t activation, float* y, int64_t y_stride,
                              void* stream) {
    if (!c) return ROVER_E_INVALID;
    // K = 0: a layer over an empty obs slice (model.py builds Encoder(0, ...) when a heightmap part is absent) = act(bias)
    if ((K > 0 && (!x || !weight)) || !y || M < 0 || K < 0 || N <= 0 || N > 256 || x_stride < K || y_stride < N || activation < 0 || activation > 4)
        return fail(c, ROVER_E_INVALID, "%s: bad arguments (M=%d K=%d N=%d act=%d)", what, M, K, N, activation);
    if (M == 0) return ROVER_OK;
    USE_DEVICE(c);
    LinearArgs a{x, x_stride, weight, bias, y, y_stride, M, K, N, activation};
    HIP_TRY(c, launch(a, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_linear_forward(rover_ctx* c, const float* x, int64_t x_stride, int32_t M, int32_t K, const float* weight, const float* bias,
                         int32_t N, int32_t activation, float* y, int64_t y_stride, void* stream) {
    return linear_forward_run(c, "linear_forward", launch_linear_act, x, x_stride, M, K, weight, bias, N, activation, y, y_stride, stream);
}

int rover_linear_forward_bf16(rover_ctx* c, const float* x, int64_t x_stride, int32_t M, int32_t K, const float* weight, const float* bias,
                              int32_t N, int32_t activation, float* y, int64_t y_stride, void* stream) {
    return linear_forward_run(c, "linear_forward_bf16", launch_linear_bf16, x, x_stride, M, K, weight, bias, N, activation, y, y_stride, stream);
}

// One chain, validated in one place.  The shape half: M, K0, the depth, every width and activation — all chain_route() reads, so all a route query looks at (no pointer of
// the descriptor but widths / activations).  0 = fine, -1 = M / K0 / the depth / a null array, i + 1 = layer i's width or activation.
// min_k0: 1 for the f32 chains; 0 for the bf16 ones, which also run a chain over an EMPTY obs slice (model.py builds Encoder(0, ...) when
// a heightmap part is absent: its first layer is act(bias), as rover_linear_forward computes it for K = 0) — x is then not read.
static int chain_shape_of(const rover_chain_desc& d, int32_t M, ChainArgs* a, int32_t min_k0 = 1) {
    if (!d.widths || !d.activations || M < 0 || d.K0 < min_k0 || (d.n_layers != 2 && d.n_layers != 4)) return -1;
    *a = ChainArgs{};
    a->M = M; a->K0 = d.K0; a->n_layers = d.n_layers;
    for (int i = 0; i < d.n_layers; ++i) {
        if (d.widths[i] <= 0 || d.widths[i] > 256 || d.activations[i] < 0 || d.activations[i] > 4) return i + 1;
        a->n[i] = d.widths[i]; a->act[i] = d.activations[i];
    }
    return 0;
}
// The whole of it, for a call that launches: the shapes, then the pointers and the row strides (0 = ok, else the error is recorded
// under `what`, the entry point that was called)
static int chain_args_of(rover_ctx* c, const rover_chain_desc& d, int32_t M, const char* what, ChainArgs* out, int32_t min_k0 = 1) {
    ChainArgs a;
    const int bad = chain_shape_of(d, M, &a, min_k0);
    if (bad < 0 || (!d.x && d.K0 > 0) || !d.y || !d.weights || !d.biases || d.x_stride < d.K0)
        return fail(c, ROVER_E_INVALID, "%s: bad arguments (M=%d K0=%d layers=%d)", what, M, d.K0, d.n_layers);
    for (int i = 0; i < d.n_layers; ++i) {
        if ((!d.weights[i] && (i > 0 || d.K0 > 0)) || bad == i + 1)
            return fail(c, ROVER_E_INVALID, "%s: layer %d: width %d activation %d", what, i, d.widths[i], d.activations[i]);
        a.w[i] = d.weights[i]; a.b[i] = d.biases[i];
    }
    if (d.y_stride < a.n[d.n_layers - 1]) return fail(c, ROVER_E_INVALID, "%s: y_stride %lld < width %d", what, (long long)d.y_stride, a.n[d.n_layers - 1]);
    a.x = d.x; a.x_stride = d.x_stride; a.y = d.y; a.y_stride = d.y_stride;
    *out = a;
    return ROVER_OK;
}

// the split-k scratch buffer, grown when a larger batch comes (not inside a stream capture — size the first call before capturing)
static int mlp_scratch_reserve(rover_ctx* c, size_t need, hipStream_t s) {
    if (need * sizeof(float) <= c->learn.mlp_scratch.bytes()) return ROVER_OK;
    HIP_TRY(c, hipStreamSynchronize(s));          // kernels still reading the old buffer
    HIP_TRY(c, c->learn.mlp_scratch.alloc(need));
    return ROVER_OK;
}

static int chain_refused(rover_ctx* c, const char* what) {
    return fail(c, ROVER_E_INVALID, "%s: net outside the built tile shapes (<= 96 -> <= 64, or <= 256 -> <= 160 -> <= 128 -> <= 16 with hidden activations none / LeakyReLU / ReLU)", what);
}

// launches what chain_route() chose (never ChainKernel::None)
static int chain_run(rover_ctx* c, const ChainArgs& a, const ChainRoute& r, hipStream_t s) {
    if (r.kernel == ChainKernel::SplitK)
        if (int e = mlp_scratch_reserve(c, chain_splitk_scratch_floats(a.M, a.K0, a.n[0]), s)) return e;
    HIP_TRY(c, launch_chain(a, r, c->learn.mlp_scratch.get(), s));
    return ROVER_OK;
}

// the f32 and the bf16 entry points differ in the route function alone (chain_route / chain_route_bf16: rover_mlp.hip)
typedef ChainRoute (*ChainRouteFn)(const ChainArgs&);
static int32_t chain_min_k0(ChainRouteFn route) { return route == chain_route_bf16 ? 0 : 1; }

static int chain_forward(rover_ctx* c, const rover_chain_desc& d, int32_t M, const char* what, ChainRouteFn route, void* stream) {
    if (!c) return ROVER_E_INVALID;
    ChainArgs a;
    if (int r = chain_args_of(c, d, M, what, &a, chain_min_k0(route))) return r;
    if (M == 0) return ROVER_OK;
    const ChainRoute r = route(a);
    if (r.kernel == ChainKernel::None) return chain_refused(c, what);
    USE_DEVICE(c);
    return chain_run(c, a, r, (hipStream_t)stream);
}

int rover_mlp_chain_forward(rover_ctx* c, const float* x, int64_t x_stride, int32_t M, int32_t K0, int32_t n_layers,
                            const float* const* weights, const float* const* biases, const int32_t* widths, const int32_t* activations,
                            float* y, int64_t y_stride, void* stream) {
    const rover_chain_desc d{x, x_stride, K0, n_layers, weights, biases, widths, activations, y, y_stride};
    return chain_forward(c, d, M, "mlp_chain_forward", chain_route, stream);
}

int rover_mlp_chain_forward_bf16(rover_ctx* c, const float* x, int64_t x_stride, int32_t M, int32_t K0, int32_t n_layers,
                                 const float* const* weights, const float* const* biases, const int32_t* widths, const int32_t* activations,
                                 float* y, int64_t y_stride, void* stream) {
    const rover_chain_desc d{x, x_stride, K0, n_layers, weights, biases, widths, activations, y, y_stride};
    return chain_forward(c, d, M, "mlp_chain_forward_bf16", chain_route_bf16, stream);
}

int rover_bf16_round(const float* in, int64_t n, float* out) {
    if (n < 0 || (n > 0 && (!in || !out))) return fail(nullptr, ROVER_E_INVALID, "bf16_round: bad arguments (n=%lld)", (long long)n);
    for (int64_t i = 0; i < n; ++i) out[i] = (float)bf16_rne(in[i]);
    return ROVER_OK;
}

int rover_mlp_chain_pair_forward(rover_ctx* c, int32_t M, const rover_chain_desc* da, const rover_chain_desc* db, const float* copy_src,
                                 int64_t copy_src_stride, float* copy_dst, int64_t copy_dst_stride, int32_t copy_cols, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!da || !db || copy_cols < 0 || (copy_cols > 0 && (!copy_src || !copy_dst || copy_src_stride < copy_cols || copy_dst_stride < copy_cols)))
        return fail(c, ROVER_E_INVALID, "mlp_chain_pair_forward: bad arguments (copy_cols=%d)", copy_cols);
    ChainArgs a, b;
    if (int r = chain_args_of(c, *da, M, "mlp_chain_pair_forward", &a)) return r;
    if (int r = chain_args_of(c, *db, M, "mlp_chain_pair_forward", &b)) return r;
    if (M == 0) return ROVER_OK;
    const ChainRoute ra = chain_route(a), rb = chain_route(b);
    if (ra.kernel == ChainKernel::None || rb.kernel == ChainKernel::None) return chain_refused(c, "mlp_chain_pair_forward");
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (chain_pair_side_by_side(ra, rb)) {
        const size_t fa = chain_splitk_scratch_floats(a.M, a.K0, a.n[0]), fb = chain_splitk_scratch_floats(b.M, b.K0, b.n[0]);
        if (int r = mlp_scratch_reserve(c, fa + fb, s)) return r;
        HIP_TRY(c, launch_chain_splitk_pair(a, b, ra, c->learn.mlp_scratch.get(), c->learn.mlp_scratch.get() + fa, copy_src, copy_src_stride, copy_dst,
                                            copy_dst_stride, copy_cols, s));
        return ROVER_OK;
    }
    if (copy_cols > 0)
        HIP_TRY(c, hipMemcpy2DAsync(copy_dst, (size_t)copy_dst_stride * sizeof(float), copy_src, (size_t)copy_src_stride * sizeof(float),
                                    (size_t)copy_cols * sizeof(float), (size_t)M, hipMemcpyDeviceToDevice, s));
    if (int r = chain_run(c, a, ra, s)) return r;
    return chain_run(c, b, rb, s);
}

// ---- route queries: what the forward calls above would launch, from the shapes alone (host only) ----
const char* rover_linear_route(int32_t M, int32_t K, int32_t N) {
    const LinearRoute r = linear_route(M, N);
    if (K < 0 || !r.nw) return nullptr;
    return M == 0 ? "none" : linear_route_name(r);
}

const char* rover_linear_route_bf16(int32_t M, int32_t K, int32_t N) {
    const char* name = linear_route_bf16_name(M, N);
    if (K < 0 || !name) return nullptr;
    return M == 0 ? "none" : name;
}

static const char* chain_route_query(int32_t M, int32_t K0, int32_t n_layers, const int32_t* widths, const int32_t* activations, ChainRouteFn route) {
    const rover_chain_desc d{nullptr, 0, K0, n_layers, nullptr, nullptr, widths, activations, nullptr, 0};      // a route query: shapes alone
    ChainArgs a;
    if (chain_shape_of(d, M, &a, chain_min_k0(route))) return nullptr;
    return M == 0 ? "none" : chain_route_name(route(a));
}
const char* rover_mlp_chain_route(int32_t M, int32_t K0, int32_t n_layers, const int32_t* widths, const int32_t* activations) {
    return chain_route_query(M, K0, n_layers, widths, activations, chain_route);
}
const char* rover_mlp_chain_route_bf16(int32_t M, int32_t K0, int32_t n_layers, const int32_t* widths, const int32_t* activations) {
    return chain_route_query(M, K0, n_layers, widths, activations, chain_route_bf16);
}

const char* rover_mlp_chain_pair_route(int32_t M, const rover_chain_desc* da, const rover_chain_desc* db) {
    ChainArgs a, b;
    if (!da || !db || chain_shape_of(*da, M, &a) || chain_shape_of(*db, M, &b)) return nullptr;
    if (M == 0) return "none";
    const ChainRoute ra = chain_route(a), rb = chain_route(b);
    if (ra.kernel == ChainKernel::None || rb.kernel == ChainKernel::None) return nullptr;
    static thread_local char name[96];
    char na[48];                                                     // (chain_route_name() may hand out one buffer twice)
    snprintf(na, sizeof na, "%s", chain_route_name(ra));
    if (chain_pair_side_by_side(ra, rb)) snprintf(name, sizeof name, "pair(%s)", na);
    else snprintf(name, sizeof name, "seq(%s;%s)", na, chain_route_name(rb));
    return name;
}

// ---- the Gaussian head ----
// the validated descriptor (0 = ok, else the error is recorded with c, or for rover_last_error(NULL) when c is null); no pointer is read
static int gauss_head_of(rover_ctx* c, const rover_gauss_head* g, int32_t M, bool given_mean, GaussHead* out) {
    if (!g) return fail(c, ROVER_E_INVALID, "gauss_head: null descriptor");
    if (g->A < 1 || g->A > GAUSS_MAX_A) return fail(c, ROVER_E_INVALID, "gauss_head: A = %d outside 1 .. %d", g->A, GAUSS_MAX_A);
    if (g->clip_log_std && !(g->min_log_std <= g->max_log_std))
        return fail(c, ROVER_E_INVALID, "gauss_head: min_log_std %g > max_log_std %g", (double)g->min_log_std, (double)g->max_log_std);
    if (g->clip_actions && !(g->low <= g->high)) return fail(c, ROVER_E_INVALID, "gauss_head: low %g > high %g", (double)g->low, (double)g->high);
    if (g->reduction < ROVER_REDUCE_SUM || g->reduction > ROVER_REDUCE_NONE) return fail(c, ROVER_E_INVALID, "gauss_head: unknown reduction %d", g->reduction);
    if (!g->log_std || !g->actions || !g->log_prob) return fail(c, ROVER_E_INVALID, "gauss_head: log_std, actions and log_prob must be given");
    const int lp_cols = g->reduction == ROVER_REDUCE_NONE ? g->A : 1;
    if (g->actions_stride < g->A || g->log_prob_stride < lp_cols || (g->taken_actions && g->taken_stride < g->A))
        return fail(c, ROVER_E_INVALID, "gauss_head: a row stride is shorter than its row (A = %d)", g->A);
    if (given_mean && (!g->mean || g->mean_stride < g->A)) return fail(c, ROVER_E_INVALID, "gauss_head: mean [M, A] must be given");
    if (M < 0 || g->row_offset < 0 || g->row_offset + (int64_t)M > (int64_t)1 << 32)
        return fail(c, ROVER_E_INVALID, "gauss_head: rows %lld .. + %d outside [0, 2^32)", (long long)g->row_offset, M);
    GaussHead h{};
    h.log_std = g->log_std; h.A = g->A; h.clip_log_std = g->clip_log_std != 0; h.clip_actions = g->clip_actions != 0;
    h.reduction = g->reduction; h.deterministic = g->deterministic != 0;
    h.min_log_std = g->min_log_std; h.max_log_std = g->max_log_std; h.low = g->low; h.high = g->high;
    h.seed = g->seed; h.step = g->step; h.step_dev = g->step_dev; h.row_offset = g->row_offset;
    h.taken = g->taken_actions; h.taken_stride = g->taken_stride;
    h.actions = g->actions; h.actions_stride = g->actions_stride; h.log_prob = g->log_prob; h.log_prob_stride = g->log_prob_stride;
    *out = h;
    return ROVER_OK;
}

static int chain_act(rover_ctx* c, const rover_chain_desc& d, int32_t M, const rover_gauss_head* head, const char* what, ChainRouteFn route,
                     void* stream) {
    if (!c) return ROVER_E_INVALID;
    ChainArgs a; GaussHead h{};
    if (int r = chain_args_of(c, d, M, what, &a, chain_min_k0(route))) return r;
    if (int r = gauss_head_of(c, head, M, false, &h)) return r;
    if (a.n[d.n_layers - 1] != h.A) return fail(c, ROVER_E_INVALID, "%s: the last layer is %d wide, the head has A = %d", what, a.n[d.n_layers - 1], h.A);
    if (M == 0) return ROVER_OK;
    const ChainRoute r = route(a);
    if (r.kernel == ChainKernel::None) return chain_refused(c, what);
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (chain_head_fused(r, h.A)) {
        HIP_TRY(c, launch_chain_head(a, r, h, s));
        return ROVER_OK;
    }
    if (int e = chain_run(c, a, r, s)) return e;
    HIP_TRY(c, launch_gaussian_head(a.y, a.y_stride, M, h, s));
    return ROVER_OK;
}

int rover_mlp_chain_act(rover_ctx* c, const float* x, int64_t x_stride, int32_t M, int32_t K0, int32_t n_layers, const float* const* weights,
                        const float* const* biases, const int32_t* widths, const int32_t* activations, float* y, int64_t y_stride,
                        const rover_gauss_head* head, void* stream) {
    const rover_chain_desc d{x, x_stride, K0, n_layers, weights, biases, widths, activations, y, y_stride};
    return chain_act(c, d, M, head, "mlp_chain_act", chain_route, stream);
}

int rover_mlp_chain_act_bf16(rover_ctx* c, const float* x, int64_t x_stride, int32_t M, int32_t K0, int32_t n_layers, const float* const* weights,
                             const float* const* biases, const int32_t* widths, const int32_t* activations, float* y, int64_t y_stride,
                             const rover_gauss_head* head, void* stream) {
    const rover_chain_desc d{x, x_stride, K0, n_layers, weights, biases, widths, activations, y, y_stride};
    return chain_act(c, d, M, head, "mlp_chain_act_bf16", chain_route_bf16, stream);
}

int rover_gaussian_head(rover_ctx* c, int32_t M, const rover_gauss_head* head, void* stream) {
    if (!c) return ROVER_E_INVALID;
    GaussHead h{};
    if (int r = gauss_head_of(c, head, M, true, &h)) return r;
    if (M == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_gaussian_head(head->mean, head->mean_stride, M, h, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_policy_noise(rover_ctx* c, uint64_t seed, uint64_t step, const uint64_t* step_dev, int64_t row_offset, int32_t M, int32_t A, float* eps,
                       int64_t eps_stride, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!eps || M < 0 || A < 1 || A > GAUSS_MAX_A || eps_stride < A || row_offset < 0 || row_offset + (int64_t)M > (int64_t)1 << 32)
        return fail(c, ROVER_E_INVALID, "policy_noise: bad arguments (M=%d A=%d row_offset=%lld)", M, A, (long long)row_offset);
    if (M == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_policy_noise(seed, step, step_dev, row_offset, M, A, eps, eps_stride, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_philox4x32(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
    if (!counter || !key || !out) return fail(nullptr, ROVER_E_INVALID, "philox4x32: null argument");
    uint32_t w[4] = {counter[0], counter[1], counter[2], counter[3]};
    philox4x32_10(w, key[0], key[1]);
    for (int i = 0; i < 4; ++i) out[i] = w[i];
    return ROVER_OK;
}

static const char* chain_act_route_query(int32_t M, int32_t K0, int32_t n_layers, const int32_t* widths, const int32_t* activations,
                                         const rover_gauss_head* head, ChainRouteFn route) {
    const rover_chain_desc d{nullptr, 0, K0, n_layers, nullptr, nullptr, widths, activations, nullptr, 0};
    ChainArgs a; GaussHead h{};
    if (chain_shape_of(d, M, &a, chain_min_k0(route))) {
        fail(nullptr, ROVER_E_INVALID, "mlp_chain_act_route: bad shapes (M=%d K0=%d layers=%d)", M, K0, n_layers);
        return nullptr;
    }
    if (gauss_head_of(nullptr, head, M, false, &h)) return nullptr;
    if (a.n[n_layers - 1] != h.A) {
        fail(nullptr, ROVER_E_INVALID, "mlp_chain_act_route: the last layer is %d wide, the head has A = %d", a.n[n_layers - 1], h.A);
        return nullptr;
    }
    if (M == 0) return "none";
    const char* name = chain_act_route_name(route(a), h.A);
    if (!name) fail(nullptr, ROVER_E_INVALID, "mlp_chain_act_route: net outside the built tile shapes");
    return name;
}
const char* rover_mlp_chain_act_route(int32_t M, int32_t K0, int32_t n_layers, const int32_t* widths, const int32_t* activations,
                                      const rover_gauss_head* head) {
    return chain_act_route_query(M, K0, n_layers, widths, activations, head, chain_route);
}
const char* rover_mlp_chain_act_route_bf16(int32_t M, int32_t K0, int32_t n_layers, const int32_t* widths, const int32_t* activations,
                                           const rover_gauss_head* head) {
    return chain_act_route_query(M, K0, n_layers, widths, activations, head, chain_route_bf16);
}

// ---- the learning entry points (each ends its argument checks with check_operands: rover_ctx.h) ----

// ---- rollout: GAE ----
int rover_gae(rover_ctx* c, const rover_gae_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "gae: null descriptor");
    if (d->T < 1 || d->T > 4096 || d->E < 0 || (int64_t)d->T * d->E >= (int64_t)1 << 31)
        return fail(c, ROVER_E_INVALID, "gae: T = %d outside 1 .. 4096, E = %d < 0, or T E >= 2^31", d->T, d->E);
    if (d->normalize < ROVER_GAE_RAW || d->normalize > ROVER_GAE_NORMALIZE_GIVEN) return fail(c, ROVER_E_INVALID, "gae: unknown normalize %d", d->normalize);
    if (d->E == 0) return ROVER_OK;            // nothing to read or write: no pointer is required
    const int32_t T = d->T, E = d->E;
    if (d->normalize == ROVER_GAE_NORMALIZE && (int64_t)T * E < 2)
        return fail(c, ROVER_E_INVALID, "gae: ROVER_GAE_NORMALIZE needs T E >= 2 (the unbiased std of one element is NaN)");
    Operands ops("gae");
    ops.read("rewards", d->rewards, d->rewards_stride, T, E, 4).read("values", d->values, d->values_stride, T, E, 4)
        .read("dones", d->dones, d->dones_stride, T, E, 1).read("last_values", d->last_values, E, 1, E, 4)
        .written("returns", d->returns, d->returns_stride, T, E, 4).written("advantages", d->advantages, d->advantages_stride, T, E, 4)
        .written("stats_out", d->stats_out, 3, 1, 3, 8, OP_OPTIONAL)
        .same_array("returns", "values");
    if (d->normalize == ROVER_GAE_NORMALIZE_GIVEN) ops.state("stats_in", d->stats_in, 3, 1, 3, 8);     // only read, but clear of every array
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    GaeArgs a{};
    a.T = d->T; a.E = (uint32_t)d->E; a.gamma = d->gamma; a.lam = d->lam;
    a.rewards = d->rewards; a.rewards_stride = d->rewards_stride; a.values = d->values; a.values_stride = d->values_stride;
    a.dones = d->dones; a.dones_stride = d->dones_stride; a.last_values = d->last_values;
    a.returns = d->returns; a.returns_stride = d->returns_stride; a.advantages = d->advantages; a.advantages_stride = d->advantages_stride;
    a.normalize = d->normalize; a.stats_out = d->stats_out; a.stats_in = d->normalize == ROVER_GAE_NORMALIZE_GIVEN ? d->stats_in : nullptr;
    a.partials = c->learn.gae_partials.get();
    HIP_TRY(c, launch_gae(a, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_combine_moments(const double* a, const double* b, double* out) {
    if (!a || !b || !out) return fail(nullptr, ROVER_E_INVALID, "combine_moments: null argument");
    gae_combine_moments(a, b, out);
    return ROVER_OK;
}

// ---- training: the backward of one Layer, the PPO loss ----
int rover_linear_backward(rover_ctx* c, const float* x, int64_t x_stride, const float* y, int64_t y_stride, const float* dy, int64_t dy_stride,
                          int32_t M, int32_t K, const float* weight, int32_t N, int32_t activation, float* dx, int64_t dx_stride, float* dweight,
                          float* dbias, void* stream) {
    const LinearBwdRoute r = linear_backward_route(M, K, N, dx != nullptr);
    if (!r.ok || activation < 0 || activation > 4)
        return fail(c, ROVER_E_INVALID, "linear_backward: M=%d K=%d N=%d act=%d outside M >= 0, K >= 0 (<= 256 with dx), 1 <= N <= 256, act 0 .. 4", M, K, N, activation);
    const bool need_x = dweight && K > 0, need_w = dx && K > 0;
    Operands ops("linear_backward");        // M = 0: the [M, .] operands have no element and need no pointer, their strides are checked all the same
    ops.read("dy", dy, dy_stride, M, N, 4);
    if (activation) ops.read("y", y, y_stride, M, N, 4);
    if (need_x) ops.read("x", x, x_stride, M, K, 4);
    if (need_w) ops.read("weight", weight, K, M > 0 ? N : 0, K, 4).written("dx", dx, dx_stride, M, K, 4);
    if (need_x) ops.written("dweight", dweight, K, M > 0 ? N : 0, K, 4);
    ops.written("dbias", dbias, N, M > 0 ? 1 : 0, N, 4, OP_OPTIONAL);     // (M = 0 only zeroes dweight / dbias: they were never checked there)
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    LinearBwdArgs a{x, x_stride, y, y_stride, dy, dy_stride, weight, dx, dx_stride, dweight, dbias, M, K, N, activation};
    if (M > 0 && (dweight || dbias))
        if (int e = mlp_scratch_reserve(c, linear_backward_scratch_floats(r, K, N), s)) return e;
    HIP_TRY(c, launch_linear_backward(a, r, c->learn.mlp_scratch.get(), s));
    return ROVER_OK;
}

const char* rover_linear_backward_route(int32_t M, int32_t K, int32_t N, int32_t want_dx) {
    const LinearBwdRoute r = linear_backward_route(M, K, N, want_dx != 0);
    if (!r.ok) return nullptr;
    return M == 0 ? "zero" : linear_backward_route_name(r);
}

int rover_linear_dgrad(rover_ctx* c, const float* y, int64_t y_stride, const float* dy, int64_t dy_stride, int32_t M, int32_t K, const float* weight,
                       int32_t N, int32_t activation, float* dx, int64_t dx_stride, void* stream) {
    const LinearRoute r = linear_dgrad_route(M, N, K);
    if (!r.nw || activation < 0 || activation > 4)
        return fail(c, ROVER_E_INVALID, "linear_dgrad: M=%d K=%d N=%d act=%d outside M >= 0, 1 <= K <= %d, N >= 1, act 0 .. 4", M, K, N, activation, 32 * 65535);
    if (M == 0) return ROVER_OK;
    Operands ops("linear_dgrad");
    ops.read("dy", dy, dy_stride, M, N, 4);
    if (activation) ops.read("y", y, y_stride, M, N, 4);
    ops.read("weight", weight, K, N, K, 4).written("dx", dx, dx_stride, M, K, 4);
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    LinearBwdArgs a{nullptr, 0, y, y_stride, dy, dy_stride, weight, dx, dx_stride, nullptr, nullptr, M, K, N, activation};
    HIP_TRY(c, launch_linear_dgrad(a, r, (hipStream_t)stream));
    return ROVER_OK;
}

const char* rover_linear_dgrad_route(int32_t M, int32_t K, int32_t N) {
    const LinearRoute r = linear_dgrad_route(M, N, K);
    if (!r.nw) return nullptr;
    return M == 0 ? "none" : linear_dgrad_route_name(r);
}

int rover_ppo_loss(rover_ctx* c, const rover_ppo_loss_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "ppo_loss: null descriptor");
    if (d->M < 0 || d->A < 1 || d->A > GAUSS_MAX_A) return fail(c, ROVER_E_INVALID, "ppo_loss: M = %d < 0 or A = %d outside 1 .. %d", d->M, d->A, GAUSS_MAX_A);
    if (d->reduction != ROVER_REDUCE_SUM) return fail(c, ROVER_E_INVALID, "ppo_loss: the log-prob reduction must be ROVER_REDUCE_SUM (got %d)", d->reduction);
    if (d->clip_log_std && !(d->min_log_std <= d->max_log_std))
        return fail(c, ROVER_E_INVALID, "ppo_loss: min_log_std %g > max_log_std %g", (double)d->min_log_std, (double)d->max_log_std);
    if (!(d->ratio_clip >= 0.0f) || (d->clip_predicted_values && !(d->value_clip >= 0.0f)))
        return fail(c, ROVER_E_INVALID, "ppo_loss: ratio_clip %g and value_clip %g must be >= 0", (double)d->ratio_clip, (double)d->value_clip);
    if (d->M == 0) return ROVER_OK;            // nothing to read or write: no pointer is required
    const int32_t M = d->M, A = d->A;
    Operands ops("ppo_loss");
    ops.read("mean", d->mean, d->mean_stride, M, A, 4).read("log_std", d->log_std, A, 1, A, 4).read("actions", d->actions, d->actions_stride, M, A, 4)
        .read("old_log_prob", d->old_log_prob, M, 1, M, 4).read("advantages", d->advantages, M, 1, M, 4).read("value", d->value, M, 1, M, 4)
        .read("old_values", d->old_values, M, 1, M, 4).read("returns", d->returns, M, 1, M, 4)
        .written("d_mean", d->d_mean, d->d_mean_stride, M, A, 4).written("d_value", d->d_value, M, 1, M, 4)
        .written("d_log_std", d->d_log_std, A, 1, A, 4).written("stats", d->stats, 4, 1, 4, 8);
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    PpoArgs a{};
    a.M = M; a.A = A; a.mean = d->mean; a.mean_stride = d->mean_stride; a.log_std = d->log_std; a.actions = d->actions; a.actions_stride = d->actions_stride;
    a.old_log_prob = d->old_log_prob; a.advantages = d->advantages; a.value = d->value; a.old_values = d->old_values; a.returns = d->returns;
    a.clip_log_std = d->clip_log_std != 0; a.min_log_std = d->min_log_std; a.max_log_std = d->max_log_std;
    a.ratio_clip = d->ratio_clip; a.value_clip = d->value_clip; a.clip_predicted_values = d->clip_predicted_values != 0;
    a.entropy_loss_scale = d->entropy_loss_scale; a.value_loss_scale = d->value_loss_scale;
    a.d_mean = d->d_mean; a.d_mean_stride = d->d_mean_stride; a.d_value = d->d_value; a.d_log_std = d->d_log_std; a.stats = d->stats;
    a.partials = c->learn.ppo_partials.get();
    HIP_TRY(c, launch_ppo_loss(a, (hipStream_t)stream));
    return ROVER_OK;
}

// ---- training: gradient-norm clip + Adam ----
// shared by rover_optim_plan and rover_optim_create: NULL when the sizes are acceptable, else what is wrong; *total = sum(numel)
static const char* optim_sizes_refused(int32_t n_tensors, const int64_t* numel, int64_t* total) {
    if (!numel) return "numel is NULL";
    if (n_tensors < 1 || n_tensors > 256) return "n_tensors outside 1 .. 256";
    int64_t sum = 0;
    for (int32_t i = 0; i < n_tensors; ++i) {
        if (numel[i] < 0) return "a negative numel";
        if (numel[i] >= (int64_t)1 << 31 || (sum += numel[i]) >= (int64_t)1 << 31) return "total elements >= 2^31";
    }
    *total = sum;
    return nullptr;
}

int rover_optim_plan(int32_t n_tensors, const int64_t* numel, rover_optim_chunk* chunks, int64_t capacity, int64_t* n_chunks) {
    int64_t total = 0;
    if (const char* why = optim_sizes_refused(n_tensors, numel, &total)) return fail(nullptr, ROVER_E_INVALID, "optim_plan: %s", why);
    if (!n_chunks) return fail(nullptr, ROVER_E_INVALID, "optim_plan: n_chunks is NULL");
    const int64_t n = optim_plan(n_tensors, numel, nullptr, 0);
    if (capacity < 0 || (chunks && capacity < n)) return fail(nullptr, ROVER_E_INVALID, "optim_plan: capacity %lld < %lld chunks", (long long)capacity, (long long)n);
    static_assert(sizeof(rover_optim_chunk) == sizeof(OptimChunkHost), "rover_optim_chunk is OptimChunkHost");
    if (chunks) (void)optim_plan(n_tensors, numel, reinterpret_cast<OptimChunkHost*>(chunks), capacity);
    *n_chunks = n;
    return ROVER_OK;
}

int rover_optim_create(rover_ctx* c, const rover_optim_desc* d, int32_t* handle) {
    if (!d || !handle || !d->params || !d->grads) return fail(c, ROVER_E_INVALID, "optim_create: null descriptor, handle, params or grads");
    int64_t total = 0;
    if (const char* why = optim_sizes_refused(d->n_tensors, d->numel, &total)) return fail(c, ROVER_E_INVALID, "optim_create: %s", why);
    Operands st("optim_create");        // the state by the operand rules (total = 0: the moments have no element); the tensor lists by the loops below
    st.state("step", d->step, 1, 1, 1, 8, 0, 8).state("stopped", d->stopped, 1, 1, 1, 4, 0, 4)
        .state("exp_avg", d->exp_avg, total, 1, total, 4, 0, 4).state("exp_avg_sq", d->exp_avg_sq, total, 1, total, 4, 0, 4);
    if (int e = check_operands(c, st, false)) return e;
    const int32_t n = d->n_tensors;
    std::vector<Span> ps, gs, state = {st.span(0), st.span(1)};         // the tensors with elements; the state with elements
    if (total > 0) state.insert(state.end(), {st.span(2), st.span(3)});
    for (int32_t i = 0; i < n; ++i) {
        if (d->numel[i] == 0) continue;
        if (!d->params[i] || !d->grads[i] || (uintptr_t)d->params[i] % 4 || (uintptr_t)d->grads[i] % 4)
            return fail(c, ROVER_E_INVALID, "optim_create: params[%d] or grads[%d] is NULL or misaligned", i, i);
        Span p, g;
        if (!span_of(d->params[i], d->numel[i], 1, d->numel[i], 4, &p) || !span_of(d->grads[i], d->numel[i], 1, d->numel[i], 4, &g))
            return fail(c, ROVER_E_INVALID, "optim_create: params[%d] or grads[%d]: extent too large", i, i);
        ps.push_back(p);
        gs.push_back(g);
    }
    for (size_t i = 0; i < ps.size(); ++i) {
        for (const Span& s : state)
            if (overlap(ps[i], s) || overlap(gs[i], s)) return fail(c, ROVER_E_INVALID, "optim_create: a parameter or a gradient overlaps the state");
        for (size_t j = 0; j < ps.size(); ++j)
            if (overlap(ps[i], gs[j]) || (j > i && overlap(ps[i], ps[j])))
                return fail(c, ROVER_E_INVALID, "optim_create: a parameter overlaps a gradient or another parameter");
    }
    if (!c) return fail(nullptr, ROVER_E_INVALID, "optim_create: null ctx");       // the ctx is only where the handle is kept
    USE_DEVICE(c);
    const int64_t n_chunks = optim_plan(n, d->numel, nullptr, 0);
    std::vector<OptimChunkHost> plan((size_t)n_chunks);
    (void)optim_plan(n, d->numel, plan.data(), n_chunks);
    std::vector<int64_t> offset((size_t)n, 0);                 // of tensor i in the flat state
    for (int32_t i = 1; i < n; ++i) offset[i] = offset[i - 1] + d->numel[i - 1];
    const bool state_al = ((uintptr_t)d->exp_avg | (uintptr_t)d->exp_avg_sq) % 16 == 0;
    std::vector<OptimChunk> table((size_t)n_chunks);
    for (int64_t k = 0; k < n_chunks; ++k) {
        const OptimChunkHost& h = plan[(size_t)k];
        OptimChunk& o = table[(size_t)k];
        o.p = d->params[h.tensor] + h.first;
        o.g = d->grads[h.tensor] + h.first;
        o.state = (uint32_t)(offset[h.tensor] + h.first);
        o.len = (uint32_t)h.length;
        o.flags = (((uintptr_t)d->params[h.tensor] | (uintptr_t)d->grads[h.tensor]) % 16 == 0 ? OPTIM_PG_ALIGNED : 0) |
                  (state_al && offset[h.tensor] % 4 == 0 ? OPTIM_STATE_ALIGNED : 0);
        o.pad = 0;
    }
    OptimHandle h;
    hipError_t e = h.record.alloc(1);
    if (e == hipSuccess && n_chunks > 0) e = h.chunks.alloc((size_t)n_chunks);
    if (e == hipSuccess && n_chunks > 0) e = h.partials.alloc((size_t)n_chunks);
    if (e == hipSuccess && n_chunks > 0) e = hipMemcpy(h.chunks.get(), table.data(), table.size() * sizeof(OptimChunk), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(h.record.get(), 0, sizeof(OptimRecord));
    if (e != hipSuccess) return fail(c, ROVER_E_HIP, "optim_create: %s", hipGetErrorString(e));
    h.live = true;
    h.n_chunks = (uint32_t)n_chunks;
    h.exp_avg = d->exp_avg; h.exp_avg_sq = d->exp_avg_sq; h.step = d->step; h.stopped = d->stopped;
    h.spans = state;
    h.spans.insert(h.spans.end(), ps.begin(), ps.end());
    h.spans.insert(h.spans.end(), gs.begin(), gs.end());
    size_t slot = 0;
    while (slot < c->learn.optims.size() && c->learn.optims[slot].live) ++slot;
    if (slot == c->learn.optims.size()) c->learn.optims.emplace_back();
    c->learn.optims[slot] = std::move(h);
    *handle = (int32_t)slot;
    return ROVER_OK;
}

static OptimHandle* optim_handle(rover_ctx* c, int32_t handle) {
    return handle >= 0 && (size_t)handle < c->learn.optims.size() && c->learn.optims[(size_t)handle].live ? &c->learn.optims[(size_t)handle] : nullptr;
}

int rover_optim_destroy(rover_ctx* c, int32_t handle) {
    if (!c) return ROVER_E_INVALID;
    OptimHandle* h = optim_handle(c, handle);
    if (!h) return fail(c, ROVER_E_INVALID, "optim_destroy: handle %d is not live", handle);
    USE_DEVICE(c);
    *h = OptimHandle{};                 // (the owners free their device memory)
    return ROVER_OK;
}

int rover_optim_step(rover_ctx* c, int32_t handle, const rover_optim_step_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "optim_step: null descriptor");
    if (!(d->lr >= 0.0) || !std::isfinite(d->lr) || !(d->beta1 >= 0.0 && d->beta1 < 1.0) || !(d->beta2 >= 0.0 && d->beta2 < 1.0) ||
        !(d->eps >= 0.0) || !std::isfinite(d->eps))
        return fail(c, ROVER_E_INVALID, "optim_step: lr %g and eps %g must be finite and >= 0, beta1 %g and beta2 %g in [0, 1)", d->lr, d->eps, d->beta1, d->beta2);
    if (std::isnan(d->grad_norm_clip) || std::isnan(d->gate_threshold)) return fail(c, ROVER_E_INVALID, "optim_step: grad_norm_clip or gate_threshold is NaN");
    Operands ops("optim_step");
    ops.read("gate", d->gate, 1, 1, 1, 8, OP_OPTIONAL, 8).written("norm_out", d->norm_out, 1, 1, 1, 8, OP_OPTIONAL, 8);
    if (int e = check_operands(c, ops)) return e;
    const OptimHandle* h = optim_handle(c, handle);
    if (!h) return fail(c, ROVER_E_INVALID, "optim_step: handle %d is not live", handle);
    Span out;
    if (d->norm_out && span_of(d->norm_out, 1, 1, 1, 8, &out))
        for (const Span& s : h->spans)
            if (overlap(out, s)) return fail(c, ROVER_E_INVALID, "optim_step: norm_out overlaps a parameter, a gradient or the state");
    USE_DEVICE(c);
    OptimArgs a{};
    a.chunks = h->chunks.get(); a.n_chunks = h->n_chunks; a.partials = h->partials.get(); a.record = h->record.get();
    a.exp_avg = h->exp_avg; a.exp_avg_sq = h->exp_avg_sq; a.step = h->step; a.stopped = h->stopped;
    a.lr = d->lr; a.beta1 = d->beta1; a.beta2 = d->beta2; a.eps = d->eps; a.clip = d->grad_norm_clip;
    a.gate = d->gate; a.gate_threshold = d->gate_threshold; a.norm_out = d->norm_out;
    HIP_TRY(c, launch_optim_step(a, (hipStream_t)stream));
    return ROVER_OK;
}

// ---- the student policy's recurrent block (rover_gru.hip) ----
static int gru_cell_run(rover_ctx* c, const char* what, const float* x, int64_t x_stride, const float* h_in, int64_t h_in_stride, int32_t M, int32_t K,
                        int32_t H, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const uint8_t* reset_mask, float* h_out,
                        int64_t h_out_stride, bool train, float* gates, int64_t gates_stride, void* stream,
                        hipError_t (*launch)(const GruArgs&, hipStream_t) = launch_gru_cell) {
    if (!gru_cell_route(M, K, H).nw) return fail(c, ROVER_E_INVALID, "%s: M=%d K=%d H=%d outside M >= 0, K >= 0, 1 <= H <= %d", what, M, K, H, 32 * 65535);
    if (M == 0) return ROVER_OK;                   // nothing is read or written: no pointer is required
    const int64_t G = (int64_t)3 * H;              // gate rows
    Operands ops(what);
    ops.read("h_in", h_in, h_in_stride, M, H, 4);  // (h_out may not even be h_in: a tile of h' needs whole rows of h that other workgroups still read)
    if (K > 0) ops.read("x", x, x_stride, M, K, 4).read("w_ih", w_ih, K, G, K, 4);
    ops.read("w_hh", w_hh, H, G, H, 4).read("b_ih", b_ih, G, 1, G, 4, OP_OPTIONAL).read("b_hh", b_hh, G, 1, G, 4, OP_OPTIONAL)
        .read("reset_mask", reset_mask, M, 1, M, 1, OP_OPTIONAL).written("h_out", h_out, h_out_stride, M, H, 4);
    if (train) ops.written("gates", gates, gates_stride, M, (int64_t)4 * H, 4);
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    GruArgs a{x, x_stride, h_in, h_in_stride, w_ih, w_hh, b_ih, b_hh, reset_mask, h_out, h_out_stride, M, K, H, train ? gates : nullptr, gates_stride};
    HIP_TRY(c, launch(a, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_gru_cell(rover_ctx* c, const float* x, int64_t x_stride, const float* h_in, int64_t h_in_stride, int32_t M, int32_t K, int32_t H,
                   const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const uint8_t* reset_mask, float* h_out,
                   int64_t h_out_stride, void* stream) {
    return gru_cell_run(c, "gru_cell", x, x_stride, h_in, h_in_stride, M, K, H, w_ih, w_hh, b_ih, b_hh, reset_mask, h_out, h_out_stride, false, nullptr, 0, stream);
}

int rover_gru_cell_bf16(rover_ctx* c, const float* x, int64_t x_stride, const float* h_in, int64_t h_in_stride, int32_t M, int32_t K, int32_t H,
                        const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const uint8_t* reset_mask, float* h_out,
                        int64_t h_out_stride, void* stream) {
    return gru_cell_run(c, "gru_cell_bf16", x, x_stride, h_in, h_in_stride, M, K, H, w_ih, w_hh, b_ih, b_hh, reset_mask, h_out, h_out_stride, false, nullptr, 0,
                        stream, launch_gru_cell_bf16);
}

int rover_gru_cell_train(rover_ctx* c, const float* x, int64_t x_stride, const float* h_in, int64_t h_in_stride, int32_t M, int32_t K, int32_t H,
                         const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const uint8_t* reset_mask, float* h_out,
                         int64_t h_out_stride, float* gates, int64_t gates_stride, void* stream) {
    return gru_cell_run(c, "gru_cell_train", x, x_stride, h_in, h_in_stride, M, K, H, w_ih, w_hh, b_ih, b_hh, reset_mask, h_out, h_out_stride, true, gates,
                        gates_stride, stream);
}

int rover_gru_cell_backward(rover_ctx* c, const float* dh_above, int64_t dh_above_stride, const float* dh_next, int64_t dh_next_stride, const float* gates,
                            int64_t gates_stride, const float* h_in, int64_t h_in_stride, const uint8_t* reset_mask, const float* w_hh, int32_t M, int32_t H,
                            float* dgi, int64_t dgi_stride, float* dgh, int64_t dgh_stride, float* dh_in, int64_t dh_in_stride, void* stream) {
    if (!gru_cell_backward_route(M, H).nw) return fail(c, ROVER_E_INVALID, "gru_cell_backward: M=%d H=%d outside M >= 0, 1 <= H <= %d", M, H, 32 * 65535);
    if (M == 0) return ROVER_OK;
    const int64_t G = (int64_t)3 * H;
    Operands ops("gru_cell_backward");
    ops.read("dh_above", dh_above, dh_above_stride, M, H, 4).read("dh_next", dh_next, dh_next_stride, M, H, 4, OP_OPTIONAL)
        .read("gates", gates, gates_stride, M, (int64_t)4 * H, 4).read("h_in", h_in, h_in_stride, M, H, 4)
        .read("reset_mask", reset_mask, M, 1, M, 1, OP_OPTIONAL).read("w_hh", w_hh, H, G, H, 4)
        .written("dgi", dgi, dgi_stride, M, G, 4).written("dgh", dgh, dgh_stride, M, G, 4).written("dh_in", dh_in, dh_in_stride, M, H, 4);
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    GruBwdArgs a{dh_above, dh_above_stride, dh_next, dh_next_stride, gates, gates_stride, h_in, h_in_stride, reset_mask, w_hh,
                 dgi, dgi_stride, dgh, dgh_stride, dh_in, dh_in_stride, M, H};
    HIP_TRY(c, launch_gru_cell_backward(a, (hipStream_t)stream));
    return ROVER_OK;
}

const char* rover_gru_cell_backward_route(int32_t M, int32_t H) {
    const GruRoute r = gru_cell_backward_route(M, H);
    if (!r.nw) return nullptr;
    return M == 0 ? "none" : gru_cell_backward_route_name(r);
}

const char* rover_gru_cell_route(int32_t M, int32_t K, int32_t H) {
    const GruRoute r = gru_cell_route(M, K, H);
    if (!r.nw) return nullptr;
    return M == 0 ? "none" : gru_cell_route_name(r);
}

const char* rover_gru_cell_route_bf16(int32_t M, int32_t K, int32_t H) {
    const char* name = gru_cell_route_bf16_name(M, K, H);
    if (!name) return nullptr;
    return M == 0 ? "none" : name;
}

int rover_gated_sum(rover_ctx* c, const float* add, int64_t add_stride, const float* mul, int64_t mul_stride, const float* pre, int64_t pre_stride,
                    int32_t M, int32_t N, float* out, int64_t out_stride, void* stream) {
    if (M < 0 || N < 1 || (int64_t)M * N >= (int64_t)1 << 38) return fail(c, ROVER_E_INVALID, "gated_sum: M=%d N=%d outside M >= 0, N >= 1, M N < 2^38", M, N);
    if (M == 0) return ROVER_OK;
    Operands ops("gated_sum");
    ops.read("add", add, add_stride, M, N, 4, OP_STRIDE0).read("mul", mul, mul_stride, M, N, 4, OP_STRIDE0).read("pre", pre, pre_stride, M, N, 4, OP_STRIDE0)
        .written("out", out, out_stride, M, N, 4);
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    GatedSumArgs a{add, add_stride, mul, mul_stride, pre, pre_stride, out, out_stride, M, N};
    HIP_TRY(c, launch_gated_sum(a, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_gated_sum_backward(rover_ctx* c, const float* d_out, int64_t d_out_stride, const float* mul, int64_t mul_stride, const float* pre,
                             int64_t pre_stride, int32_t M, int32_t N, float* d_mul, int64_t d_mul_stride, float* d_pre, int64_t d_pre_stride, void* stream) {
    if (M < 0 || N < 1 || (int64_t)M * N >= (int64_t)1 << 38)
        return fail(c, ROVER_E_INVALID, "gated_sum_backward: M=%d N=%d outside M >= 0, N >= 1, M N < 2^38", M, N);
    if (M == 0 || (!d_mul && !d_pre)) return ROVER_OK;
    Operands ops("gated_sum_backward");
    ops.read("d_out", d_out, d_out_stride, M, N, 4);
    if (d_pre) ops.read("mul", mul, mul_stride, M, N, 4, OP_STRIDE0);
    ops.read("pre", pre, pre_stride, M, N, 4, OP_STRIDE0).written("d_mul", d_mul, d_mul_stride, M, N, 4, OP_OPTIONAL)
        .written("d_pre", d_pre, d_pre_stride, M, N, 4, OP_OPTIONAL);
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    GatedSumBwdArgs a{d_out, d_out_stride, mul, mul_stride, pre, pre_stride, d_mul, d_mul_stride, d_pre, d_pre_stride, M, N};
    HIP_TRY(c, launch_gated_sum_backward(a, (hipStream_t)stream));
    return ROVER_OK;
}

}  // extern "C"
