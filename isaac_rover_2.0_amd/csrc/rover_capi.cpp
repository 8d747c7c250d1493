// rover_capi.cpp — the env step's unit of the C-ABI layer of librover_step.so (include/rover_step.h): context, library-owned device tables,
// planning and allocation, the knob table, kernel sequencing of the step and the ray cast, evaluation, resets, profiling.  It also defines
// fail, which rover_ctx.h declares for every unit, and keeps the thread's no-ctx error string.  The other units: rover_capi_scene.cpp (scene
// builders), rover_capi_learn.cpp (learning kernels), rover_capi_sim.cpp (sensor, motion, statistics).  No torch, no exceptions across the boundary.
#include "../../include/rover_step.h"
#include "rover_ctx.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

static const int kProfRing = 256;

static int prof_drain(rover_ctx* c) {
    for (int i = 0; i < c->prof_pending; ++i) {
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(c->ev1[i]);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev0[i], c->ev1[i]);
        if (e != hipSuccess) { c->prof_pending = 0; return ROVER_E_HIP; }
        c->prof_ms += ms;
    }
    c->prof_pending = 0;
    return ROVER_OK;
}

static thread_local std::string g_create_err;

int fail(rover_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_err = buf;
    return code;
}

static bool have_maps(const rover_ctx* c) { return c->maps[0].table.get() && c->maps[1].table.get(); }

// What plan_step reads, from the ctx: the only place that reads it for planning
static PlanInputs plan_inputs(const rover_ctx* c) {
    PlanInputs in;
    in.num_envs = c->cfg.num_envs; in.P = c->P; in.have_dist = c->have_dist; in.precision = c->precision; in.knobs = c->knobs;
    for (int w = 0; w < 2; ++w) {
        const MapTables& m = c->maps[w];
        MapShape& s = in.map[w];
        s.present = m.table.get() != nullptr;
        s.X = m.knn.X; s.Y = m.knn.Y; s.K8 = m.knn.K8; s.cells = m.cells; s.farok = m.farok;
        s.has_cull_tables = m.cull_idx.get() != nullptr;
        for (int k = 0; k < 2; ++k) s.has_staged_tables[k] = m.proof[k].lrec.get() != nullptr;
    }
    return in;
}

static uint32_t bucket_count(const StepPlan& p) { return (uint32_t)((p.n_bins + (1u << p.low_bits) - 1u) >> p.low_bits); }

// the sort's tables, for the bins and the digit the plan says
static int alloc_bins(rover_ctx* c) {
    const StepPlan& p = c->plan;
    c->bins_ok = false;
    if (!have_maps(c)) return ROVER_OK;
    if (p.n_bins > 0xfffffffeull) return fail(c, ROVER_E_INVALID, "too many map cells for ray binning");
    if (!c->d_block_sums.get()) HIP_TRY(c, c->d_block_sums.alloc(2 * 4096 + 8));   // bucket totals + bucket starts
    if (c->have_dist) {                                   // table size depends on E*R8 too
        const uint64_t n_blocks = ((uint64_t)c->cfg.num_envs * p.R8 + 4095) / 4096;
        HIP_TRY(c, c->d_bkt_table.alloc((uint64_t)bucket_count(p) * n_blocks + 1));
        // zero from the start, here and not in the first step: a first step that is only CAPTURED (hipGraph) would record the clearing
        // without running it, and an eager step after it would count into whatever the allocation held
        HIP_TRY(c, hipMemset(c->d_bkt_table.get(), 0, c->d_bkt_table.bytes()));
        c->bkt_table_dirty = false;
        c->bins_ok = true;
    }
    return ROVER_OK;
}

// the candidate queue and its per-wave counters, as large as the plan says (nothing to do for a plan without a queue)
static int alloc_cull_queue(rover_ctx* c) {
    const StepPlan& p = c->plan;
    CullQueue& q = c->queue;
    if (!c->ws_ok || !p.queue_entries) return ROVER_OK;
    // (the counters are sized by the ray count, the queue — once capped by the budget — is not: a second rover_set_distribution with more
    //  rays must grow the counters even when the queue keeps its size)
    const bool fits = q.entries.get() && q.stats.get() && p.queue_entries == q.sized_for.queue_entries && p.stat_slots == q.sized_for.stat_slots;
    q.sized_for = p;
    if (fits) return ROVER_OK;
    q.entries.reset(); q.stats.reset();
    // no fallback to another kernel: a queue that cannot be allocated is an error the caller sees
    if (hipError_t e = q.entries.alloc(p.queue_entries))
        return fail(c, ROVER_E_NOMEM, "culled ray cast: candidate queue of %llu bytes: %s", (unsigned long long)(p.queue_entries * sizeof(uint2)), hipGetErrorString(e));
    HIP_TRY(c, q.stats.alloc(p.stat_slots));
    q.counters_written_under = StepPlan{};
    HIP_TRY(c, hipMemset(q.stats.get(), 0, q.stats.bytes()));
    return ROVER_OK;
}

static int alloc_workspace(rover_ctx* c);

// Every change of a plan input ends here: the plan, then the buffers it sizes — `what` names those beyond the queue that the change can
// resize — here, never in a step (hipMalloc is not allowed while a stream is capturing).  r: the caller's own result; after an error the
// plan is still brought up to date (rover_get_info reports it), and the buffers are left as they are.
enum Realloc { REALLOC_QUEUE, REALLOC_BINS, REALLOC_WORKSPACE };
static int replan(rover_ctx* c, Realloc what = REALLOC_QUEUE, int r = ROVER_OK) {
    c->plan = plan_step(plan_inputs(c));
    if (!r && what == REALLOC_WORKSPACE) r = alloc_workspace(c);
    if (!r && what == REALLOC_BINS) r = alloc_bins(c);
    return r ? r : alloc_cull_queue(c);
}

static int alloc_workspace(rover_ctx* c) {
    c->ws_ok = false;
    c->d_rays.reset(); c->d_dist_out.reset(); c->d_euler.reset(); c->d_heading.reset(); c->d_sorted.reset();
    c->d_bins.reset(); c->d_pairs.reset();
    const uint64_t E = (uint64_t)c->cfg.num_envs;
    const uint64_t n = E * c->plan.R8;
    if (n > 0xffffffffull) return fail(c, ROVER_E_INVALID, "num_envs * rays_per_env = %llu exceeds 2^32", (unsigned long long)n);
    HIP_TRY(c, c->d_rays.alloc(n));
    HIP_TRY(c, c->d_dist_out.alloc(n));
    HIP_TRY(c, c->d_euler.alloc(E * 3));
    HIP_TRY(c, c->d_heading.alloc(E));
    HIP_TRY(c, c->d_sorted.alloc(n));
    HIP_TRY(c, c->d_bins.alloc(n));
    HIP_TRY(c, c->d_pairs.alloc(n));
    HIP_TRY(c, hipMemset(c->d_euler.get(), 0, c->d_euler.bytes()));
    HIP_TRY(c, hipMemset(c->d_heading.get(), 0, c->d_heading.bytes()));
    c->workspace_bytes = n * (sizeof(RayRec) + sizeof(float) + 2 * sizeof(uint32_t) + sizeof(uint2)) + E * (4 * sizeof(float) + sizeof(int64_t));
    c->rays_valid = false;
    c->obs_valid = false;
    c->ws_ok = true;
    return alloc_bins(c);
}


// ---- internal triangle numbering of the culled ray cast's tables (rover_set_knn_map) -----------------------------------------
// The caller's triangle order means nothing (a decimated .ply lists triangles in no spatial order), but the kernel gains from
// two properties of the ids it works with: (i) consecutive ids are neighbours in space (one gather instruction of a wave then
// touches few cache lines, and bins that follow each other re-use each other's records in L2), (ii) a lane's packed pair holds two
// triangles that are candidates for the same rays (a queue entry then carries two candidates: fewer entries, fewer exact-phase
// lanes).  So: triangles are matched into spatial partners — mutual nearest centroids first (on a grid mesh exactly the two
// halves of every mesh cell), then greedily the nearest unmatched neighbour — and a pair gets the ids 2p, 2p + 1, pairs in
// Morton order of their first member; an unmatched triangle gets 2p and leaves 2p + 1 a hole.  order[new] = old (0xffffffff =
// hole), newid[old] = new.  A min over the same set of triangles does not depend on the numbering: results are unchanged.
static void cull_numbering(const std::vector<float2>& cen, std::vector<uint32_t>& order, std::vector<uint32_t>& newid) {
    const uint32_t T = (uint32_t)cen.size(), NONE = 0xffffffffu;
    auto finite = [](const float2& p) { return std::fabs(p.x) < 1e30f && std::fabs(p.y) < 1e30f; };
    float bx0 = 0.f, bx1 = 0.f, by0 = 0.f, by1 = 0.f;
    bool any = false;
    uint32_t n_fin = 0;
    for (const float2& p : cen) {
        if (!finite(p)) continue;
        ++n_fin;
        if (!any) { bx0 = bx1 = p.x; by0 = by1 = p.y; any = true; }
        bx0 = p.x < bx0 ? p.x : bx0; bx1 = p.x > bx1 ? p.x : bx1; by0 = p.y < by0 ? p.y : by0; by1 = p.y > by1 ? p.y : by1;
    }
    // Morton rank (16 bits per axis of the bounding box; broken triangles last)
    const double sx = bx1 > bx0 ? 65535.0 / ((double)bx1 - bx0) : 0.0, sy = by1 > by0 ? 65535.0 / ((double)by1 - by0) : 0.0;
    auto spread = [](uint32_t v) {                     // 16 bits -> every second bit of 32
        v = (v | (v << 8)) & 0x00ff00ffu; v = (v | (v << 4)) & 0x0f0f0f0fu;
        v = (v | (v << 2)) & 0x33333333u; v = (v | (v << 1)) & 0x55555555u;
        return v;
    };
    std::vector<uint64_t> key((size_t)T);
    for (uint32_t t = 0; t < T; ++t) {
        uint32_t m = 0xffffffffu;
        if (finite(cen[t])) m = (spread((uint32_t)(((double)cen[t].x - bx0) * sx)) << 1) | spread((uint32_t)(((double)cen[t].y - by0) * sy));
        key[t] = ((uint64_t)m << 32) | t;
    }
    std::sort(key.begin(), key.end());
    // uniform hash grid over the centroids, ~4 per bucket at mean density
    const double area = ((double)bx1 - bx0 + 1e-6) * ((double)by1 - by0 + 1e-6);
    double h = std::sqrt(area * 4.0 / (double)(n_fin ? n_fin : 1));
    uint32_t gx = (uint32_t)(((double)bx1 - bx0) / h) + 1, gy = (uint32_t)(((double)by1 - by0) / h) + 1;
    while ((uint64_t)gx * gy > (1u << 24)) { h *= 2.0; gx = (uint32_t)(((double)bx1 - bx0) / h) + 1; gy = (uint32_t)(((double)by1 - by0) / h) + 1; }
    auto bucket = [&](const float2& p, uint32_t& ix, uint32_t& iy) {
        ix = (uint32_t)(((double)p.x - bx0) / h); iy = (uint32_t)(((double)p.y - by0) / h);
        ix = ix >= gx ? gx - 1 : ix; iy = iy >= gy ? gy - 1 : iy;
    };
    std::vector<uint32_t> start((size_t)gx * gy + 1, 0), items((size_t)n_fin);
    for (uint32_t t = 0; t < T; ++t) if (finite(cen[t])) { uint32_t ix, iy; bucket(cen[t], ix, iy); ++start[(size_t)ix * gy + iy + 1]; }
    for (size_t b = 0; b < (size_t)gx * gy; ++b) start[b + 1] += start[b];
    {
        std::vector<uint32_t> cur(start.begin(), start.end() - 1);
        for (uint32_t t = 0; t < T; ++t) if (finite(cen[t])) { uint32_t ix, iy; bucket(cen[t], ix, iy); items[cur[(size_t)ix * gy + iy]++] = t; }
    }
    std::vector<uint32_t> partner((size_t)T, NONE);
    // nearest other centroid in the 3 x 3 buckets around t among those for which ok(u); ties by id
    auto nearest = [&](uint32_t t, auto&& ok) {
        uint32_t ix, iy, best = NONE;
        bucket(cen[t], ix, iy);
        double bd = 1e300;
        for (uint32_t a = ix ? ix - 1 : 0; a <= (ix + 1 < gx ? ix + 1 : gx - 1); ++a)
            for (uint32_t b = iy ? iy - 1 : 0; b <= (iy + 1 < gy ? iy + 1 : gy - 1); ++b)
                for (uint32_t k = start[(size_t)a * gy + b]; k < start[(size_t)a * gy + b + 1]; ++k) {
                    const uint32_t u = items[k];
                    if (u == t || !ok(u)) continue;
                    const double dx = (double)cen[u].x - cen[t].x, dy = (double)cen[u].y - cen[t].y, d = dx * dx + dy * dy;
                    if (d < bd || (d == bd && u < best)) { bd = d; best = u; }
                }
        return best;
    };
    {   // pass 1: mutual nearest neighbours
        std::vector<uint32_t> nn((size_t)T, NONE);
        for (uint32_t t = 0; t < T; ++t) if (finite(cen[t])) nn[t] = nearest(t, [](uint32_t) { return true; });
        for (uint32_t t = 0; t < T; ++t) if (nn[t] != NONE && nn[t] > t && nn[nn[t]] == t) { partner[t] = nn[t]; partner[nn[t]] = t; }
    }
    // pass 2, in Morton order: the nearest still unmatched neighbour
    for (uint32_t r = 0; r < T; ++r) {
        const uint32_t t = (uint32_t)key[r];
        if (partner[t] != NONE || !finite(cen[t])) continue;
        const uint32_t u = nearest(t, [&](uint32_t v) { return partner[v] == NONE; });
        if (u != NONE) { partner[t] = u; partner[u] = t; }
    }
    order.clear();
    order.reserve((size_t)T + T / 8);
    std::vector<uint8_t> done((size_t)T, 0);
    for (uint32_t r = 0; r < T; ++r) {
        const uint32_t t = (uint32_t)key[r];
        if (done[t]) continue;
        const uint32_t u = partner[t];
        done[t] = 1;
        newid[t] = (uint32_t)order.size(); order.push_back(t);
        if (u != NONE) { done[u] = 1; newid[u] = (uint32_t)order.size(); order.push_back(u); }
        else order.push_back(NONE);
    }
}

// rover_set_knn_map's work, into `m` alone: the re-packed map, then — where the culled ray cast can serve the map (64 lanes x 4 triangles;
// triangle ids and the map bit share 32 bits of a queue entry) — its tables, then the staged kernel's.  The build's own buffers go on return.
static int build_map_tables(rover_ctx* c, MapTables& m, int which, const int32_t* map_idx, int32_t X, int32_t Y, int32_t K, const int32_t* tris,
                            int32_t T, const uint16_t* verts, int32_t V, float cell, float shift_x, float shift_y) {
    const uint64_t n_cells = (uint64_t)X * Y;
    const uint32_t K8 = (uint32_t)((K + 7) / 8 * 8);
    DevBuf<int32_t> d_idx, d_tris;
    DevBuf<uint16_t> d_verts;
    hipError_t e;
    if ((e = d_idx.alloc(n_cells * K)) != hipSuccess || (e = d_tris.alloc((uint64_t)T * 3)) != hipSuccess ||
        (e = d_verts.alloc((uint64_t)V * 3)) != hipSuccess || (e = m.table.alloc(n_cells * 9ull * K8)) != hipSuccess)
        return fail(c, ROVER_E_NOMEM, "set_knn_map: hipMalloc (%llu B table): %s", (unsigned long long)(n_cells * 9ull * K8 * sizeof(uint16_t)),
                    hipGetErrorString(e));
    if ((e = hipMemcpy(d_idx.get(), map_idx, d_idx.bytes(), hipMemcpyDefault)) != hipSuccess ||
        (e = hipMemcpy(d_tris.get(), tris, d_tris.bytes(), hipMemcpyDefault)) != hipSuccess ||
        (e = hipMemcpy(d_verts.get(), verts, d_verts.bytes(), hipMemcpyDefault)) != hipSuccess ||
        (e = launch_repack(d_idx.get(), d_tris.get(), d_verts.get(), n_cells, (uint32_t)K, K8, (uint32_t)T, (uint32_t)V, m.table.get(), nullptr)) != hipSuccess ||
        (e = hipDeviceSynchronize()) != hipSuccess)
        return fail(c, ROVER_E_HIP, "set_knn_map: %s", hipGetErrorString(e));
    m.knn = KnnDev{m.table.get(), X, Y, K, (int32_t)K8, cell, shift_x, shift_y, 1.0f / cell};
    m.lane_pp = lane_pairs_per_row(K8);
    m.tris = T; m.cells = (int64_t)n_cells;
    if (K8 > 256 || (uint32_t)T >= 0x1ffffffu) return ROVER_OK;
    // internal triangle numbering (spatial partners get ids 2p, 2p + 1, pairs ordered along a Morton curve): cull_numbering()
    std::vector<uint32_t> order, newid((size_t)T);
    {
        DevBuf<float2> d_cen;
        std::vector<float2> cen((size_t)T);
        if ((e = d_cen.alloc(T)) != hipSuccess ||
            (e = launch_tri_centroids(d_tris.get(), d_verts.get(), (uint32_t)T, (uint32_t)V, d_cen.get(), nullptr)) != hipSuccess ||
            (e = hipMemcpy(cen.data(), d_cen.get(), d_cen.bytes(), hipMemcpyDeviceToHost)) != hipSuccess)
            return fail(c, ROVER_E_HIP, "set_knn_map: triangle centroids: %s", hipGetErrorString(e));
        cull_numbering(cen, order, newid);
    }
    const uint32_t T_int = (uint32_t)order.size();
    if (T_int >= 0x3ffffffu) return fail(c, ROVER_E_INVALID, "set_knn_map: too many triangles for the culled ray cast's 26-bit ids");
    // the culled ray cast's tables and the build's buffers (qrow: per cell and proof, read only by the build kernels)
    DevBuf<uint32_t> d_qrow[2], d_order, d_newid, d_cnt;
    DevBuf<float> d_nz;
    if ((e = m.cull_idx.alloc(n_cells * K8)) != hipSuccess || (e = m.rtab.alloc((uint64_t)T_int * 10u)) != hipSuccess ||
        (e = m.proof[0].ctab.alloc(T_int)) != hipSuccess || (e = m.proof[1].ctab.alloc(T_int)) != hipSuccess ||
        (e = m.proof[0].far.alloc(3 * n_cells)) != hipSuccess || (e = m.proof[1].far.alloc(3 * n_cells)) != hipSuccess ||
        (e = d_qrow[0].alloc(n_cells)) != hipSuccess || (e = d_qrow[1].alloc(n_cells)) != hipSuccess || (e = d_nz.alloc(T_int)) != hipSuccess ||
        (e = d_cnt.alloc(8)) != hipSuccess || (e = d_order.alloc(T_int)) != hipSuccess || (e = d_newid.alloc(T)) != hipSuccess)
        return fail(c, ROVER_E_HIP, "set_knn_map: cull tables: %s", hipGetErrorString(e));
    // The staged kernel's tables are optional, each proof's on its own: which proofs get them is the "staged_tables" option, and an allocation
    // that fails drops that proof's (the culled kernel then runs for it, plan_step) — unless variant 4 was asked for by name.
    for (int k = 0; k < 2; ++k) {
        if (!((c->knobs.staged_tables >> k) & 1)) continue;
        ProofTables& p = m.proof[k];
        if ((e = p.lvl.alloc(n_cells * lane_lvl_stride())) != hipSuccess || (e = p.lrec.alloc(n_cells * 2ull * m.lane_pp)) != hipSuccess ||
            (e = p.lid.alloc(n_cells * m.lane_pp)) != hipSuccess) {
            p.lvl.reset(); p.lrec.reset(); p.lid.reset();
            if (c->knobs.variant == 4)
                return fail(c, ROVER_E_NOMEM, "set_knn_map: the staged ray cast's tables (%llu B per proof) do not fit and raycast_variant 4 was requested: %s",
                            (unsigned long long)(n_cells * ((uint64_t)lane_lvl_stride() * sizeof(float4) + (uint64_t)m.lane_pp * (2 * sizeof(uint4) + sizeof(uint2)))),
                            hipGetErrorString(e));
        }
    }
    CullBuildArgs a{};
    a.map_idx = d_idx.get(); a.tris = d_tris.get(); a.verts = d_verts.get();
    a.n_cells = n_cells; a.K = (uint32_t)K; a.K8 = K8; a.T = (uint32_t)T; a.T_int = T_int; a.V = (uint32_t)V;
    a.order = d_order.get(); a.newid = d_newid.get(); a.idx4 = m.cull_idx.get(); a.rtab = m.rtab.get();
    a.ctab = m.proof[0].ctab.get(); a.ctab_h = m.proof[1].ctab.get(); a.qrow = d_qrow[0].get(); a.qrow_h = d_qrow[1].get();
    a.far = m.proof[0].far.get(); a.far_h = m.proof[1].far.get(); a.nz_scratch = d_nz.get(); a.counts = d_cnt.get();
    a.ph = cull_proof_h(c->knobs.cull_eta_h, c->knobs.cull_split_h); a.Y = (uint32_t)Y; a.cell_size = cell; a.shift_x = shift_x; a.shift_y = shift_y;
    a.lane = m.proof[0].view(); a.lane_h = m.proof[1].view();
    uint32_t h_cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((e = hipMemcpy(d_order.get(), order.data(), d_order.bytes(), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(d_newid.get(), newid.data(), d_newid.bytes(), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemset(d_cnt.get(), 0, d_cnt.bytes())) != hipSuccess || (e = launch_cull_build(a, nullptr)) != hipSuccess ||
        (e = hipDeviceSynchronize()) != hipSuccess || (e = hipMemcpy(h_cnt, d_cnt.get(), sizeof h_cnt, hipMemcpyDeviceToHost)) != hipSuccess)
        return fail(c, ROVER_E_HIP, "set_knn_map: cull tables (%llu B): %s", (unsigned long long)m.bytes(), hipGetErrorString(e));
    m.proof[0].always = h_cnt[0]; m.proof[0].nocone = h_cnt[1];
    m.proof[1].always = h_cnt[2]; m.proof[1].nocone = h_cnt[3];
    m.farok = h_cnt[4];
    const bool box = a.lane.lrec && (c->knobs.lane_box > 0 || (c->knobs.lane_box < 0 && lane_box_share_met(h_cnt[5], h_cnt[6])));
    // One row per two cells (option "lane_pair_rows": auto = the terrain map, whose cells nearly all hold rays, so that a row is read once for
    // the rays of both): taken where every row's union fits a row — else the map keeps the per-cell tables built above.  The tables are
    // allocated again for the form (rows of the largest union: about 0.6 of the per-cell size); as before, a proof whose tables do not fit goes without.
    if ((a.lane.lrec || a.lane_h.lrec) && n_cells < (1ull << 24) && (uint32_t)T < (1u << 30) &&
        (c->knobs.lane_pair_rows > 0 || (c->knobs.lane_pair_rows < 0 && which == ROVER_MAP_TERRAIN))) {
        const uint64_t n_rows = lane_pair_rows_count(n_cells, (uint32_t)Y);
        DevBuf<uint2> d_upair;
        if (d_upair.alloc(n_rows * 128ull) == hipSuccess) {
            if ((e = launch_lane_union(a, d_upair.get(), nullptr)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess ||
                (e = hipMemcpy(h_cnt + 7, d_cnt.get() + 7, sizeof(uint32_t), hipMemcpyDeviceToHost)) != hipSuccess)
                return fail(c, ROVER_E_HIP, "set_knn_map: staged tables, the rows' unions: %s", hipGetErrorString(e));
            const uint32_t pp = lane_pair_rows_pp(h_cnt[7]);
            if (pp) {
                for (int k = 0; k < 2; ++k) {
                    ProofTables& p = m.proof[k];
                    if (!p.lrec.get()) continue;
                    p.lvl.reset(); p.lrec.reset(); p.lid.reset();
                    if (p.lvl.alloc(n_rows * lane_lvl_stride()) != hipSuccess || p.lrec.alloc(n_rows * 2ull * pp) != hipSuccess ||
                        p.lid.alloc(n_rows * pp) != hipSuccess) { p.lvl.reset(); p.lrec.reset(); p.lid.reset(); }
                }
                a.lane = m.proof[0].view(); a.lane_h = m.proof[1].view();
                if ((e = launch_lane_pair_rows(a, d_upair.get(), pp, box ? 1 : 0, nullptr)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess)
                    return fail(c, ROVER_E_HIP, "set_knn_map: staged tables in shared-row form: %s", hipGetErrorString(e));
                m.lane_pp = pp; m.lane_pair_rows = true; m.lane_box = box && a.lane.lrec;
                return ROVER_OK;
            }
        }
    }
    // the form of test (A)'s records in the f32 proof's staged tables (option "lane_box"): boxes where most pairs fill theirs
    if (box) {
        if ((e = launch_lane_box(a, nullptr)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess)
            return fail(c, ROVER_E_HIP, "set_knn_map: staged tables in box form: %s", hipGetErrorString(e));
        m.lane_box = true;
    }
    return ROVER_OK;
}

// ---- knobs: one table for the ROVER_* environment (rover_create) and rover_set_option -------------------------------------------------
// What a change invalidates, and how the two sides differ where they do, are data of the row.
enum : unsigned { KNOB_REPLAN = 1, KNOB_BINS = 2, KNOB_RAYS_OBS = 4 };      // the plan; the sort's tables too; the ray workspace and the obs state
enum : unsigned {
    KNOB_OPT_ALSO_ZERO = 1,     // the option accepts 0 (the library's choice) beside its range; the environment only the range
    KNOB_ENV_AS_BOOL = 2,       // the environment's value is read as v != 0
    KNOB_REAL = 4,              // a real number (atof), else an integer (atol)
    KNOB_MUST_RUN = 8,          // the option names a kernel: a variant that cannot run is refused (staged_tables_missing)
};
struct KnobRow {
    const char* option;         // rover_set_option name, or NULL
    const char* env;            // read at rover_create, or NULL
    double opt_lo, opt_hi;      // accepted by the option; anything else is ROVER_E_INVALID
    double env_lo, env_hi;      // accepted from the environment; anything else is ignored
    unsigned flags;
    void (*set)(rover_ctx*, double);
    unsigned invalidates;
    const char* values;         // the option's accepted values in words (its error message)
};
#define KNOB_SET(field, expr) [](rover_ctx* c, double v) { c->field = (expr); }
static const double kIntMin = -2147483648.0, kIntMax = 2147483647.0, kLongMax = 9223372036854775807.0;
static const KnobRow kKnobs[] = {
    {"raycast_variant", "ROVER_RAYCAST_VARIANT", 0, 4, 1, 4, KNOB_MUST_RUN, KNOB_SET(knobs.variant, (int)v), KNOB_REPLAN,
     "0 (auto), 1 (env order), 2 (binned), 3 (culled) or 4 (staged)"},
    {"raycast_run", "ROVER_RAYCAST_RUN", 0, 4096, 1, 4096, 0, KNOB_SET(knobs.run, (uint32_t)v), KNOB_REPLAN, "0 (auto) or in [1, 4096]"},
    {"lane_env_order", "ROVER_LANE_ENV_ORDER", -1, 1, kIntMin, kIntMax, KNOB_ENV_AS_BOOL, KNOB_SET(knobs.lane_env_order, (int)v), KNOB_REPLAN,
     "-1 (auto), 0 or 1"},
    {"lane_rocks", "ROVER_LANE_ROCKS", -1, 1, kIntMin, kIntMax, KNOB_ENV_AS_BOOL, KNOB_SET(knobs.lane_rocks, (int)v), KNOB_REPLAN, "-1 (auto), 0 or 1"},
    {"lane_box", "ROVER_LANE_BOX", -1, 1, kIntMin, kIntMax, KNOB_ENV_AS_BOOL, KNOB_SET(knobs.lane_box, (int)v), 0,      // takes effect at the next rover_set_knn_map
     "-1 (auto), 0 or 1"},
    {"lane_pair_rows", "ROVER_LANE_PAIR_ROWS", -1, 1, kIntMin, kIntMax, KNOB_ENV_AS_BOOL, KNOB_SET(knobs.lane_pair_rows, (int)v), 0,      // (the same)
     "-1 (auto), 0 or 1"},
    {"lane_rebase", "ROVER_LANE_REBASE", 0, 1, kIntMin, kIntMax, KNOB_ENV_AS_BOOL, KNOB_SET(lane_rebase, (int32_t)v), 0,      // read at every launch: no plan, no table depends on it
     "0 or 1"},
    {nullptr, "ROVER_CULL_LAZY", 1, 0, kIntMin, kIntMax, 0, KNOB_SET(knobs.cull_lazy, (int)v), KNOB_REPLAN, nullptr},
    {"bin_low_bits", "ROVER_BIN_LOW_BITS", 8, 12, 8, 12, KNOB_OPT_ALSO_ZERO, KNOB_SET(knobs.low_bits_opt, (uint32_t)v), KNOB_REPLAN | KNOB_BINS,
     "0 (chosen by the library) or in [8, 12]"},
    {"cull_queue_mb", "ROVER_CULL_QUEUE_MB", 1, 1 << 20, 1, kLongMax, 0, KNOB_SET(knobs.cull_budget, (uint64_t)v << 20), KNOB_REPLAN, "in [1, 1048576]"},
    {nullptr, "ROVER_CULLH_ETA", 1, 0, 0.02, 0.5, KNOB_REAL, KNOB_SET(knobs.cull_eta_h, v), 0, nullptr},
    {nullptr, "ROVER_CULLH_SPLIT", 1, 0, 0.5, 64.0, KNOB_REAL, KNOB_SET(knobs.cull_split_h, v), 0, nullptr},
    {"staged_tables", nullptr, 0, 3, 1, 0, 0, KNOB_SET(knobs.staged_tables, (int)v), 0,      // takes effect at the next rover_set_knn_map
     "0 (none), 1 (f32 proof), 2 (as-shipped fp16 proof) or 3 (both)"},
    {"raycast_early_out", nullptr, 0, 1, 1, 0, 0, KNOB_SET(knobs.early_out, (uint32_t)v), 0, "0 or 1"},
    // (what an observation means changes with these two: rover_calculate_metrics wants a fresh rover_get_observations)
    {"ray_precision", nullptr, 0, 2, 1, 0, 0, KNOB_SET(precision, (int)v), KNOB_REPLAN | KNOB_RAYS_OBS, "0 (fp32), 1 (fp16 sources) or 2 (as shipped)"},
    {"cell_index_mode", nullptr, 0, 1, 1, 0, 0, KNOB_SET(cell_rcp, (int32_t)v), KNOB_RAYS_OBS, "0 (cpu_div) or 1 (cuda_rcp)"},
    {"occlusion_route", nullptr, 0, 1, 1, 0, 0, KNOB_SET(occlusion_route, (int32_t)v), 0,      // read at every call: no table depends on it
     "0 (plain march) or 1 (ordered columns and the tile-max table)"},
};
#undef KNOB_SET

static const KnobRow* knob_by_option(const char* name) {
    for (const KnobRow& k : kKnobs)
        if (k.option && !strcmp(k.option, name)) return &k;
    return nullptr;
}
static bool knob_option_accepts(const KnobRow& k, double v) {
    return (v >= k.opt_lo && v <= k.opt_hi) || ((k.flags & KNOB_OPT_ALSO_ZERO) && v == 0);
}

static void plan_to_c(const StepPlan& p, rover_raycast_plan* out) {
    out->variant = p.variant; out->proof = p.proof; out->sorted = p.sorted ? 1 : 0; out->env_order = p.env_order ? 1 : 0;
    out->rocks_staged = p.rocks_staged ? 1 : 0; out->run = (int32_t)p.run; out->env_run = (int32_t)p.env_run;
    out->lazy_far = p.lazy_far ? 1 : 0; out->skip_clear = p.skip_clear ? 1 : 0;
    out->cull_launches = (int32_t)p.cull_launches; out->low_bits = (int32_t)p.low_bits;
    out->sort_entry_dwords = (int32_t)p.sort_entry_dwords; out->hist_fused = p.hist_fused ? 1 : 0;
}

extern "C" {

#ifndef ROVER_SRC_HASH
#define ROVER_SRC_HASH "unknown"
#endif
const char* rover_version(void) { return "rover_step 0.3 (gfx950) src-" ROVER_SRC_HASH; }

const char* rover_last_error(const rover_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int rover_create(const rover_cfg* cfg, rover_ctx** out) {
    if (!cfg || !out) return fail(nullptr, ROVER_E_INVALID, "rover_create: null argument");
    if (cfg->num_envs <= 0) return fail(nullptr, ROVER_E_INVALID, "rover_create: num_envs must be > 0 (got %d)", cfg->num_envs);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, ROVER_E_HIP, "rover_create: no HIP device available (%s)", hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, ROVER_E_INVALID, "rover_create: device %d out of range (have %d)", cfg->device, ndev);
    rover_ctx* c = new (std::nothrow) rover_ctx();
    if (!c) return fail(nullptr, ROVER_E_NOMEM, "rover_create: out of host memory");
    c->cfg = *cfg;
    if (c->cfg.num_envs_global <= 0) c->cfg.num_envs_global = c->cfg.num_envs;
    if (c->cfg.max_episode_length <= 0) c->cfg.max_episode_length = 3000;
    for (const KnobRow& k : kKnobs) {
        const char* text = k.env ? getenv(k.env) : nullptr;
        if (!text) continue;
        double v = (k.flags & KNOB_REAL) ? atof(text) : (double)atol(text);
        if (v < k.env_lo || v > k.env_hi) continue;
        if (k.flags & KNOB_ENV_AS_BOOL) v = v != 0 ? 1 : 0;
        k.set(c, v);
    }
    (void)replan(c);                 // (no maps, no distribution yet: nothing to size)
    DeviceGuard guard(cfg->device);
    e = guard.err;
    if (e == hipSuccess) e = c->d_block_cnt.alloc((size_t)cfg->num_envs / 256 + 2);
    if (e == hipSuccess) e = c->d_goal_work.alloc(2 * (size_t)cfg->num_envs);
    if (e == hipSuccess) e = c->d_ids_work.alloc((size_t)cfg->num_envs);
    if (e == hipSuccess) e = c->learn.gae_partials.alloc(3 * (size_t)GAE_MAX_BLOCKS);
    if (e == hipSuccess) e = c->learn.ppo_partials.alloc((3 + (size_t)GAUSS_MAX_A) * PPO_MAX_BLOCKS);
    if (e != hipSuccess) { delete c; return fail(nullptr, ROVER_E_HIP, "rover_create: %s", hipGetErrorString(e)); }
    *out = c;
    return ROVER_OK;
}

void rover_destroy(rover_ctx* c) {
    if (!c) return;
    DeviceGuard guard(c->cfg.device);         // the owners free their device memory on the ctx's device
    for (auto& e : c->ev0) (void)hipEventDestroy(e);
    for (auto& e : c->ev1) (void)hipEventDestroy(e);
    delete c;
}

int rover_set_knn_map(rover_ctx* c, int which, const int32_t* map_idx, int32_t X, int32_t Y, int32_t K, const int32_t* tris,
                      int32_t T, const uint16_t* verts, int32_t V, float cell, float shift_x, float shift_y) {
    if (!c) return ROVER_E_INVALID;
    if (which != ROVER_MAP_TERRAIN && which != ROVER_MAP_ROCKS) return fail(c, ROVER_E_INVALID, "set_knn_map: which=%d", which);
    if (!map_idx || !tris || !verts) return fail(c, ROVER_E_INVALID, "set_knn_map: null table pointer");
    if (X <= 0 || Y <= 0 || K <= 0 || T <= 0 || V <= 0 || !(cell > 0.0f))
        return fail(c, ROVER_E_INVALID, "set_knn_map: bad shape X=%d Y=%d K=%d T=%d V=%d cell=%g", X, Y, K, T, V, (double)cell);
    if ((uint64_t)X * (uint64_t)Y > 0xffffffffull) return fail(c, ROVER_E_INVALID, "set_knn_map: X*Y exceeds 2^32 cells");
    USE_DEVICE(c);
    MapTables m;
    if (int r = build_map_tables(c, m, which, map_idx, X, Y, K, tris, T, verts, V, cell, shift_x, shift_y)) return r;      // (the previous map stays)
    c->maps[which] = std::move(m);
    c->rays_valid = false;
    return replan(c, REALLOC_BINS);
}

int rover_set_distribution(rover_ctx* c, const double* pts, int32_t P, const int64_t* sparse_idx, int32_t Ns,
                           const int64_t* dense_idx, int32_t Nd) {
    if (!c) return ROVER_E_INVALID;
    if (!pts || P <= 0 || Ns < 0 || Nd < 0 || (Ns > 0 && !sparse_idx) || (Nd > 0 && !dense_idx))
        return fail(c, ROVER_E_INVALID, "set_distribution: bad arguments (P=%d Ns=%d Nd=%d)", P, Ns, Nd);
    USE_DEVICE(c);
    std::vector<double> hp((size_t)P * 3);
    std::vector<int64_t> hs((size_t)Ns), hd((size_t)Nd);
    HIP_TRY(c, hipMemcpy(hp.data(), pts, hp.size() * sizeof(double), hipMemcpyDefault));
    if (Ns) HIP_TRY(c, hipMemcpy(hs.data(), sparse_idx, hs.size() * sizeof(int64_t), hipMemcpyDefault));
    if (Nd) HIP_TRY(c, hipMemcpy(hd.data(), dense_idx, hd.size() * sizeof(int64_t), hipMemcpyDefault));
    std::vector<int32_t> idx;
    idx.reserve((size_t)Ns + Nd);
    for (int64_t v : hs) idx.push_back((int32_t)v);
    for (int64_t v : hd) idx.push_back((int32_t)v);
    for (int32_t v : idx)
        if (v < 0 || v >= P) return fail(c, ROVER_E_INVALID, "set_distribution: index %d outside [0,%d)", v, P);
    c->have_dist = false;
    ++c->dist_gen;
    c->d_dist.reset(); c->d_obs_idx.reset();
    const int r = [&]() -> int {
        HIP_TRY(c, c->d_dist.alloc(hp.size()));
        HIP_TRY(c, hipMemcpy(c->d_dist.get(), hp.data(), c->d_dist.bytes(), hipMemcpyHostToDevice));
        HIP_TRY(c, c->d_obs_idx.alloc(idx.size() + 1));
        HIP_TRY(c, hipMemset(c->d_obs_idx.get(), 0, c->d_obs_idx.bytes()));      // assemble_obs_kernel reads entry 0 from every lane
        if (!idx.empty()) HIP_TRY(c, hipMemcpy(c->d_obs_idx.get(), idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        c->P = P; c->Ns = Ns; c->Nd = Nd;
        c->have_dist = true;
        return ROVER_OK;
    }();
    return replan(c, REALLOC_WORKSPACE, r);         // (a failure half way leaves no distribution: the plan says so too)
}

int rover_set_heightfield(rover_ctx* c, const float* hm, int32_t N0, int32_t N1, float hscale, float vscale, float sx, float sy) {
    if (!c) return ROVER_E_INVALID;
    if (!hm || N0 <= 0 || N1 <= 0 || !(hscale > 0.0f)) return fail(c, ROVER_E_INVALID, "set_heightfield: bad arguments");
    USE_DEVICE(c);
    DevBuf<float> d;
    HIP_TRY(c, d.alloc((uint64_t)N0 * N1));
    HIP_TRY(c, hipMemcpy(d.get(), hm, d.bytes(), hipMemcpyDefault));       // (the previous heightfield stays in place)
    c->d_hm = std::move(d);
    ++c->hf_gen;
    c->hf = HeightDev{c->d_hm.get(), N0, N1, hscale, vscale, sx, sy, 1.0f / hscale, c->cell_rcp};
    c->have_hf = true;
    return ROVER_OK;
}

int rover_set_stones(rover_ctx* c, const float* info7, int32_t S) {
    if (!c) return ROVER_E_INVALID;
    if (S < 0 || (S > 0 && !info7)) return fail(c, ROVER_E_INVALID, "set_stones: bad arguments");
    USE_DEVICE(c);
    std::vector<float> h((size_t)S * 7);
    if (S) HIP_TRY(c, hipMemcpy(h.data(), info7, h.size() * sizeof(float), hipMemcpyDefault));
    // stone-occupancy grid: 2 m cells over the stones' bounding box padded by r_max + 1.4 m (the largest threshold the
    // task uses, rover.py:660) + margin; a cell lists the stones whose inflated disc reaches it.
    const float cell = 2.0f, reach = 1.4f + 0.05f;
    float x0 = 0.f, y0 = 0.f, x1 = 1.f, y1 = 1.f, rmax = 0.f;
    bool any = false, poisoned = false;
    for (int s = 0; s < S; ++s) {
        float x = h[7 * s], y = h[7 * s + 1], r = h[7 * s + 6];
        // torch.min propagates NaN (rover.py:538): one NaN stone makes nearest_rock NaN for every query, and
        // NaN <= thr is False -> nothing ever collides.  Reproduced by leaving every cell list empty.
        if (!(x == x) || !(y == y) || !(r == r)) { poisoned = true; continue; }
        if (!any) { x0 = x1 = x; y0 = y1 = y; any = true; }
        x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1; y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
        rmax = r > rmax ? r : rmax;
    }
    const float pad = rmax + reach;
    x0 -= pad; y0 -= pad; x1 += pad; y1 += pad;
    int nx = (int)((x1 - x0) / cell) + 1, ny = (int)((y1 - y0) / cell) + 1;
    if (nx < 1) nx = 1; if (ny < 1) ny = 1;
    if ((int64_t)nx * ny > (int64_t)1 << 24) return fail(c, ROVER_E_INVALID, "set_stones: stone extent too large for the 2 m grid");
    std::vector<std::vector<uint32_t>> lists((size_t)nx * ny);
    for (int s = 0; s < S && any && !poisoned; ++s) {
        float x = h[7 * s], y = h[7 * s + 1], r = h[7 * s + 6];
        if (!(x == x) || !(y == y) || !(r == r)) continue;
        float rr = r + reach;
        int cx0 = (int)((x - rr - x0) / cell), cx1 = (int)((x + rr - x0) / cell);
        int cy0 = (int)((y - rr - y0) / cell), cy1 = (int)((y + rr - y0) / cell);
        cx0 = cx0 < 0 ? 0 : cx0; cy0 = cy0 < 0 ? 0 : cy0; cx1 = cx1 >= nx ? nx - 1 : cx1; cy1 = cy1 >= ny ? ny - 1 : cy1;
        for (int cx = cx0; cx <= cx1; ++cx)
            for (int cy = cy0; cy <= cy1; ++cy) lists[(size_t)cx * ny + cy].push_back((uint32_t)s);   // stone order kept
    }
    std::vector<uint32_t> start((size_t)nx * ny + 1, 0), idx;
    for (size_t k = 0; k < lists.size(); ++k) { start[k + 1] = start[k] + (uint32_t)lists[k].size(); idx.insert(idx.end(), lists[k].begin(), lists[k].end()); }
    std::vector<float4> xyr(idx.size() + 1);
    for (size_t k = 0; k < idx.size(); ++k) {
        const uint32_t sidx = idx[k];
        float fid; memcpy(&fid, &sidx, sizeof fid);
        xyr[k] = float4{h[7 * (size_t)sidx], h[7 * (size_t)sidx + 1], h[7 * (size_t)sidx + 6], fid};
    }
    DevBuf<uint32_t> d_start;
    DevBuf<float4> d_xyr;
    DevBuf<float> d_info;
    hipError_t e;
    if ((e = d_start.alloc(start.size())) != hipSuccess || (e = d_xyr.alloc(xyr.size())) != hipSuccess ||
        (e = d_info.alloc((uint64_t)S * 7 + 1)) != hipSuccess ||
        (e = hipMemcpy(d_start.get(), start.data(), d_start.bytes(), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(d_xyr.get(), xyr.data(), d_xyr.bytes(), hipMemcpyHostToDevice)) != hipSuccess ||
        (S && (e = hipMemcpy(d_info.get(), h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess))
        return fail(c, ROVER_E_HIP, "set_stones: %s", hipGetErrorString(e));        // the previous stone tables stay in place
    c->d_stones = std::move(d_info); c->d_grid_start = std::move(d_start); c->d_grid_xyr = std::move(d_xyr);
    c->sgrid = StoneGridDev{c->d_grid_start.get(), c->d_grid_xyr.get(), x0, y0, 1.0f / cell, nx, ny};
    c->S = S;
    c->have_stones = true;
    return ROVER_OK;
}

int rover_set_curriculum_level(rover_ctx* c, int32_t level) {
    if (!c) return ROVER_E_INVALID;
    c->cfg.curriculum_level = level;
    return ROVER_OK;
}

// ---- step ------------------------------------------------------------------------------------------
static int check_precision(rover_ctx* c) {
    if (c->precision == 2 && c->plan.variant < 2)
        return fail(c, ROVER_E_STATE, "ray_precision 2 (as shipped, fp16 maths) needs ray-cast variant 2 or 3 (K <= 256 on both maps)");
    // a variant asked for by name is the one that runs, or the call fails: the staged kernel needs the tables of the arithmetic in force
    if (c->knobs.variant == 4 && staged_tables_missing(plan_inputs(c)))
        return fail(c, ROVER_E_STATE, "raycast_variant 4 (staged) was requested but its tables for ray_precision %d are not there (option "
                                      "staged_tables, or they did not fit when the maps were set)", c->precision);
    return ROVER_OK;
}

static int check_ready(rover_ctx* c) {
    if (!have_maps(c)) return fail(c, ROVER_E_STATE, "terrain and rocks maps must be set (rover_set_knn_map)");
    if (!c->have_dist) return fail(c, ROVER_E_STATE, "ray distribution must be set (rover_set_distribution)");
    if (!c->ws_ok || !c->bins_ok) return fail(c, ROVER_E_STATE, "the step workspace is not allocated (an earlier rover_set_* call failed)");
    return check_precision(c);
}

static CullArgs cull_args(const rover_ctx* c, const StepPlan& p, uint32_t n_valid) {
    CullArgs a{};
    a.rays = c->d_rays.get(); a.sorted = c->d_sorted.get(); a.n_sorted = n_valid;
    a.n_terrain = (uint32_t)c->cfg.num_envs * (uint32_t)c->P;
    const MapTables &m0 = c->maps[0], &m1 = c->maps[1];
    const int k = p.proof;                // the as-shipped fp16 arithmetic: its own proof tables, the fp16 exact phase
    a.idx0 = m0.cull_idx.get(); a.idx1 = m1.cull_idx.get();
    a.ctab0 = m0.proof[k].ctab.get(); a.ctab1 = m1.proof[k].ctab.get();
    a.rtab0 = m0.rtab.get(); a.rtab1 = m1.rtab.get();
    a.half = k;
    const CullProofH ph = cull_proof_h(c->knobs.cull_eta_h, c->knobs.cull_split_h);
    a.c_a_h = ph.c_a; a.tau2_h = ph.tau2;
    a.far0 = m0.proof[k].far.get(); a.far1 = m1.proof[k].far.get();
    a.near0 = a.far0 + 2ull * (uint64_t)m0.cells; a.near1 = a.far1 + 2ull * (uint64_t)m1.cells;
    a.k2_far = cull_far_k2(a.half, ph);
    a.lazy_far = p.lazy_far ? 1 : 0;
    a.skip_clear = p.skip_clear ? 1 : 0;
    a.kp0 = (uint32_t)c->maps[0].knn.K8; a.kp1 = (uint32_t)c->maps[1].knn.K8;
    a.run = p.run;
    a.out = c->d_dist_out.get();
    a.queue = c->queue.entries.get();
    a.stats = c->queue.stats.get();
    a.queue_entries = p.queue_entries;          // (check_queue: the queue was sized for p)
    return a;
}

// the culled / staged ray cast's candidate queue and counters were sized for plan p (replan; never in a step: no hipMalloc inside a stream capture)
static int check_queue(rover_ctx* c, const StepPlan& p) {
    const CullQueue& q = c->queue;
    if (p.variant >= 3 && (!q.entries.get() || !q.stats.get() || q.sized_for != p))
        return fail(c, ROVER_E_STATE, "the culled ray cast's candidate queue is not allocated for the options in force");
    return ROVER_OK;
}

// the ray-cast launch(es) of plan p, on the ray records / sorted list in the workspace
static int run_raycast(rover_ctx* c, const StepPlan& p, uint32_t n_valid, hipStream_t s) {
    const uint32_t E = (uint32_t)c->cfg.num_envs;
    CullQueue& q = c->queue;
    if (p.variant >= 3 && q.stats.get() && p != q.counters_written_under) {
        // the per-wave counters of rover_get_cull_info: a launch writes the slots of its own waves; when the way the rays are cast changed
        // since the last launch (another kernel, order or run length: another number of waves) the slots are cleared first
        HIP_TRY(c, hipMemsetAsync(q.stats.get(), 0, q.stats.bytes(), s));
        q.counters_written_under = p;
    }
    if (p.variant == 4) {
        LaneArgs l{};
        l.rays = c->d_rays.get(); l.sorted = c->d_sorted.get(); l.n_sorted = n_valid; l.n_terrain = E * (uint32_t)c->P;
        for (int w = 0; w < 2; ++w) {
            const LaneTables t = c->maps[w].proof[p.proof].view();
            l.lvl[w] = t.lvl; l.lrec[w] = t.lrec; l.lid[w] = t.lid; l.rtab[w] = c->maps[w].rtab.get(); l.pp[w] = c->maps[w].lane_pp;
        }
        {
            const CullProofH ph = cull_proof_h(c->knobs.cull_eta_h, c->knobs.cull_split_h);
            l.half = p.proof; l.c_a_h = ph.c_a; l.k2_far = cull_far_k2(l.half, ph);
            l.forms = p.proof ? 0u : (c->maps[0].lane_box ? 1u : 0u) | (c->maps[1].lane_box ? 2u : 0u);
            for (int w = 0; w < 2; ++w) { l.forms |= c->maps[w].lane_pair_rows ? 4u << w : 0u; l.y[w] = (uint32_t)c->maps[w].knn.Y; }
            l.forms |= c->lane_rebase ? 16u : 0u;
        }
        l.run = p.run; l.out = c->d_dist_out.get(); l.stats = q.stats.get();
        if (p.env_order) {      // every slot (padding included), in env order, one launch
            l.sorted = nullptr; l.n_sorted = E * p.R8; l.n_terrain = l.n_sorted; l.run = p.env_run;
            HIP_TRY(c, launch_raycast_lane(l, s));
            return ROVER_OK;
        }
        if (p.rocks_staged) {
            HIP_TRY(c, launch_raycast_lane(l, s));
        } else {
            // the terrain rays (the first E x P of the sorted list: terrain bins sort first) through the staged kernel, the rock rays — few per
            // bin, a tenth of them off every cone (the horizontal body rays) — through the culled one, which reads 800 bytes of ids per bin
            // where the staged kernel reads the 3.5 KB of a cell's whole row for one such ray
            CullArgs a = cull_args(c, p, n_valid);
            l.n_sorted = l.n_terrain < n_valid ? l.n_terrain : n_valid;
            a.sorted += l.n_sorted; a.n_sorted -= l.n_sorted; a.n_terrain = 0;
            a.stats += lane_waves(l.n_sorted, l.run);
            // (the two launches touch disjoint rays, results and counters; side by side on a second stream they measured slower: 125 against
            //  127 M env-steps/s)
            HIP_TRY(c, launch_raycast_lane(l, s));
            if (a.n_sorted) HIP_TRY(c, launch_raycast_culled(a, s));
        }
    } else if (p.variant == 3)
        HIP_TRY(c, launch_raycast_culled(cull_args(c, p, n_valid), s));
    else if (p.variant == 2)
        HIP_TRY(c, launch_raycast_binned(c->d_rays.get(), c->d_sorted.get(), n_valid, c->maps[0].knn.table, c->maps[1].knn.table,
                                         (uint32_t)c->maps[0].knn.K8, (uint32_t)c->maps[1].knn.K8, p.run, p.proof != 0, c->knobs.early_out, c->d_dist_out.get(), s));
    else
        HIP_TRY(c, launch_raycast(c->d_rays.get(), E * p.R8, c->maps[0].knn.table, c->maps[1].knn.table, (uint32_t)c->maps[0].knn.K8,
                                  (uint32_t)c->maps[1].knn.K8, c->d_dist_out.get(), s));
    return ROVER_OK;
}

// The ray pipeline of a step: env records + ray records, the bucket sort by (map, cell), the ray cast -> d_dist_out [E][R8].
// euler_in != NULL (rover_get_depths): the poses come as euler angles, quat / joints / target may be NULL, and the ctx's euler / heading
// state of the last observation is left alone.
static int cast_rays(rover_ctx* c, const float* pos, const float* quat, const float* joints, const float* target, const float* euler_in,
                     hipStream_t s, const float* import_src = nullptr, const float* import_dir = nullptr) {
    const uint32_t E = (uint32_t)c->cfg.num_envs;
    PrepArgs p{};
    const StepPlan& plan = c->plan;
    p.E = E; p.P = (uint32_t)c->P; p.R8 = plan.R8;
    p.pos = pos; p.quat = quat; p.joints = joints; p.target = target; p.euler_in = euler_in;
    p.dist = c->d_dist.get(); p.terrain = c->maps[0].knn; p.rocks = c->maps[1].knn;
    p.rays = c->d_rays.get(); p.euler = euler_in ? nullptr : c->d_euler.get(); p.heading = euler_in ? nullptr : c->d_heading.get();
    if (int r = check_queue(c, plan)) return r;
    const uint32_t n_valid = E * (26u + (uint32_t)c->P);
    p.rocks_bin_offset = (uint32_t)((uint64_t)c->maps[0].knn.X * c->maps[0].knn.Y);
    const bool sorts = plan.sorted;
    if (sorts) p.bin_out = c->d_bins.get();
    p.precision = c->precision;
    p.cell_rcp = c->cell_rcp;
    // the sort's first pass (keys per coarse bucket and tile) inside prep_rays_kernel where a 64-env block's keys lie in one tile: the
    // table is zero between steps (allocation, then the sort's last kernel) — unless a step failed half way
    // (caller-supplied rays, rover_cast_rays: import_rays_kernel writes the records and keys, the sort counts its keys itself)
    const bool hist_fused = !import_src && plan.hist_fused;
    if (hist_fused) {
        if (c->bkt_table_dirty) HIP_TRY(c, hipMemsetAsync(c->d_bkt_table.get(), 0, c->d_bkt_table.bytes(), s));
        c->bkt_table_dirty = true;
        p.hist = c->d_bkt_table.get(); p.hist_low_bits = plan.low_bits; p.hist_buckets = bucket_count(plan); p.hist_blocks_per_tile = plan.hist_blocks_per_tile;
    }
    if (import_src) {
        // caller-supplied directions: the culled / staged ray cast's proofs need them of unit length (what -normalize() gives)
        uint32_t* const not_unit = plan.variant >= 3 ? c->d_block_cnt.get() + (size_t)c->cfg.num_envs / 256 + 1 : nullptr;      // (the spare word behind the block counts)
        if (not_unit) HIP_TRY(c, hipMemsetAsync(not_unit, 0, sizeof(uint32_t), s));
        HIP_TRY(c, launch_import_rays(import_src, import_dir, E, plan.R8, (uint32_t)c->P, c->maps[0].knn, c->maps[1].knn, p.rocks_bin_offset, c->precision,
                                      c->cell_rcp, c->d_rays.get(), sorts ? c->d_bins.get() : nullptr, s, not_unit));
        if (not_unit) {
            uint32_t bad = 0;
            HIP_TRY(c, hipMemcpyAsync(&bad, not_unit, sizeof bad, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            if (bad) {
                c->rays_valid = false;
                return fail(c, ROVER_E_INVALID, "cast_rays: %u directions are not of unit length (|d|^2 within %g of 1: pass -normalize(direction) as "
                            "rover_export_rays returns it, or use raycast_variant 1 / 2, which evaluate every triangle)", bad, c->precision == 2 ? 4.0e-3 : 1.0e-5);
            }
        }
    } else {
        HIP_TRY(c, launch_prep(p, s));
    }
    if (sorts)
        HIP_TRY(c, launch_bin_rays(c->d_bins.get(), E * plan.R8, n_valid, (uint32_t)plan.n_bins, plan.low_bits, plan.sort_entry_dwords == 1,
                                   c->d_bkt_table.get(), c->d_pairs.get(), c->d_block_sums.get(), c->d_sorted.get(), hist_fused, s));
    // fused histogram: bucket_sort_kernel has cleared the table again; otherwise the table (if the sort ran) holds this step's offsets
    if (sorts) c->bkt_table_dirty = !hist_fused;        // (variant 1 does not touch the table)
    const bool timed = c->profiling && (c->prof_seen++ % c->prof_every) == 0;
    if (timed) {
        if (c->prof_pending == kProfRing && prof_drain(c)) return fail(c, ROVER_E_HIP, "profiling: event drain failed");
        HIP_TRY(c, hipEventRecord(c->ev0[c->prof_pending], s));
    }
    if (int r = run_raycast(c, plan, n_valid, s)) return r;
    if (timed) {
        HIP_TRY(c, hipEventRecord(c->ev1[c->prof_pending], s));
        ++c->prof_pending;
        ++c->prof_launches;
    }
    c->ws_plan = plan;
    c->rays_valid = true;
    return ROVER_OK;
}

// launch_obs false (rover_step): the obs pass is left to the caller, which hands *obs_args to do_metrics — one grid for both passes
static int do_observations(rover_ctx* c, const rover_step_in* in, const rover_step_out* out, hipStream_t s, bool launch_obs, ObsArgs* obs_args) {
    if (!in->pos || !in->quat || !in->joints || !in->target || !in->lin_hist || !in->ang_hist)
        return fail(c, ROVER_E_INVALID, "get_observations: null input pointer");
    if (!out->obs) return fail(c, ROVER_E_INVALID, "get_observations: obs is required");
    const uint32_t E = (uint32_t)c->cfg.num_envs, W = (uint32_t)(4 + c->Ns + c->Nd);
    const int64_t stride = out->obs_stride ? out->obs_stride : (int64_t)W;
    if (stride < (int64_t)W) return fail(c, ROVER_E_INVALID, "obs_stride %lld < row width %u", (long long)stride, W);
    if (int r = cast_rays(c, in->pos, in->quat, in->joints, in->target, nullptr, s)) return r;
    c->obs_valid = true;
    ObsArgs o{};
    o.E = E; o.W = W; o.R8 = c->plan.R8; o.obs_stride = stride;
    o.pos = in->pos; o.target = in->target; o.heading = c->d_heading.get(); o.lin_hist = in->lin_hist; o.ang_hist = in->ang_hist;
    o.dist = c->d_dist_out.get(); o.obs_idx = c->d_obs_idx.get(); o.obs = out->obs; o.fp16_div = c->precision == 2;
    if (launch_obs) HIP_TRY(c, launch_assemble_obs(o, s));
    *obs_args = o;
    if (out->ray_dist || out->wheel_dist || out->body_dist || out->ray_src || out->hit_pt)
        HIP_TRY(c, launch_export_dist(c->d_dist_out.get(), c->d_rays.get(), E, c->plan.R8, (uint32_t)c->P, c->precision, out->ray_dist, out->wheel_dist,
                                      out->body_dist, out->ray_src, out->hit_pt, s));
    if (out->euler) HIP_TRY(c, hipMemcpyAsync(out->euler, c->d_euler.get(), (uint64_t)E * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (out->heading_diff) HIP_TRY(c, hipMemcpyAsync(out->heading_diff, c->d_heading.get(), (uint64_t)E * sizeof(float), hipMemcpyDeviceToDevice, s));
    return ROVER_OK;
}

// with_obs != NULL: the obs pass of a do_observations(launch_obs = false) runs in the same launch
static int do_metrics(rover_ctx* c, const rover_step_in* in, const rover_step_out* out, int inc, int coll, int met, int done,
                      hipStream_t s, bool count_done = false, const ObsArgs* with_obs = nullptr) {
    if (!in->pos || !in->target) return fail(c, ROVER_E_INVALID, "metrics/done: null input pointer");
    if ((inc || met || done) && !in->progress) return fail(c, ROVER_E_INVALID, "metrics/done: progress is required");
    if (!out->rock_collision) return fail(c, ROVER_E_INVALID, "metrics/done: rock_collision is required");
    if (met && (!in->joints || !in->lin_hist || !in->ang_hist || !out->rew))
        return fail(c, ROVER_E_INVALID, "calculate_metrics: joints, lin_hist, ang_hist and rew are required");
    if (done && (!in->euler_pre || !out->reset)) return fail(c, ROVER_E_INVALID, "is_done: euler_pre and reset are required");
    if (coll && out->stone_collision) {
        if (!c->have_stones) return fail(c, ROVER_E_STATE, "stone_collision: rover_set_stones first");
        if (!(out->stone_margin <= 1.4f)) return fail(c, ROVER_E_INVALID, "stone_margin %g exceeds the 1.4 m reach of the stone grid", (double)out->stone_margin);
    }
    MetricsArgs m{};
    m.E = (uint32_t)c->cfg.num_envs; m.R8 = c->plan.R8;
    m.curriculum_level = c->cfg.curriculum_level; m.max_episode_length = c->cfg.max_episode_length;
    m.num_envs_global = c->cfg.num_envs_global;
    m.do_increment = inc; m.do_collision = coll; m.do_metrics = met; m.do_done = done;
    m.pos_reward = c->cfg.pos_reward; m.heading_contraint_reward = c->cfg.heading_contraint_reward;
    m.motion_contraint_reward = c->cfg.motion_contraint_reward; m.goal_angle_reward = c->cfg.goal_angle_reward;
    m.boogie_contraint_reward = c->cfg.boogie_contraint_reward;
    m.wheel_thr = c->precision == 2 ? 0.7998046875f : 0.8f;                // fp16(0.8), fp16(0.45): Python scalars compared
    m.body_thr = c->precision == 2 ? 0.449951171875f : 0.45f;              // against fp16 tensors (rover.py:667-668)
    m.pos = in->pos; m.target = in->target; m.joints = in->joints; m.lin_hist = in->lin_hist; m.ang_hist = in->ang_hist;
    m.euler_pre = in->euler_pre; m.heading = c->d_heading.get(); m.dist = c->d_dist_out.get();
    m.progress = in->progress; m.rock_collision = out->rock_collision; m.rew = out->rew; m.reset = out->reset;
    m.ex_pos_reward = out->ex_pos_reward; m.ex_collision = out->ex_collision_penalty; m.ex_upright = out->ex_uprightness_penalty;
    m.ex_heading = out->ex_heading_contraint_penalty; m.ex_motion = out->ex_motion_contraint_penalty;
    m.block_cnt = count_done ? c->d_block_cnt.get() : nullptr;
    m.stone_collision = coll ? out->stone_collision : nullptr; m.stone_margin = out->stone_margin;
    m.done_u8 = done ? out->done_u8 : nullptr;
    m.sgrid = c->sgrid; m.info7 = c->d_stones.get();
    m.ex_goal_angle = out->ex_goal_angle_penalty; m.ex_lin = out->ex_torque_penalty_driving; m.ex_ang = out->ex_torque_penalty_steering;
    // the evaluation latch: check_collision's update (rover.py:670-672, level >= 2 only) and is_done's (:620-631); never metrics alone
    if (c->eval_on && ((coll && c->cfg.curriculum_level >= 2) || done)) {
        if (!in->progress) return fail(c, ROVER_E_INVALID, "evaluation: progress is required (the latch records it)");
        m.eval_res = c->d_eval_res.get(); m.eval_step = c->d_eval_step.get();
    }
    if (with_obs) HIP_TRY(c, launch_obs_metrics(*with_obs, m, s));
    else HIP_TRY(c, launch_metrics_done(m, s));
    return ROVER_OK;
}

int rover_get_observations(rover_ctx* c, const rover_step_in* in, const rover_step_out* out, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!in || !out) return fail(c, ROVER_E_INVALID, "get_observations: null struct");
    if (int r = check_ready(c)) return r;
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    ObsArgs o{};
    if (int r = do_observations(c, in, out, s, true, &o)) return r;
    if (!out->rock_collision) return ROVER_OK;
    // check_collision (rover.py:292-293) is part of get_observations: run only the collision stage
    return do_metrics(c, in, out, 0, 1, 0, 0, s);
}

int rover_calculate_metrics(rover_ctx* c, const rover_step_in* in, const rover_step_out* out, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!in || !out) return fail(c, ROVER_E_INVALID, "calculate_metrics: null struct");
    if (int r = check_ready(c)) return r;
    if (!c->obs_valid) return fail(c, ROVER_E_STATE, "calculate_metrics: call rover_get_observations first (rover.py:479 reads self.heading_diff)");
    USE_DEVICE(c);
    return do_metrics(c, in, out, 0, 0, 1, 0, (hipStream_t)stream);
}

int rover_is_done(rover_ctx* c, const rover_step_in* in, const rover_step_out* out, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!in || !out) return fail(c, ROVER_E_INVALID, "is_done: null struct");
    if (int r = check_ready(c)) return r;
    USE_DEVICE(c);
    return do_metrics(c, in, out, 0, 0, 0, 1, (hipStream_t)stream);
}

int rover_get_depths(rover_ctx* c, const float* positions, const float* rotations_euler, float* distances, float* points,
                     float* sources, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!positions || !rotations_euler) return fail(c, ROVER_E_INVALID, "get_depths: positions and rotations are required");
    if (int r = check_ready(c)) return r;
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (int r = cast_rays(c, positions, nullptr, nullptr, nullptr, rotations_euler, s)) return r;
    if (distances || points || sources)
        HIP_TRY(c, launch_export_dist(c->d_dist_out.get(), c->d_rays.get(), (uint32_t)c->cfg.num_envs, c->plan.R8, (uint32_t)c->P, c->precision, distances,
                                      nullptr, nullptr, sources, points, s));
    return ROVER_OK;
}

int rover_get_collisions(rover_ctx* c, const float* positions, const float* rotations_euler, const float* joints, float* wheel_dist,
                         float* body_dist, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!positions || !rotations_euler) return fail(c, ROVER_E_INVALID, "get_collisions: positions and rotations are required");
    if (int r = check_ready(c)) return r;
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (int r = cast_rays(c, positions, nullptr, joints, nullptr, rotations_euler, s)) return r;
    if (wheel_dist || body_dist)
        HIP_TRY(c, launch_export_dist(c->d_dist_out.get(), c->d_rays.get(), (uint32_t)c->cfg.num_envs, c->plan.R8, (uint32_t)c->P, c->precision, nullptr,
                                      wheel_dist, body_dist, nullptr, nullptr, s));
    return ROVER_OK;
}

int rover_export_rays(rover_ctx* c, float* src, float* dir, int32_t* cell, float* dist, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (int r = check_ready(c)) return r;
    if (!c->rays_valid) return fail(c, ROVER_E_STATE, "export_rays: no ray records yet (run a step first)");
    USE_DEVICE(c);
    HIP_TRY(c, launch_export_rays(c->d_rays.get(), c->d_dist_out.get(), (uint32_t)c->cfg.num_envs, c->plan.R8, (uint32_t)c->P, src, dir, cell, dist,
                                  (hipStream_t)stream));
    return ROVER_OK;
}

int rover_cast_rays(rover_ctx* c, const float* src, const float* dir, float* dist, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!src || !dir || !dist) return fail(c, ROVER_E_INVALID, "cast_rays: src, dir and dist are required");
    if (int r = check_ready(c)) return r;
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (int r = cast_rays(c, nullptr, nullptr, nullptr, nullptr, nullptr, s, src, dir)) return r;
    HIP_TRY(c, launch_export_rays(c->d_rays.get(), c->d_dist_out.get(), (uint32_t)c->cfg.num_envs, c->plan.R8, (uint32_t)c->P, nullptr, nullptr, nullptr, dist, s));
    return ROVER_OK;
}

int rover_compact_resets(rover_ctx* c, const int64_t* reset, int64_t* ids, int32_t* n_reset, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!reset || !ids || !n_reset) return fail(c, ROVER_E_INVALID, "compact_resets: null pointer");
    USE_DEVICE(c);
    HIP_TRY(c, launch_compact(reset, (uint32_t)c->cfg.num_envs, (int64_t)c->cfg.env_offset, c->d_block_cnt.get(), false, ids, n_reset,
                              (hipStream_t)stream));
    return ROVER_OK;
}

int rover_step(rover_ctx* c, const rover_step_in* in, const rover_step_out* out, uint32_t flags, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!in || !out) return fail(c, ROVER_E_INVALID, "step: null struct");
    if (int r = check_ready(c)) return r;
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if ((flags & ROVER_STEP_COMPACT) && (!out->reset_ids || !out->n_reset))
        return fail(c, ROVER_E_INVALID, "step: ROVER_STEP_COMPACT needs reset_ids and n_reset");
    ObsArgs o{};                      // the obs pass is launched by do_metrics, in one grid with the metrics pass
    if (int r = do_observations(c, in, out, s, false, &o)) return r;
    const bool compact = (flags & ROVER_STEP_COMPACT) != 0;
    if (int r = do_metrics(c, in, out, (flags & ROVER_STEP_INCREMENT_PROGRESS) ? 1 : 0, 1, 1, 1, s, compact, &o)) return r;
    if (compact)
        HIP_TRY(c, launch_compact(out->reset, (uint32_t)c->cfg.num_envs, (int64_t)c->cfg.env_offset, c->d_block_cnt.get(), true,
                                  out->reset_ids, out->n_reset, s));
    return ROVER_OK;
}

// ---- evaluation mode -------------------------------------------------------------------------------
int rover_set_evaluation(rover_ctx* c, int32_t enable) {
    if (!c) return ROVER_E_INVALID;
    USE_DEVICE(c);
    c->eval_on = false;
    c->d_eval_res.reset(); c->d_eval_step.reset();
    if (!enable) return ROVER_OK;
    const size_t E = (size_t)c->cfg.num_envs;
    HIP_TRY(c, c->d_eval_res.alloc(E));
    HIP_TRY(c, c->d_eval_step.alloc(E));
    HIP_TRY(c, hipMemset(c->d_eval_res.get(), 0, c->d_eval_res.bytes()));
    HIP_TRY(c, hipMemset(c->d_eval_step.get(), 0, c->d_eval_step.bytes()));
    HIP_TRY(c, hipDeviceSynchronize());
    c->eval_on = true;
    return ROVER_OK;
}

int rover_eval_clear(rover_ctx* c, const int64_t* env_ids, int32_t n, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!c->eval_on) return fail(c, ROVER_E_STATE, "eval_clear: evaluation is off (rover_set_evaluation(ctx, 1) first)");
    const int32_t E = c->cfg.num_envs;
    if (env_ids && (n < 0 || n > E)) return fail(c, ROVER_E_INVALID, "eval_clear: n = %d outside [0, %d]", n, E);
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (env_ids && n > 0) {                 // the ids are checked on the host: the call waits for the stream that wrote them
        std::vector<int64_t> h((size_t)n);
        HIP_TRY(c, hipStreamSynchronize(s));
        HIP_TRY(c, hipMemcpy(h.data(), env_ids, h.size() * sizeof(int64_t), hipMemcpyDefault));
        for (int32_t i = 0; i < n; ++i)
            if (h[i] < 0 || h[i] >= E) return fail(c, ROVER_E_INVALID, "eval_clear: env id %lld outside [0, %d)", (long long)h[i], E);
    }
    HIP_TRY(c, launch_eval_clear(c->d_eval_res.get(), c->d_eval_step.get(), (uint32_t)E, env_ids, env_ids ? (uint32_t)n : (uint32_t)E, s));
    return ROVER_OK;
}

int rover_eval_read(rover_ctx* c, int64_t* eval_res, int64_t* eval_step, int64_t* summary8, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!c->eval_on) return fail(c, ROVER_E_STATE, "eval_read: evaluation is off (rover_set_evaluation(ctx, 1) first)");
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t bytes = (uint64_t)c->cfg.num_envs * sizeof(int64_t);
    if (eval_res) HIP_TRY(c, hipMemcpyAsync(eval_res, c->d_eval_res.get(), bytes, hipMemcpyDeviceToDevice, s));
    if (eval_step) HIP_TRY(c, hipMemcpyAsync(eval_step, c->d_eval_step.get(), bytes, hipMemcpyDeviceToDevice, s));
    if (summary8) HIP_TRY(c, launch_eval_summary(c->d_eval_res.get(), c->d_eval_step.get(), (uint32_t)c->cfg.num_envs, summary8, s));
    return ROVER_OK;
}

int rover_quat_to_euler(rover_ctx* c, const float* quat, float* euler, int32_t n, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!quat || !euler || n < 0) return fail(c, ROVER_E_INVALID, "quat_to_euler: bad arguments");
    if (n == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_quat_to_euler(quat, euler, (uint32_t)n, (hipStream_t)stream));
    return ROVER_OK;
}

// ---- reset path ------------------------------------------------------------------------------------
int rover_clearance(rover_ctx* c, const float* xy, int32_t n, float* out, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!c->have_stones) return fail(c, ROVER_E_STATE, "clearance: rover_set_stones first");
    if (n < 0 || (n > 0 && (!xy || !out))) return fail(c, ROVER_E_INVALID, "clearance: bad arguments");
    if (n == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_clearance(c->d_stones.get(), (uint32_t)c->S, xy, (uint32_t)n, out, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_shift_spawns(rover_ctx* c, float* pos3, int32_t n, int32_t max_iter, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!c->have_stones) return fail(c, ROVER_E_STATE, "shift_spawns: rover_set_stones first");
    if (n < 0 || (n > 0 && !pos3) || max_iter < 0) return fail(c, ROVER_E_INVALID, "shift_spawns: bad arguments");
    if (n == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_shift_spawns(c->sgrid, c->d_stones.get(), pos3, (uint32_t)n, max_iter, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_sample_height(rover_ctx* c, const float* xy, int32_t n, float* out, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!c->have_hf) return fail(c, ROVER_E_STATE, "sample_height: rover_set_heightfield first");
    if (n < 0 || (n > 0 && (!xy || !out))) return fail(c, ROVER_E_INVALID, "sample_height: bad arguments");
    if (n == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_sample_height(c->hf, xy, (uint32_t)n, out, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_generate_goals(rover_ctx* c, const int64_t* env_ids, int32_t n, const float* initial_pos3, float* target3, float radius,
                         const float* draws, int32_t max_draws, uint64_t seed, int32_t* n_draws_used, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!c->have_stones || !c->have_hf) return fail(c, ROVER_E_STATE, "generate_goals: rover_set_stones and rover_set_heightfield first");
    if (n < 0 || n > c->cfg.num_envs || (n > 0 && (!env_ids || !initial_pos3 || !target3)) || max_draws <= 0)
        return fail(c, ROVER_E_INVALID, "generate_goals: bad arguments (n=%d, max_draws=%d)", n, max_draws);
    if (n == 0) return ROVER_OK;
    USE_DEVICE(c);
    GoalArgs g{c->d_stones.get(), (uint32_t)c->S, c->hf, c->sgrid, env_ids, 0, (uint32_t)n, nullptr, initial_pos3, target3, radius, draws,
               max_draws, seed, nullptr, (int32_t*)c->d_goal_work.get(), n_draws_used};
    HIP_TRY(c, launch_generate_goals(g, (uint32_t)n, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_reset_envs(rover_ctx* c, const rover_reset_io* io, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!io) return fail(c, ROVER_E_INVALID, "reset_envs: null struct");
    if (!io->reset_ids || !io->initial_pos3 || !io->pos3 || !io->quat4 || !io->reset || !io->progress)
        return fail(c, ROVER_E_INVALID, "reset_envs: reset_ids, initial_pos3, pos3, quat4, reset and progress are required");
    if (!io->n_reset_dev && (io->n_reset_host < 0 || io->n_reset_host > c->cfg.num_envs))
        return fail(c, ROVER_E_INVALID, "reset_envs: n_reset_host=%d out of range", io->n_reset_host);
    if (io->draws && io->n_reset_dev) return fail(c, ROVER_E_INVALID, "reset_envs: caller-supplied draws need n_reset_host");
    // yaw_deg[i] is read for every i < n: with the count on the device n can be any value up to num_envs
    if (io->yaw_deg && io->yaw_deg_len < (io->n_reset_dev ? c->cfg.num_envs : io->n_reset_host))
        return fail(c, ROVER_E_INVALID, "reset_envs: yaw_deg holds %d entries, %d may be read", io->yaw_deg_len,
                    io->n_reset_dev ? c->cfg.num_envs : io->n_reset_host);
    if (io->target3 && (!c->have_stones || !c->have_hf))
        return fail(c, ROVER_E_STATE, "reset_envs: goal validation needs rover_set_stones and rover_set_heightfield");
    if (!io->n_reset_dev && io->n_reset_host == 0) return ROVER_OK;
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    ResetArgs a{};
    a.ids = io->reset_ids; a.id_offset = c->cfg.env_offset; a.n_host = (uint32_t)io->n_reset_host; a.n_dev = io->n_reset_dev;
    a.initial_pos3 = io->initial_pos3; a.pos3 = io->pos3; a.quat4 = io->quat4; a.joint_pos13 = io->joint_pos13;
    a.joint_vel13 = io->joint_vel13; a.base_pos3 = io->base_pos3; a.reset = io->reset; a.progress = io->progress;
    a.yaw_deg = io->yaw_deg; a.seed = io->seed; a.seed_dev = io->seed_dev;
    const uint32_t n_max = io->n_reset_dev ? (uint32_t)c->cfg.num_envs : (uint32_t)io->n_reset_host;
    HIP_TRY(c, launch_reset_envs(a, n_max, s));
    if (io->target3) {
        GoalArgs g{c->d_stones.get(), (uint32_t)c->S, c->hf, c->sgrid, io->reset_ids, (int64_t)c->cfg.env_offset, (uint32_t)io->n_reset_host,
                   io->n_reset_dev, io->initial_pos3, io->target3, io->radius > 0.f ? io->radius : 8.0f, io->draws,
                   io->max_draws > 0 ? io->max_draws : 256, io->seed, io->seed_dev, (int32_t*)c->d_goal_work.get(), io->n_draws_used};
        HIP_TRY(c, launch_generate_goals(g, n_max, s));
    }
    return ROVER_OK;
}

int rover_pre_physics_step(rover_ctx* c, const float* actions, const float* quat, float* lin_hist, float* ang_hist,
                           float* euler_pre, float* pos_targets13, float* vel_targets13, float* actions_nn, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!actions || !lin_hist || !ang_hist) return fail(c, ROVER_E_INVALID, "pre_physics_step: actions and both histories are required");
    if (euler_pre && !quat) return fail(c, ROVER_E_INVALID, "pre_physics_step: euler_pre needs quat");
    USE_DEVICE(c);
    PrePhysicsArgs a{(uint32_t)c->cfg.num_envs, actions, quat, lin_hist, ang_hist, euler_pre, pos_targets13, vel_targets13, actions_nn};
    HIP_TRY(c, launch_pre_physics(a, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_ackermann(rover_ctx* c, const float* lin, const float* ang, int32_t n, float* steering, float* velocities, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (n < 0 || (n > 0 && (!lin || !ang || !steering || !velocities))) return fail(c, ROVER_E_INVALID, "ackermann: bad arguments");
    if (n == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_ackermann(lin, ang, (uint32_t)n, steering, velocities, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_get_info(const rover_ctx* c, rover_info* info) {
    if (!c || !info) return ROVER_E_INVALID;
    memset(info, 0, sizeof *info);
    info->P = c->P; info->Ns = c->Ns; info->Nd = c->Nd; info->rays_per_env_padded = (int32_t)c->plan.R8;
    for (int w = 0; w < 2; ++w) {
        info->K[w] = c->maps[w].knn.K; info->K8[w] = c->maps[w].knn.K8; info->X[w] = c->maps[w].knn.X; info->Y[w] = c->maps[w].knn.Y;
        info->table_bytes[w] = c->maps[w].bytes();
    }
    // the per-step workspace: ray records, distances, sort buffers, env records, and the culled ray cast's queue + counters
    info->workspace_bytes = c->workspace_bytes + c->queue.entries.bytes() + c->queue.stats.bytes();
    info->raycast_variant = c->plan.variant;
    info->cell_index_mode = c->cell_rcp; info->ray_precision = c->precision;
    info->raycast_sorted = c->plan.sorted ? 1 : 0;
    info->raycast_rocks_staged = c->plan.rocks_staged ? 1 : 0;
    for (int w = 0; w < 2; ++w) { info->lane_box[w] = c->maps[w].lane_box ? 1 : 0; info->lane_pair_rows[w] = c->maps[w].lane_pair_rows ? 1 : 0; }
    return ROVER_OK;
}

int rover_get_raycast_plan(const rover_ctx* c, rover_raycast_plan* out) {
    if (!c || !out) return ROVER_E_INVALID;
    memset(out, 0, sizeof *out);
    plan_to_c(c->plan, out);
    return ROVER_OK;
}

int rover_get_cull_info(rover_ctx* c, rover_cull_info* out) {
    if (!c || !out) return ROVER_E_INVALID;
    memset(out, 0, sizeof *out);
    for (int w = 0; w < 2; ++w) {             // (of the proof tables the precision in force uses)
        const MapTables& m = c->maps[w];
        out->triangles[w] = m.tris;
        out->always_candidate_triangles[w] = m.proof[c->plan.proof].always;
        out->cells_without_cone[w] = m.proof[c->plan.proof].nocone;
        out->cells_with_far_bound[w] = m.farok;
    }
    out->far_records_on_demand = (c->have_dist && c->maps[0].table.get()) ? (uint64_t)c->plan.lazy_far : 0;
    const CullQueue& q = c->queue;
    out->queue_bytes = q.entries.bytes();
    out->launches_per_step = q.entries.get() ? q.sized_for.cull_launches : 0;
    if (!q.stats.get() || c->ws_plan.variant < 3) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, hipDeviceSynchronize());
    std::vector<uint4> h(q.stats.bytes() / sizeof(uint4));
    HIP_TRY(c, hipMemcpy(h.data(), q.stats.get(), q.stats.bytes(), hipMemcpyDeviceToHost));
    for (const uint4& v : h) {
        out->candidate_pairs += v.x; out->rays += v.y & 0xffu; out->rays_far_skipped += v.y >> 8; out->rays_both_tests += v.z & 0xffu; out->rays_not_scanned += v.z >> 8; out->bins += v.w & 0xffu;
        out->lane_items += (v.w >> 8) & 0x3ffffu; out->lane_flushes += v.w >> 26;      // (zero in the words the culled kernel's waves write)
        out->max_pairs_per_run = v.x > out->max_pairs_per_run ? v.x : out->max_pairs_per_run;
    }
    return ROVER_OK;
}

int rover_set_option(rover_ctx* c, const char* name, int64_t value) {
    if (!c || !name) return ROVER_E_INVALID;
    USE_DEVICE(c);                                 // some options (re)allocate device workspace
    const KnobRow* k = knob_by_option(name);
    if (!k) return fail(c, ROVER_E_INVALID, "unknown option '%s'", name);
    if (!knob_option_accepts(*k, (double)value)) return fail(c, ROVER_E_INVALID, "%s must be %s", name, k->values);
    if ((k->flags & KNOB_MUST_RUN) && value == 4 && staged_tables_missing(plan_inputs(c)))
        return fail(c, ROVER_E_STATE, "raycast_variant 4 (staged) needs its tables for the arithmetic in force: they were not built (option "
                                      "staged_tables, or they did not fit when the maps were set)");
    k->set(c, (double)value);
    if (k->invalidates & KNOB_RAYS_OBS) {
        c->hf.rcp = c->cell_rcp;
        c->rays_valid = false;
        c->obs_valid = false;
    }
    return (k->invalidates & KNOB_REPLAN) ? replan(c, (k->invalidates & KNOB_BINS) ? REALLOC_BINS : REALLOC_QUEUE) : ROVER_OK;
}

int rover_plan_raycast(const rover_plan_query* q, rover_raycast_plan* out) {
    if (!q || !out) return fail(nullptr, ROVER_E_INVALID, "plan_raycast: null argument");
    if (q->num_envs <= 0 || q->P < 0 || (q->have_dist && q->P == 0))
        return fail(nullptr, ROVER_E_INVALID, "plan_raycast: num_envs=%d P=%d have_dist=%d", q->num_envs, q->P, q->have_dist);
    const struct { const char* option; int64_t value; } given[] = {
        {"raycast_variant", q->raycast_variant}, {"raycast_run", q->raycast_run}, {"lane_env_order", q->lane_env_order}, {"lane_rocks", q->lane_rocks},
        {"bin_low_bits", q->bin_low_bits}, {"cull_queue_mb", q->cull_queue_mb}, {"ray_precision", q->ray_precision}};
    for (const auto& g : given)
        if (!knob_option_accepts(*knob_by_option(g.option), (double)g.value))
            return fail(nullptr, ROVER_E_INVALID, "plan_raycast: %s must be %s", g.option, knob_by_option(g.option)->values);
    PlanInputs in;
    in.num_envs = q->num_envs; in.P = q->P; in.have_dist = q->have_dist != 0; in.precision = q->ray_precision;
    in.knobs.variant = q->raycast_variant; in.knobs.run = (uint32_t)q->raycast_run; in.knobs.lane_env_order = q->lane_env_order;
    in.knobs.lane_rocks = q->lane_rocks; in.knobs.cull_lazy = q->cull_lazy; in.knobs.low_bits_opt = (uint32_t)q->bin_low_bits;
    in.knobs.cull_budget = (uint64_t)q->cull_queue_mb << 20;
    for (int w = 0; w < 2; ++w) {
        MapShape& m = in.map[w];
        if (q->map_present[w] && (q->X[w] <= 0 || q->Y[w] <= 0 || q->K8[w] <= 0 || q->K8[w] % 8 || q->cells_with_far_bound[w] < 0 ||
                                  q->cells_with_far_bound[w] > (int64_t)q->X[w] * q->Y[w]))
            return fail(nullptr, ROVER_E_INVALID, "plan_raycast: map %d: X=%d Y=%d K8=%d cells_with_far_bound=%lld", w, q->X[w], q->Y[w], q->K8[w],
                        (long long)q->cells_with_far_bound[w]);
        if (!q->map_present[w]) continue;
        m.present = true; m.X = q->X[w]; m.Y = q->Y[w]; m.K8 = q->K8[w]; m.cells = (int64_t)q->X[w] * q->Y[w]; m.farok = q->cells_with_far_bound[w];
        m.has_cull_tables = q->has_cull_tables[w] != 0;
        for (int k = 0; k < 2; ++k) m.has_staged_tables[k] = q->has_staged_tables[w][k] != 0;
    }
    memset(out, 0, sizeof *out);
    plan_to_c(plan_step(in), out);
    return ROVER_OK;
}

int rover_set_profiling(rover_ctx* c, int32_t enable) {
    if (!c) return ROVER_E_INVALID;
    USE_DEVICE(c);
    if (enable && c->ev0.empty()) {
        // created into locals and swapped in only when all 2 x 256 exist: a partial failure leaves the ctx without events
        std::vector<hipEvent_t> e0, e1;
        hipError_t e = hipSuccess;
        for (int i = 0; i < kProfRing && e == hipSuccess; ++i) {
            hipEvent_t a = nullptr, b = nullptr;
            e = hipEventCreate(&a);
            if (e == hipSuccess) { e0.push_back(a); e = hipEventCreate(&b); }
            if (e == hipSuccess) e1.push_back(b);
        }
        if (e != hipSuccess) {
            for (auto& x : e0) (void)hipEventDestroy(x);
            for (auto& x : e1) (void)hipEventDestroy(x);
            return fail(c, ROVER_E_HIP, "set_profiling: hipEventCreate: %s", hipGetErrorString(e));
        }
        c->ev0.swap(e0); c->ev1.swap(e1);
    }
    if (c->prof_pending) (void)prof_drain(c);
    c->profiling = enable != 0;
    if (enable) { c->prof_ms = 0.0; c->prof_launches = 0; c->prof_seen = 0; c->prof_every = enable > 1 ? enable : 1; }
    return ROVER_OK;
}

int rover_get_profile(rover_ctx* c, rover_profile* out) {
    if (!c || !out) return ROVER_E_INVALID;
    USE_DEVICE(c);
    if (prof_drain(c)) return fail(c, ROVER_E_HIP, "get_profile: event drain failed");
    out->raycast_ms = c->prof_ms;
    out->launches = c->prof_launches;
    out->pairs_per_launch = (uint64_t)c->cfg.num_envs * ((uint64_t)c->P * (uint64_t)c->maps[0].knn.K + 26ull * (uint64_t)c->maps[1].knn.K);
    return ROVER_OK;
}

int rover_replay_raycast(rover_ctx* c, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (int r = check_ready(c)) return r;
    if (!c->rays_valid) return fail(c, ROVER_E_STATE, "replay_raycast: no ray records yet (run a step first)");
    USE_DEVICE(c);
    StepPlan p = c->plan;
    if (p.sorted && !c->ws_plan.sorted) { p = StepPlan{}; p.variant = 1; p.R8 = c->plan.R8; }     // no sorted list from the last step: only an env-order kernel can replay
    if (int r = check_queue(c, p)) return r;
    return run_raycast(c, p, (uint32_t)c->cfg.num_envs * (26u + (uint32_t)c->P), (hipStream_t)stream);
}

}  // extern "C"
