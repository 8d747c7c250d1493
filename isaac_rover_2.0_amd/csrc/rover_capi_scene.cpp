// rover_capi_scene.cpp — the scene builders of the C-ABI layer (include/rover_step.h): the KNN map builder, the heightfield rasteriser,
// the Mars terrain generator.  They run before an env exists: of the ctx they use the device number and the error string, no member.
#include "../../include/rover_step.h"
#include "rover_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

extern "C" {

// IEEE binary16 <-> binary32 on the host (round to nearest even), for the reference-ranking coordinate tables
static float half_bits_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1fu, man = h & 0x3ffu;
    uint32_t u;
    if (exp == 0) {
        if (man == 0) u = sign;
        else { int e = -1; uint32_t m = man; do { ++e; m <<= 1; } while (!(m & 0x400u)); u = sign | ((uint32_t)(127 - 15 - e) << 23) | ((m & 0x3ffu) << 13); }
    } else if (exp == 31) u = sign | 0x7f800000u | (man << 13);
    else u = sign | ((exp + 112u) << 23) | (man << 13);
    float f; memcpy(&f, &u, sizeof f); return f;
}
static uint16_t float_to_half_bits(float f) {
    uint32_t u; memcpy(&u, &f, sizeof u);
    const uint32_t sign = (u >> 16) & 0x8000u;
    u &= 0x7fffffffu;
    if (u >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (u > 0x7f800000u ? 0x200u : 0u));
    if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                        // rounds to infinity
    if (u < 0x38800000u) {                                                         // subnormal half or zero
        if (u < 0x33000000u) return (uint16_t)sign;
        const int shift = 126 - (int)(u >> 23);                                    // 14 .. 24
        const uint32_t m = (u & 0x7fffffu) | 0x800000u;
        uint32_t r = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
        if (rem > halfway || (rem == halfway && (r & 1u))) ++r;
        return (uint16_t)(sign | r);
    }
    uint32_t r = (u - 0x38000000u) >> 13;
    const uint32_t rem = u & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) ++r;
    return (uint16_t)(sign | r);
}

static int build_knn_map_impl(rover_ctx* c, const float* vertices, int32_t V, const int32_t* triangles, int32_t T, int32_t X, int32_t Y,
                              float res, int32_t K, int ref, const uint16_t* cell_x_f16, const uint16_t* cell_y_f16,
                              int32_t* map_idx_out);

int rover_build_knn_map(rover_ctx* c, const float* vertices, int32_t V, const int32_t* triangles, int32_t T, int32_t X, int32_t Y,
                        float res, int32_t K, int32_t* map_idx_out) {
    return build_knn_map_impl(c, vertices, V, triangles, T, X, Y, res, K, 0, nullptr, nullptr, map_idx_out);
}

int rover_build_knn_map_ref(rover_ctx* c, const float* vertices, int32_t V, const int32_t* triangles, int32_t T, int32_t X, int32_t Y,
                            float res, int32_t K, const uint16_t* cell_x_f16, const uint16_t* cell_y_f16, int32_t* map_idx_out) {
    return build_knn_map_impl(c, vertices, V, triangles, T, X, Y, res, K, 1, cell_x_f16, cell_y_f16, map_idx_out);
}

static int build_knn_map_impl(rover_ctx* c, const float* vertices, int32_t V, const int32_t* triangles, int32_t T, int32_t X, int32_t Y,
                              float res, int32_t K, int ref, const uint16_t* cell_x_f16, const uint16_t* cell_y_f16,
                              int32_t* map_idx_out) {
    if (!c) return ROVER_E_INVALID;
    if (!vertices || !triangles || !map_idx_out || V <= 0 || T <= 0 || X <= 0 || Y <= 0 || K <= 0 || !(res > 0.0f))
        return fail(c, ROVER_E_INVALID, "build_knn_map: bad arguments");
    if (T < K) return fail(c, ROVER_E_INVALID, "build_knn_map: the mesh has %d triangles, fewer than K=%d", T, K);
    if (K > 4096) return fail(c, ROVER_E_INVALID, "build_knn_map: K=%d exceeds the builder's limit of 4096", K);
    USE_DEVICE(c);
    DevBuf<float> d_v, d_cx, d_cy, d_cell;
    DevBuf<int32_t> d_t, d_over;
    DevBuf<uint32_t> d_cur, d_items, d_bs, d_start;
#define KNN_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess) return fail(c, ROVER_E_HIP, "build_knn_map: %s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)
    KNN_TRY(d_v.alloc((size_t)V * 3));
    KNN_TRY(d_t.alloc((size_t)T * 3));
    KNN_TRY(d_cx.alloc(T));
    KNN_TRY(d_cy.alloc(T));
    KNN_TRY(d_items.alloc(T));
    KNN_TRY(d_over.alloc(1));
    KNN_TRY(d_bs.alloc(8192));
    KNN_TRY(hipMemcpy(d_v.get(), vertices, d_v.bytes(), hipMemcpyDefault));
    KNN_TRY(hipMemcpy(d_t.get(), triangles, d_t.bytes(), hipMemcpyDefault));
    KNN_TRY(hipMemset(d_over.get(), 0, sizeof(int32_t)));
    KNN_TRY(launch_knn_centroids(d_v.get(), d_t.get(), (uint32_t)T, (uint32_t)V, ref, d_cx.get(), d_cy.get(), nullptr));
    if (ref) {
        // cell coordinates as fp16 values: the caller's tables (what the reference's torch.arange(0, X res, res, dtype=float16)
        // gave on the host that built the map), or fp16(float(i) * res) — ATen's CUDA arange kernel, the reference's own device
        std::vector<float> cell((size_t)X + (size_t)Y);
        std::vector<uint16_t> hx((size_t)X), hy((size_t)Y);
        if (cell_x_f16) KNN_TRY(hipMemcpy(hx.data(), cell_x_f16, hx.size() * sizeof(uint16_t), hipMemcpyDefault));
        if (cell_y_f16) KNN_TRY(hipMemcpy(hy.data(), cell_y_f16, hy.size() * sizeof(uint16_t), hipMemcpyDefault));
        for (int32_t i = 0; i < X; ++i) cell[(size_t)i] = half_bits_to_float(cell_x_f16 ? hx[(size_t)i] : float_to_half_bits((float)i * res));
        for (int32_t j = 0; j < Y; ++j) cell[(size_t)X + j] = half_bits_to_float(cell_y_f16 ? hy[(size_t)j] : float_to_half_bits((float)j * res));
        KNN_TRY(d_cell.alloc(cell.size()));
        KNN_TRY(hipMemcpy(d_cell.get(), cell.data(), d_cell.bytes(), hipMemcpyHostToDevice));
    }
    // bucket grid over the centroids' bounding box; bucket edge ~ the radius that holds K/4 centroids at mean density
    std::vector<float> hx((size_t)T), hy((size_t)T);
    KNN_TRY(hipMemcpy(hx.data(), d_cx.get(), d_cx.bytes(), hipMemcpyDeviceToHost));
    KNN_TRY(hipMemcpy(hy.data(), d_cy.get(), d_cy.bytes(), hipMemcpyDeviceToHost));
    // (NaN centroids are left out of the box, the first triangle's included: they all land in bucket 0 and rank last)
    float x0 = 0.0f, x1 = 0.0f, y0 = 0.0f, y1 = 0.0f;
    bool any_x = false, any_y = false;
    for (int32_t t = 0; t < T; ++t) {
        if (hx[t] == hx[t]) { x0 = (any_x && x0 < hx[t]) ? x0 : hx[t]; x1 = (any_x && x1 > hx[t]) ? x1 : hx[t]; any_x = true; }
        if (hy[t] == hy[t]) { y0 = (any_y && y0 < hy[t]) ? y0 : hy[t]; y1 = (any_y && y1 > hy[t]) ? y1 : hy[t]; any_y = true; }
    }
    // the largest |coordinate - origin| of any centroid or cell point: knn_select_kernel's stop slack is absolute in it
    const double cell_x1 = (double)((float)(X - 1) * res), cell_y1 = (double)((float)(Y - 1) * res);
    const float span = (float)std::max({(double)x1 - x0, (double)y1 - y0, std::fabs((double)x0), std::fabs(cell_x1 - x0), std::fabs((double)y0),
                                        std::fabs(cell_y1 - y0)});
    const double area = ((double)x1 - x0 + 1e-6) * ((double)y1 - y0 + 1e-6);
    // (an infinite centroid would make the bucket edge infinite or NaN, and the sizing below would never settle)
    if (!std::isfinite(area)) return fail(c, ROVER_E_INVALID, "build_knn_map: the centroids' bounding box is not finite");
    double gsz = std::sqrt(area * (double)K / (4.0 * (double)T));
    if (gsz < (double)res) gsz = (double)res;
    // A cell's search gathers whole rings of buckets into LDS (8192 candidates at most).  On a strongly non-uniform mesh (a
    // decimated terrain: millimetre triangles on the rocks, metre-sized ones between them) a ring sized for the MEAN density can
    // hold more than that next to a dense patch: the bucket edge is halved and the search repeated (same result: the ranking
    // does not depend on the bucket size).
    hipError_t e2 = hipSuccess;
    int32_t over = 0;
    for (int attempt = 0; attempt < 6; ++attempt, gsz *= 0.5) {
        uint32_t nbx = (uint32_t)(((double)x1 - x0) / gsz) + 1, nby = (uint32_t)(((double)y1 - y0) / gsz) + 1;
        while ((uint64_t)nbx * nby > (1u << 22)) { gsz *= 2.0; nbx = (uint32_t)(((double)x1 - x0) / gsz) + 1; nby = (uint32_t)(((double)y1 - y0) / gsz) + 1; attempt = 99; }
        const float g = (float)gsz, inv_g = 1.0f / g;
        const uint32_t nb = nbx * nby;
        d_start.reset();
        KNN_TRY(d_cur.alloc((size_t)nb + 1));
        KNN_TRY(hipMemset(d_cur.get(), 0, d_cur.bytes()));
        KNN_TRY(hipMemset(d_over.get(), 0, sizeof(int32_t)));
        KNN_TRY(launch_knn_bucket(d_cx.get(), d_cy.get(), (uint32_t)T, x0, y0, inv_g, nbx, nby, d_cur.get(), d_items.get(), 1, nullptr));
        KNN_TRY(launch_scan_exclusive(d_cur.get(), nb + 1, d_bs.get(), nullptr));
        e2 = d_start.alloc((size_t)nb + 1);
        if (e2 == hipSuccess) e2 = hipMemcpy(d_start.get(), d_cur.get(), d_cur.bytes(), hipMemcpyDeviceToDevice);
        if (e2 == hipSuccess) e2 = launch_knn_bucket(d_cx.get(), d_cy.get(), (uint32_t)T, x0, y0, inv_g, nbx, nby, d_cur.get(), d_items.get(), 0, nullptr);
        if (e2 == hipSuccess) e2 = launch_knn_select(d_cx.get(), d_cy.get(), d_start.get(), d_items.get(), x0, y0, g, span, nbx, nby, (uint32_t)X, (uint32_t)Y,
                                                     res, (uint32_t)K, d_cell.get(), d_cell.get() ? d_cell.get() + X : nullptr, map_idx_out, d_over.get(), nullptr);
        if (e2 == hipSuccess) e2 = hipDeviceSynchronize();
        over = 0;
        if (e2 == hipSuccess) e2 = hipMemcpy(&over, d_over.get(), sizeof over, hipMemcpyDeviceToHost);
        if (e2 != hipSuccess || !over) break;
    }
#undef KNN_TRY
    if (e2 != hipSuccess) return fail(c, ROVER_E_HIP, "build_knn_map: %s", hipGetErrorString(e2));
    if (over) return fail(c, ROVER_E_INVALID, "build_knn_map: a search ring held more than 8192 candidate triangles (mesh too dense for K=%d)", K);
    return ROVER_OK;
}

// Host only: the sizes that separate the rasteriser's routes
int rover_heightfield_limits(int32_t out[4]) {
    if (!out) return fail(nullptr, ROVER_E_INVALID, "heightfield_limits: null argument");
    out[0] = RASTER_SMALL_NODES; out[1] = RASTER_TILE_I; out[2] = RASTER_TILE_J; out[3] = RASTER_GROUP;
    return ROVER_OK;
}

// The arguments are validated before the ctx is looked at, as for rover_motion_step
int rover_build_heightfield(rover_ctx* c, const float* vertices, int32_t V, const int32_t* triangles, int32_t T, int32_t N0, int32_t N1,
                            float horizontal_scale, float shift_x, float shift_y, float fill, float* hm_out, int64_t stats[2]) {
    if (N0 < 1 || N1 < 1 || N0 > RASTER_MAX_NODES || N1 > RASTER_MAX_NODES)
        return fail(c, ROVER_E_INVALID, "build_heightfield: N0 = %d or N1 = %d is outside 1 .. %d", N0, N1, RASTER_MAX_NODES);
    if (!std::isfinite(horizontal_scale) || !(horizontal_scale > 0.0f))
        return fail(c, ROVER_E_INVALID, "build_heightfield: horizontal_scale = %g is not finite or not > 0", (double)horizontal_scale);
    if (!std::isfinite(shift_x) || !std::isfinite(shift_y))
        return fail(c, ROVER_E_INVALID, "build_heightfield: shift = (%g, %g) is not finite", (double)shift_x, (double)shift_y);
    if (V < 0 || T < 0) return fail(c, ROVER_E_INVALID, "build_heightfield: V = %d or T = %d is negative", V, T);
    if ((V > 0 && !vertices) || (T > 0 && !triangles) || !hm_out)
        return fail(c, ROVER_E_INVALID, "build_heightfield: vertices, triangles and hm_out must be given");
    if (!c) return fail(nullptr, ROVER_E_INVALID, "build_heightfield: null ctx");
    USE_DEVICE(c);
#define HF_TRY(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e__ = (expr);                                                                              \
        if (e__ != hipSuccess) return fail(c, ROVER_E_HIP, "build_heightfield: %s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)
    DevBuf<float> d_v;
    DevBuf<int32_t> d_t;
    DevBuf<uint4> d_snap;
    DevBuf<uint32_t> d_large, d_tiles;
    DevBuf<unsigned long long> d_counts;            // {uncovered, skipped, length of the list}
    DevBuf<uint64_t> d_start;
    const size_t nv = V > 0 ? (size_t)V : 1, nt = T > 0 ? (size_t)T : 1;
    const uint64_t nodes = (uint64_t)N0 * (uint64_t)N1;
    HF_TRY(d_v.alloc(nv * 3));
    HF_TRY(d_t.alloc(nt * 3));
    HF_TRY(d_snap.alloc(nv));
    HF_TRY(d_large.alloc(nt));
    HF_TRY(d_tiles.alloc(nt));
    HF_TRY(d_counts.alloc(3));
    if (V > 0) HF_TRY(hipMemcpy(d_v.get(), vertices, (size_t)V * 3 * sizeof(float), hipMemcpyDefault));
    if (T > 0) HF_TRY(hipMemcpy(d_t.get(), triangles, (size_t)T * 3 * sizeof(int32_t), hipMemcpyDefault));
    HF_TRY(hipMemset(d_counts.get(), 0, d_counts.bytes()));
    HF_TRY(hipMemset(hm_out, 0, nodes * sizeof(float)));                                  // key 0: never covered
    RasterArgs a{};
    a.snap = d_snap.get(); a.tris = d_t.get(); a.V = V; a.T = T; a.N0 = N0; a.N1 = N1;
    a.keys = reinterpret_cast<uint32_t*>(hm_out);
    a.n_large = reinterpret_cast<uint32_t*>(d_counts.get() + 2);
    a.large_tri = d_large.get(); a.large_tiles = d_tiles.get(); a.stats = d_counts.get();
    HF_TRY(launch_raster_snap(d_v.get(), (uint32_t)V, horizontal_scale, shift_x, shift_y, d_snap.get(), nullptr));
    HF_TRY(launch_raster_small(a, nullptr));
    unsigned long long counts[3] = {0, 0, 0};
    HF_TRY(hipMemcpy(counts, d_counts.get(), sizeof counts, hipMemcpyDeviceToHost));      // (synchronises)
    const uint32_t n_large = (uint32_t)(counts[2] & 0xffffffffull);
    if (n_large > (uint32_t)T) return fail(c, ROVER_E_HIP, "build_heightfield: the list holds %u triangles of %d", n_large, T);
    if (n_large) {
        std::vector<uint32_t> tiles(n_large);
        std::vector<uint64_t> start((size_t)n_large + 1);
        HF_TRY(hipMemcpy(tiles.data(), d_tiles.get(), (size_t)n_large * sizeof(uint32_t), hipMemcpyDeviceToHost));
        start[0] = 0;
        for (uint32_t i = 0; i < n_large; ++i) start[(size_t)i + 1] = start[i] + tiles[i];
        HF_TRY(d_start.alloc(start.size()));
        HF_TRY(hipMemcpy(d_start.get(), start.data(), d_start.bytes(), hipMemcpyHostToDevice));
        HF_TRY(launch_raster_large(a, d_start.get(), n_large, start[n_large], nullptr));
    }
    HF_TRY(launch_raster_decode(a.keys, nodes, fill, d_counts.get(), nullptr));
    HF_TRY(hipDeviceSynchronize());
    HF_TRY(hipMemcpy(counts, d_counts.get(), sizeof counts, hipMemcpyDeviceToHost));
#undef HF_TRY
    if (stats) { stats[0] = (int64_t)counts[0]; stats[1] = (int64_t)counts[1]; }
    return ROVER_OK;
}

// ---- Mars terrain generator ----
static_assert(MARS_TILE == ROVER_MARS_TILE, "the kernel's tile is the ABI's");

// shared by rover_mars_heightfield and rover_mars_tiles: true when the descriptor is acceptable, else *why says what is wrong.  This is
// what keeps the kernel inside its buffers: a window or a kept stamp that fails here never reaches the device.
static bool mars_desc_ok(const rover_mars_desc* d, std::string* why) {
    char buf[256];
    buf[0] = 0;
#define MARS_REFUSE(...) do { snprintf(buf, sizeof buf, __VA_ARGS__); *why = buf; return false; } while (0)
    if (!d) MARS_REFUSE("desc is NULL");
    if (d->rows < 1 || d->cols < 1 || d->rows > ROVER_MARS_MAX_SIDE || d->cols > ROVER_MARS_MAX_SIDE)
        MARS_REFUSE("rows = %d or cols = %d is outside 1 .. %d", d->rows, d->cols, ROVER_MARS_MAX_SIDE);
    if (d->n_hills < 0) MARS_REFUSE("n_hills = %d is negative", d->n_hills);
    if (d->n_classes < 0 || d->n_classes > ROVER_MARS_MAX_CLASSES) MARS_REFUSE("n_classes = %d is outside 0 .. %d", d->n_classes, ROVER_MARS_MAX_CLASSES);
    if (d->n_stamps < 0) MARS_REFUSE("n_stamps = %d is negative", d->n_stamps);
    if (d->g_len < 1 || !d->g) MARS_REFUSE("g is NULL or g_len = %d is below 1", d->g_len);
    if (d->n_hills > 0 && (!d->hill_window || !d->hill_amp)) MARS_REFUSE("hill_window or hill_amp is NULL with n_hills = %d", d->n_hills);
    if (d->n_classes > 0 && (!d->class_side || !d->class_tables)) MARS_REFUSE("class_side or class_tables is NULL with n_classes = %d", d->n_classes);
    if (d->n_stamps > 0 && (!d->stamp_row || !d->stamp_col || !d->stamp_class || !d->stamp_factor || !d->stamp_kept))
        MARS_REFUSE("a stamp array is NULL with n_stamps = %d", d->n_stamps);
    for (int32_t k = 0; k < d->n_classes; ++k)
        if (d->class_side[k] < 1 || d->class_side[k] > ROVER_MARS_MAX_TABLE)
            MARS_REFUSE("class_side[%d] = %d is outside 1 .. %d", k, d->class_side[k], ROVER_MARS_MAX_TABLE);
    for (int32_t i = 0; i < d->n_hills; ++i) {
        const int32_t* w = d->hill_window + 6 * (size_t)i;
        const int64_t r0 = w[0], r1 = w[1], c0 = w[2], c1 = w[3], a0 = w[4], b0 = w[5];
        if (r0 < 0 || r1 < r0 || r1 > d->rows || c0 < 0 || c1 < c0 || c1 > d->cols)
            MARS_REFUSE("hill_window[%d] = rows %d:%d, columns %d:%d is not inside the %d x %d field", i, w[0], w[1], w[2], w[3], d->rows, d->cols);
        if (a0 < 0 || b0 < 0 || a0 + (r1 - r0) > d->g_len || b0 + (c1 - c0) > d->g_len)
            MARS_REFUSE("hill_window[%d] reads g from %d and %d: outside its %d entries", i, w[4], w[5], d->g_len);
        if (!std::isfinite(d->hill_amp[i])) MARS_REFUSE("hill_amp[%d] is not finite", i);
    }
    for (int32_t s = 0; s < d->n_stamps; ++s) {
        if (!d->stamp_kept[s]) continue;
        const int32_t k = d->stamp_class[s];
        if (k < 0 || k >= d->n_classes) MARS_REFUSE("stamp_class[%d] = %d is outside 0 .. %d", s, k, d->n_classes - 1);
        const int64_t side = d->class_side[k], r = d->stamp_row[s], c = d->stamp_col[s];
        if (r < 0 || c < 0 || r + side > d->rows || c + side > d->cols)
            MARS_REFUSE("stamp %d (stamp_row = %d, stamp_col = %d, side %d) is not inside the %d x %d field", s, d->stamp_row[s], d->stamp_col[s],
                        (int)side, d->rows, d->cols);
        if (!std::isfinite(d->stamp_factor[s])) MARS_REFUSE("stamp_factor[%d] is not finite", s);
    }
#undef MARS_REFUSE
    return true;
}

static inline uint32_t mars_tiles_of(int32_t n) { return ((uint32_t)n + MARS_TILE - 1) / MARS_TILE; }

// the total length of the tile lists of a descriptor that passed mars_desc_ok
static int64_t mars_count_items(const rover_mars_desc& d) {
    int64_t total = 0;
    for (int32_t s = 0; s < d.n_stamps; ++s) {
        if (!d.stamp_kept[s]) continue;
        const int32_t side = d.class_side[d.stamp_class[s]], r = d.stamp_row[s], c = d.stamp_col[s];
        total += (int64_t)((r + side - 1) / MARS_TILE - r / MARS_TILE + 1) * ((c + side - 1) / MARS_TILE - c / MARS_TILE + 1);
    }
    return total;
}

// start [tiles + 1], items [mars_count_items]: the stamps are visited in index order, so every tile's list is ascending
static void mars_fill_lists(const rover_mars_desc& d, int32_t* start, int32_t* items) {
    const uint32_t tiles_c = mars_tiles_of(d.cols);
    const size_t tiles = (size_t)mars_tiles_of(d.rows) * tiles_c;
    std::fill(start, start + tiles + 1, 0);
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<int32_t> cursor;
        if (pass == 1) {                                  // counts -> exclusive sum
            int32_t sum = 0;
            for (size_t t = 0; t <= tiles; ++t) { const int32_t n = start[t]; start[t] = sum; sum += n; }
            cursor.assign(start, start + tiles);
        }
        for (int32_t s = 0; s < d.n_stamps; ++s) {
            if (!d.stamp_kept[s]) continue;
            const int32_t side = d.class_side[d.stamp_class[s]], r = d.stamp_row[s], c = d.stamp_col[s];
            for (int32_t ti = r / MARS_TILE; ti <= (r + side - 1) / MARS_TILE; ++ti)
                for (int32_t tj = c / MARS_TILE; tj <= (c + side - 1) / MARS_TILE; ++tj) {
                    const size_t t = (size_t)ti * tiles_c + (size_t)tj;
                    if (pass == 0) ++start[t]; else items[cursor[t]++] = s;
                }
        }
    }
}

int rover_mars_tiles(const rover_mars_desc* d, int32_t* tile_start, int32_t* tile_items, int64_t capacity, int64_t* n_items) {
    std::string why;
    if (!mars_desc_ok(d, &why)) return fail(nullptr, ROVER_E_INVALID, "mars_tiles: %s", why.c_str());
    if (!n_items) return fail(nullptr, ROVER_E_INVALID, "mars_tiles: n_items is NULL");
    const int64_t n = mars_count_items(*d);
    if (n > INT32_MAX) return fail(nullptr, ROVER_E_INVALID, "mars_tiles: the tile lists hold %lld items, more than 2^31 - 1", (long long)n);
    const bool want = tile_start || tile_items;
    if (want && (!tile_start || (!tile_items && n > 0))) return fail(nullptr, ROVER_E_INVALID, "mars_tiles: tile_start and tile_items go together");
    if (capacity < 0 || (want && capacity < n))
        return fail(nullptr, ROVER_E_INVALID, "mars_tiles: capacity %lld < %lld items", (long long)capacity, (long long)n);
    if (want) mars_fill_lists(*d, tile_start, tile_items);
    *n_items = n;
    return ROVER_OK;
}

// The arguments are validated before the ctx is looked at, as for rover_build_heightfield
int rover_mars_heightfield(rover_ctx* c, const rover_mars_desc* d, double* hf, uint8_t* rock_mask, void* stream) {
    std::string why;
    if (!mars_desc_ok(d, &why)) return fail(c, ROVER_E_INVALID, "mars_heightfield: %s", why.c_str());
    if (!hf) return fail(c, ROVER_E_INVALID, "mars_heightfield: hf is NULL");
    const int64_t n_items = mars_count_items(*d);
    if (n_items > INT32_MAX) return fail(c, ROVER_E_INVALID, "mars_heightfield: the tile lists hold %lld items, more than 2^31 - 1", (long long)n_items);
    if (!c) return fail(nullptr, ROVER_E_INVALID, "mars_heightfield: null ctx");
    USE_DEVICE(c);
#define MARS_TRY(expr)                                                                                        \
    do {                                                                                                      \
        hipError_t e__ = (expr);                                                                              \
        if (e__ != hipSuccess) return fail(c, ROVER_E_HIP, "mars_heightfield: %s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)
    // host tables in the kernel's records
    const uint32_t tiles_r = mars_tiles_of(d->rows), tiles_c = mars_tiles_of(d->cols);
    const size_t tiles = (size_t)tiles_r * tiles_c;
    std::vector<MarsHill> hills((size_t)d->n_hills);
    for (int32_t i = 0; i < d->n_hills; ++i) {
        const int32_t* w = d->hill_window + 6 * (size_t)i;
        hills[i] = MarsHill{w[0], w[1], w[2], w[3], w[4], w[5], d->hill_amp[i]};
    }
    uint32_t table_at[ROVER_MARS_MAX_CLASSES + 1] = {0};
    for (int32_t k = 0; k < d->n_classes; ++k) table_at[k + 1] = table_at[k] + (uint32_t)(d->class_side[k] * d->class_side[k]);
    const size_t table_doubles = table_at[d->n_classes];
    std::vector<MarsStamp> stamps((size_t)d->n_stamps, MarsStamp{0, 0, 0u, 0u, 0.0, 0.0});
    for (int32_t s = 0; s < d->n_stamps; ++s)
        if (d->stamp_kept[s]) {
            const int32_t k = d->stamp_class[s];
            stamps[s] = MarsStamp{d->stamp_row[s], d->stamp_col[s], (uint32_t)d->class_side[k], table_at[k], d->stamp_factor[s], 0.0};
        }
    std::vector<int32_t> start(tiles + 1), items((size_t)n_items);
    mars_fill_lists(*d, start.data(), items.data());
    DevBuf<MarsHill> d_hills;
    DevBuf<MarsStamp> d_stamps;
    DevBuf<double> d_g, d_tables;
    DevBuf<int32_t> d_start, d_items;
    MARS_TRY(d_hills.alloc(std::max<size_t>(hills.size(), 1)));
    MARS_TRY(d_stamps.alloc(std::max<size_t>(stamps.size(), 1)));
    MARS_TRY(d_g.alloc((size_t)d->g_len));
    MARS_TRY(d_tables.alloc(std::max<size_t>(table_doubles, 1)));
    MARS_TRY(d_start.alloc(start.size()));
    MARS_TRY(d_items.alloc(std::max<size_t>(items.size(), 1)));
    if (!hills.empty()) MARS_TRY(hipMemcpy(d_hills.get(), hills.data(), hills.size() * sizeof(MarsHill), hipMemcpyHostToDevice));
    if (!stamps.empty()) MARS_TRY(hipMemcpy(d_stamps.get(), stamps.data(), stamps.size() * sizeof(MarsStamp), hipMemcpyHostToDevice));
    MARS_TRY(hipMemcpy(d_g.get(), d->g, (size_t)d->g_len * sizeof(double), hipMemcpyHostToDevice));
    if (table_doubles) MARS_TRY(hipMemcpy(d_tables.get(), d->class_tables, table_doubles * sizeof(double), hipMemcpyHostToDevice));
    MARS_TRY(hipMemcpy(d_start.get(), start.data(), start.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!items.empty()) MARS_TRY(hipMemcpy(d_items.get(), items.data(), items.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    MarsArgs a{};
    a.hf = hf; a.mask = rock_mask; a.rows = d->rows; a.cols = d->cols; a.tiles_r = tiles_r; a.tiles_c = tiles_c;
    a.hills = d_hills.get(); a.n_hills = d->n_hills; a.g = d_g.get(); a.tables = d_tables.get(); a.stamps = d_stamps.get();
    a.tile_start = d_start.get(); a.tile_items = d_items.get();
    MARS_TRY(launch_mars_heightfield(a, (hipStream_t)stream));
    MARS_TRY(hipStreamSynchronize((hipStream_t)stream));          // the tables above are freed on return
#undef MARS_TRY
    return ROVER_OK;
}

}  // extern "C"
