// rover_raster.hip — the heightfield of a triangle mesh (rover_build_heightfield; the definition is written out in include/rover_step.h
// and DESIGN.md §4.18): for every node of an N0 x N1 grid the highest point of the mesh above it.
//
// Coverage is the hardware rasterisers' fixed-point rule: every vertex is snapped once to 1/256 of the node spacing (snap kernel, one
// 16-byte record per vertex), a node is inside a triangle iff its three integer edge functions are >= 0.  That is exact int64
// arithmetic — watertight, independent of the order of triangles and of lanes.  The height is the barycentric combination in f64, rounded
// to f32 once, and reaches hm through an integer atomicMax on an order-preserving key of the f32 bits (key 0 = never covered): an integer
// maximum does not depend on arrival order, so every run writes the same bits.  No float atomics.
//
// Triangles scatter into the nodes of their bounding box, by one of two routes (rover_heightfield_limits):
//   small  box of <= RASTER_SMALL_NODES nodes: a group of RASTER_GROUP lanes (a quarter wave) per triangle strides over the box,
//          neighbouring lanes on neighbouring j (the contiguous axis);
//   large  appended to a list (one atomic per wave: the wave's large triangles are ranked by a ballot) with the number of grid-aligned
//          RASTER_TILE_I x RASTER_TILE_J tiles its box touches; the host turns the counts into tile offsets and a second launch
//          rasterises one (triangle, tile) per workgroup — a wave covers 64 consecutive j of one row per atomic instruction (256
//          contiguous bytes), and a tile that lies wholly outside one edge is dropped after four corner tests.
// A last pass decodes the keys in place, writes `fill` into the nodes no triangle covered and counts them (one atomic per block).
//
// Built with -ffp-contract=off: every written f64 operation is one IEEE rounding, in the written order (tests/raster_ref.py restates it).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rover_internal.h"

namespace rover {

// one snapped vertex: X, Y in sub-units (|.| <= 2^25), z as given, ok = 0 where a coordinate is not finite or X / Y is out of range
struct SnapVert { int32_t X, Y; float z; uint32_t ok; };
static_assert(sizeof(SnapVert) == 16, "SnapVert must be 16 bytes");

__global__ void __launch_bounds__(256) raster_snap_kernel(const float* __restrict__ v, uint32_t V, float hs, float shift_x, float shift_y,
                                                          SnapVert* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= V) return;
    const float x = v[3ull * i], y = v[3ull * i + 1], z = v[3ull * i + 2];
    const double X = rint((((double)x - (double)shift_x) / (double)hs) * 256.0);
    const double Y = rint((((double)y - (double)shift_y) / (double)hs) * 256.0);
    const double lim = (double)RASTER_MAX_SNAP;
    // (a NaN or infinite X / Y fails its comparison)
    const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && fabs(X) <= lim && fabs(Y) <= lim;
    SnapVert s;
    s.X = ok ? (int32_t)X : 0; s.Y = ok ? (int32_t)Y : 0; s.z = z; s.ok = ok ? 1u : 0u;
    *reinterpret_cast<int4*>(out + i) = *reinterpret_cast<const int4*>(&s);
}

struct TriSetup {
    int32_t ax, ay, bx, by, cx, cy;
    float za, zb, zc;
    int64_t area;                    // > 0: the oriented area
    int32_t neg;                     // the stored winding had area < 0: the three weights are negated
    int32_t i0, i1, j0, j1;          // the nodes of the bounding box, clipped to the grid (inclusive)
};

enum { TRI_NOTHING = 0, TRI_DRAW = 1, TRI_SKIPPED = 2 };

__device__ __forceinline__ SnapVert load_snap(const SnapVert* sv, int32_t i) {
    const int4 r = *reinterpret_cast<const int4*>(sv + i);
    SnapVert s;
    s.X = r.x; s.Y = r.y; s.z = __int_as_float(r.z); s.ok = (uint32_t)r.w;
    return s;
}

// TRI_SKIPPED: an index outside [0, V) or a vertex that is not ok (counted); TRI_NOTHING: zero area, or a box that holds no node
__device__ __forceinline__ int tri_setup(const RasterArgs& a, uint32_t t, TriSetup& s) {
    const int32_t ia = a.tris[3ull * t], ib = a.tris[3ull * t + 1], ic = a.tris[3ull * t + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= a.V || ib >= a.V || ic >= a.V) return TRI_SKIPPED;
    const SnapVert* sv = static_cast<const SnapVert*>(a.snap);
    const SnapVert A = load_snap(sv, ia), B = load_snap(sv, ib), C = load_snap(sv, ic);
    if (!(A.ok & B.ok & C.ok)) return TRI_SKIPPED;
    s.ax = A.X; s.ay = A.Y; s.bx = B.X; s.by = B.Y; s.cx = C.X; s.cy = C.Y;
    s.za = A.z; s.zb = B.z; s.zc = C.z;
    const int64_t area = (int64_t)(s.bx - s.ax) * (int64_t)(s.cy - s.ay) - (int64_t)(s.by - s.ay) * (int64_t)(s.cx - s.ax);
    if (area == 0) return TRI_NOTHING;
    s.neg = area < 0;
    s.area = area < 0 ? -area : area;
    const int32_t min_x = min(s.ax, min(s.bx, s.cx)), max_x = max(s.ax, max(s.bx, s.cx));
    const int32_t min_y = min(s.ay, min(s.by, s.cy)), max_y = max(s.ay, max(s.by, s.cy));
    // node i sits at 256 i: ceil(min / 256) .. floor(max / 256) (the shift is arithmetic: it floors negative values too)
    s.i0 = max((min_x + (RASTER_SUB - 1)) >> 8, 0); s.i1 = min(max_x >> 8, a.N0 - 1);
    s.j0 = max((min_y + (RASTER_SUB - 1)) >> 8, 0); s.j1 = min(max_y >> 8, a.N1 - 1);
    return (s.i0 <= s.i1 && s.j0 <= s.j1) ? TRI_DRAW : TRI_NOTHING;
}

// the three edge functions of the oriented triangle at node (i, j)
__device__ __forceinline__ void edge_functions(const TriSetup& s, int32_t i, int32_t j, int64_t& wa, int64_t& wb, int64_t& wc) {
    const int64_t px = (int64_t)i << 8, py = (int64_t)j << 8;
    wa = (int64_t)(s.cx - s.bx) * (py - s.by) - (int64_t)(s.cy - s.by) * (px - s.bx);
    wb = (int64_t)(s.ax - s.cx) * (py - s.cy) - (int64_t)(s.ay - s.cy) * (px - s.cx);
    wc = (int64_t)(s.bx - s.ax) * (py - s.ay) - (int64_t)(s.by - s.ay) * (px - s.ax);
    if (s.neg) { wa = -wa; wb = -wb; wc = -wc; }
}

// order-preserving key of an f32: larger value <=> larger key, -0 below +0, and never 0
__device__ __forceinline__ uint32_t height_key(float z) {
    const uint32_t b = __float_as_uint(z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ void raster_node(const RasterArgs& a, const TriSetup& s, int32_t i, int32_t j) {
    int64_t wa, wb, wc;
    edge_functions(s, i, j, wa, wb, wc);
    if ((wa | wb | wc) < 0) return;                   // some weight is negative: outside
    const double z = (((double)wa * (double)s.za + (double)wb * (double)s.zb) + (double)wc * (double)s.zc) / (double)s.area;
    atomicMax(a.keys + ((uint64_t)i * (uint32_t)a.N1 + (uint32_t)j), height_key((float)z));
}

__device__ __forceinline__ uint32_t tiles_of(const TriSetup& s) {
    const uint32_t ti = (uint32_t)((s.i1 / RASTER_TILE_I) - (s.i0 / RASTER_TILE_I) + 1);
    const uint32_t tj = (uint32_t)((s.j1 / RASTER_TILE_J) - (s.j0 / RASTER_TILE_J) + 1);
    return ti * tj;                                   // at most (131072 / 32) (131072 / 64) = 2^23
}

// route "small" for every triangle, and the list of the others
__global__ void __launch_bounds__(256) raster_small_kernel(RasterArgs a) {
    const uint32_t sub = threadIdx.x & (RASTER_GROUP - 1);
    const uint64_t t = (uint64_t)blockIdx.x * (256 / RASTER_GROUP) + (threadIdx.x / RASTER_GROUP);
    TriSetup s;
    int status = TRI_NOTHING;
    if (t < (uint64_t)a.T) status = tri_setup(a, (uint32_t)t, s);
    bool large = false;
    if (status == TRI_DRAW) {
        const uint32_t w = (uint32_t)(s.j1 - s.j0 + 1);
        const uint64_t nodes = (uint64_t)w * (uint32_t)(s.i1 - s.i0 + 1);
        large = nodes > (uint64_t)RASTER_SMALL_NODES;
        if (!large)
            for (uint32_t n = sub; n < (uint32_t)nodes; n += RASTER_GROUP) raster_node(a, s, s.i0 + (int32_t)(n / w), s.j0 + (int32_t)(n % w));
    }
    // one atomic per wave for the list, one for the skipped count: the group leaders are ranked by a ballot
    const uint32_t lane = threadIdx.x & 63u;
    const bool lead = sub == 0;
    const unsigned long long m_large = __ballot(lead && large);
    if (m_large) {
        const int first = __ffsll((long long)m_large) - 1;
        uint32_t base = 0;
        if ((int)lane == first) base = atomicAdd(a.n_large, (uint32_t)__popcll(m_large));
        base = (uint32_t)__shfl((int)base, first);
        if (lead && large) {
            const uint32_t slot = base + (uint32_t)__popcll(m_large & ((1ull << lane) - 1ull));
            a.large_tri[slot] = (uint32_t)t;           // slot < T: every triangle is appended at most once
            a.large_tiles[slot] = tiles_of(s);
        }
    }
    const unsigned long long m_skip = __ballot(lead && status == TRI_SKIPPED);
    if (m_skip && lane == 0) atomicAdd(a.stats + 1, (unsigned long long)__popcll(m_skip));
}

// route "large": workgroup = one (triangle, tile); tile_start [n_large + 1] = the exclusive sum of large_tiles
__global__ void __launch_bounds__(256) raster_large_kernel(RasterArgs a, const uint64_t* __restrict__ tile_start, uint32_t n_large, uint64_t total) {
    const int32_t lane = (int32_t)(threadIdx.x & 63u), wave = (int32_t)(threadIdx.x >> 6);
    for (uint64_t b = blockIdx.x; b < total; b += gridDim.x) {
        uint32_t lo = 0, hi = n_large;                 // tile_start[lo] <= b < tile_start[hi]
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (tile_start[mid] <= b) lo = mid; else hi = mid;
        }
        TriSetup s;
        if (tri_setup(a, a.large_tri[lo], s) != TRI_DRAW) continue;        // (cannot happen: the list holds drawn triangles only)
        const uint32_t local = (uint32_t)(b - tile_start[lo]);
        const uint32_t tiles_j = (uint32_t)((s.j1 / RASTER_TILE_J) - (s.j0 / RASTER_TILE_J) + 1);
        const int32_t ibase = ((s.i0 / RASTER_TILE_I) + (int32_t)(local / tiles_j)) * RASTER_TILE_I;
        const int32_t jbase = ((s.j0 / RASTER_TILE_J) + (int32_t)(local % tiles_j)) * RASTER_TILE_J;
        const int32_t ilo = max(ibase, s.i0), ihi = min(ibase + RASTER_TILE_I - 1, s.i1);
        const int32_t jlo = max(jbase, s.j0), jhi = min(jbase + RASTER_TILE_J - 1, s.j1);
        if (ilo > ihi || jlo > jhi) continue;          // (cannot happen: every listed tile meets the box)
        // an edge function is affine: its maximum over the tile is at a corner; all four below 0 = the tile is outside that edge
        int64_t ma, mb, mc, wa, wb, wc;
        edge_functions(s, ilo, jlo, ma, mb, mc);
        edge_functions(s, ilo, jhi, wa, wb, wc); ma = max(ma, wa); mb = max(mb, wb); mc = max(mc, wc);
        edge_functions(s, ihi, jlo, wa, wb, wc); ma = max(ma, wa); mb = max(mb, wb); mc = max(mc, wc);
        edge_functions(s, ihi, jhi, wa, wb, wc); ma = max(ma, wa); mb = max(mb, wb); mc = max(mc, wc);
        if ((ma | mb | mc) < 0) continue;
        const int32_t j = jbase + lane;
        if (j < jlo || j > jhi) continue;              // (lane-level: no barrier follows)
        for (int32_t i = ibase + wave; i <= ihi; i += 4)
            if (i >= ilo) raster_node(a, s, i, j);
    }
}

// keys -> heights in place; a key of 0 becomes `fill` and is counted
__global__ void __launch_bounds__(256) raster_decode_kernel(uint32_t* __restrict__ keys, uint64_t n, float fill, unsigned long long* __restrict__ stats) {
    __shared__ uint32_t s_count[4];
    uint32_t mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t k = keys[i];
        uint32_t bits;
        if (k == 0u) { bits = __float_as_uint(fill); ++mine; }
        else bits = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
        keys[i] = bits;
    }
    // a thread visits at most n / (gridDim 256) + 1 nodes: the launcher keeps that, times 256, inside 32 bits
    for (int o = 32; o > 0; o >>= 1) mine += (uint32_t)__shfl_down((int)mine, o);
    if ((threadIdx.x & 63u) == 0) s_count[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t c = s_count[0] + s_count[1] + s_count[2] + s_count[3];
        if (c) atomicAdd(stats, (unsigned long long)c);
    }
}

hipError_t launch_raster_snap(const float* vertices, uint32_t V, float hs, float shift_x, float shift_y, void* snap, hipStream_t s) {
    if (V == 0) return hipSuccess;
    hipLaunchKernelGGL(raster_snap_kernel, dim3(blocks_for(V, 256)), dim3(256), 0, s, vertices, V, hs, shift_x, shift_y, (SnapVert*)snap);
    return hipGetLastError();
}

hipError_t launch_raster_small(const RasterArgs& a, hipStream_t s) {
    if (a.T == 0) return hipSuccess;
    hipLaunchKernelGGL(raster_small_kernel, dim3(blocks_for((uint64_t)a.T, 256 / RASTER_GROUP)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_raster_large(const RasterArgs& a, const uint64_t* tile_start, uint32_t n_large, uint64_t total, hipStream_t s) {
    if (n_large == 0 || total == 0) return hipSuccess;
    const uint32_t grid = (uint32_t)(total < (1ull << 20) ? total : (1ull << 20));      // more tiles than that: workgroups take several
    hipLaunchKernelGGL(raster_large_kernel, dim3(grid), dim3(256), 0, s, a, tile_start, n_large, total);
    return hipGetLastError();
}

hipError_t launch_raster_decode(uint32_t* keys, uint64_t n, float fill, unsigned long long* stats, hipStream_t s) {
    const uint64_t blocks = (n + 255) / 256;
    const uint32_t grid = (uint32_t)(blocks < 65536 ? blocks : 65536);                  // n <= 2^34: at most 1024 nodes per thread
    hipLaunchKernelGGL(raster_decode_kernel, dim3(grid), dim3(256), 0, s, keys, n, fill, stats);
    return hipGetLastError();
}

}  // namespace rover
