// sr_overlap.hip -- sr_overlap_triangles: the triangles of the model that cross each triangle of a batch, lowest TriangleIndex first, with
// a count and the mask of every pair (gfx950).
//
// For query triangle A and scene triangle j the pair is REPORTED iff tri_overlap_mask(A, v9[j]) != 0 (sr_tri_overlap.h: all 18 coordinates
// finite, the FP64 boxes overlap, an edge of one meets the other; one text for these kernels, the host check and the numpy model).
// count = the number of reported j, the row = the first min(count, K) of them by j ascending with their masks (OverlapList, same header).
// A REGULAR query (each vertex passes closest_regular) walks the own BVH in k_cp_walk's frame (sr_closest.hip): one lane per query, a
// while-while walk with an LDS stack.  The cull: the query's FP64 box relative to the root centre, rounded to fp32 and widened
// OUTWARD, against a child's stored fp32 box, closed on all three axes -- a box-against-box test, so there is no nearer child, no bound on
// the stack and no re-test on a pop.  Every other query of a pass, and every query of brute force, runs the per-record loop over v9 in
// index order.  SR_OVERLAP_ANY: a query stops at its first reported triangle and its count is 1.
// The pass driver and the lane's pick are sr_batch.h's; the keys of a pass (the Morton cell of the centre of the query's box) and the two
// kernels are this file's.
#include <hipcub/hipcub.hpp>

#include "sr_batch.h"
#include "sr_closest.h"
#include "sr_tri_overlap.h"

namespace sr {

extern __shared__ __attribute__((aligned(16))) unsigned char lds_overlap[];

__device__ __forceinline__ unsigned int ot_spread7(unsigned int v) {       // 7 bits -> every third bit (k_cp_keys' spread)
    v &= 0x7fu;
    v = (v | (v << 8)) & 0x700fu;
    v = (v | (v << 4)) & 0x430c3u;
    v = (v | (v << 2)) & 0x49249u;
    return v;
}

__device__ __forceinline__ void ot_fetch(const double* __restrict__ tris, size_t i, double A[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) A[k] = tris[i * 9 + k];
}

// Key of a pass's query: the 7-bit Morton cell of the centre of its FP64 box in the root box (centres outside clamp to the edge cells), 21
// bits; `skip` (point_order_skip_mask) marks an IRREGULAR query -- a vertex fails closest_regular -- which the walk never sees: the stable
// sort leaves those at the end of the pass in input order.  !sorted: the key is that bit alone (a compaction that keeps the input order).
__global__ __launch_bounds__(256) void k_ot_keys(const double* __restrict__ tris, unsigned int n, int sorted, unsigned int skip, double lx, double ly,
                                                 double lz, double sx, double sy, double sz, double cx, double cy, double cz, double diag,
                                                 unsigned int* __restrict__ keys, unsigned int* __restrict__ idx) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    double A[9];
    ot_fetch(tris, i, A);
    const double centre[3] = {cx, cy, cz};
    unsigned int key = 0u;
    if (!closest_regular(A, centre, diag) || !closest_regular(A + 3, centre, diag) || !closest_regular(A + 6, centre, diag)) key = skip;
    else if (sorted) {
        double lo[3], hi[3];
        ov_box(A, lo, hi);
        const double mx = (lo[0] + hi[0]) * 0.5, my = (lo[1] + hi[1]) * 0.5, mz = (lo[2] + hi[2]) * 0.5;
        const int kx = (int)fmin(127.0, fmax(0.0, (mx - lx) * sx)), ky = (int)fmin(127.0, fmax(0.0, (my - ly) * sy)), kz = (int)fmin(127.0, fmax(0.0, (mz - lz) * sz));
        key = (ot_spread7((unsigned)kx) << 2) | (ot_spread7((unsigned)ky) << 1) | ot_spread7((unsigned)kz);
    }
    keys[i] = key;
    idx[i] = i;
}

struct OtArgs {
    const double* tris;
    PassSlice pass;
    int K, any;
    uint32_t* out_count;         // [n] or nullptr
    int32_t*  out_index;         // [n][K] or nullptr: then the rows of s_index, [pass][K]
    uint8_t*  out_mask;          // [n][K] or nullptr
    int32_t*  s_index;
    unsigned long long* stats;
};

__device__ __forceinline__ void ot_rows(const OtArgs& a, size_t i, unsigned int src, OverlapList& L) {
    int32_t* ir = nullptr;
    if (a.K > 0) ir = a.out_index ? a.out_index + i * (size_t)a.K : a.s_index + (size_t)src * (size_t)a.K;
    L.init(ir, a.K);
}
// the end of a query: the sorted row, its masks, the count
__device__ __forceinline__ void ot_store(const DevScene& sc, const OtArgs& a, size_t i, const double A[9], OverlapList& L) {
    L.finish(A, sc.v9, (a.out_mask && a.K > 0) ? a.out_mask + i * (size_t)a.K : nullptr);
    if (a.out_count) a.out_count[i] = L.count;
}

// one end of the query's box in the tree's frame: the FP64 difference rounded to fp32 away from the box, widened by 2^-22 of itself and
// 1e-30 more (at most / at least the exact difference whatever the rounding)
__device__ __forceinline__ float ot_wide_lo(double q, double centre) {
    const float p = __double2float_rd(q - centre);
    return (p - fabsf(p) * 2.384185791015625e-7f) - 1e-30f;
}
__device__ __forceinline__ float ot_wide_hi(double q, double centre) {
    const float p = __double2float_ru(q - centre);
    return (p + fabsf(p) * 2.384185791015625e-7f) + 1e-30f;
}
__device__ __forceinline__ bool ot_box_hit(const float lo[3], const float hi[3], float wlx, float wly, float wlz, float whx, float why, float whz) {
    return wlx <= hi[0] && lo[0] <= whx && wly <= hi[1] && lo[1] <= why && wlz <= hi[2] && lo[2] <= whz;
}

// The tree walk of the regular queries
template <bool STATS>
__global__ __launch_bounds__(256) void k_ot_walk(DevScene sc, OtArgs a) {
    const int tid = threadIdx.x;
    Stack st{reinterpret_cast<int32_t*>(lds_overlap) + tid, 256};
    unsigned int src;
    const bool live = pass_pick(a.pass, blockIdx.x * 256u + (unsigned int)tid, src);
    Ctr c = {0, 0, 0, 0};
    if (live) {
        const size_t i = (size_t)a.pass.first + (size_t)src;
        double A[9];
        ot_fetch(a.tris, i, A);
        c.rays = 1;
        OverlapList L;
        ot_rows(a, i, src, L);
        const bool any = a.any != 0;
        double qlo[3], qhi[3];
        ov_box(A, qlo, qhi);
        const float wlx = ot_wide_lo(qlo[0], sc.root.centre[0]), wly = ot_wide_lo(qlo[1], sc.root.centre[1]), wlz = ot_wide_lo(qlo[2], sc.root.centre[2]);
        const float whx = ot_wide_hi(qhi[0], sc.root.centre[0]), why = ot_wide_hi(qhi[1], sc.root.centre[1]), whz = ot_wide_hi(qhi[2], sc.root.centre[2]);
        int sp = 0;
        int32_t ni = 0, leafA = -1, leafB = -1;
        bool done = false;
        while (!done) {
            while (ni >= 0 && leafA < 0) {
                const BvhNode n = sc.bnodes[ni];
                c.nodes++;
                const bool h0 = n.n0 >= 0 && ot_box_hit(n.lo0, n.hi0, wlx, wly, wlz, whx, why, whz);
                const bool h1 = n.n1 >= 0 && ot_box_hit(n.lo1, n.hi1, wlx, wly, wlz, whx, why, whz);
                walk_step(n, h0, h1, true, st, sp, ni, leafA, leafB);       // (tree order: child 0 first)
            }
            if (leafA < 0) break;
            while (leafA >= 0 && !done) {
                const int32_t lfirst = leafA & kLeafMask, cn = (leafA >> kLeafShift) & 15;
                leafA = leafB;
                leafB = -1;
                c.leaves++;
                for (int k = 0; k < cn; ++k) {
                    const int32_t j = sc.btris[lfirst + k].aux;
                    c.geom++;
                    if (tri_overlap_mask(A, sc.v9 + (size_t)j * 9) != 0u) {
                        L.offer(j);
                        if (any) { done = true; break; }
                    }
                }
            }
        }
        ot_store(sc, a, i, A, L);
    }
    if (STATS) cp_stat_add(lds_overlap, a.stats, c);                      // (every thread of the workgroup arrives here)
}

// The per-record loop over v9 in index order: brute force (every query, input order) and the irregular tail of a SR_MODE_BVH pass.
// O(triangles) per query.
template <bool STATS>
__global__ __launch_bounds__(256) void k_ot_loop(DevScene sc, OtArgs a) {
    unsigned int src;
    const bool live = pass_pick(a.pass, blockIdx.x * 256u + threadIdx.x, src);
    Ctr c = {0, 0, 0, 0};
    if (live) {
        const size_t i = (size_t)a.pass.first + (size_t)src;
        double A[9];
        ot_fetch(a.tris, i, A);
        c.rays = 1;
        OverlapList L;
        ot_rows(a, i, src, L);
        const bool any = a.any != 0;
        for (int32_t j = 0; j < sc.ntris; ++j) {
            c.geom++;
            if (tri_overlap_mask(A, sc.v9 + (size_t)j * 9) != 0u) {
                L.offer(j);
                if (any) break;
            }
        }
        ot_store(sc, a, i, A, L);
    }
    if (STATS) cp_stat_add(lds_overlap, a.stats, c);
}

namespace {

hipError_t launch_ot_walk(const OverlapLaunch& L, const OtArgs& a) {
    const size_t lds = (size_t)stack_levels(L.sc, MODE_BVH) * 256 * 4;
    if (L.stats) hipLaunchKernelGGL((k_ot_walk<true>), lane_grid(a.pass), dim3(256), lds, L.stream, L.sc, a);
    else hipLaunchKernelGGL((k_ot_walk<false>), lane_grid(a.pass), dim3(256), lds, L.stream, L.sc, a);
    return hipGetLastError();
}

hipError_t launch_ot_loop(const OverlapLaunch& L, const OtArgs& a) {
    if (L.stats) hipLaunchKernelGGL((k_ot_loop<true>), lane_grid(a.pass), dim3(256), 16, L.stream, L.sc, a);    // (cp_stat_add's four words)
    else hipLaunchKernelGGL((k_ot_loop<false>), lane_grid(a.pass), dim3(256), 0, L.stream, L.sc, a);
    return hipGetLastError();
}

// the order of a pass (cp_order's, on the queries' box centres): the regular queries first -- sorted: by Morton cell, ties in input order;
// !sorted: in input order -- then the others
hipError_t ot_order(const BatchLaunch& L, const RootBox& root, const double* tris, unsigned int n, const PassBuffers& b) {
    const bool sorted = !L.input_order;
    double s[3];
    for (int k = 0; k < 3; ++k) { const double e = root.max[k] - root.min[k]; s[k] = e > 0 ? 128.0 / e : 0.0; }
    const unsigned int skip = point_order_skip_mask(sorted);
    int end_bit = 0;
    while ((skip >> end_bit) != 0u) ++end_bit;                            // the skip bit is the key's highest
    hipLaunchKernelGGL(k_ot_keys, dim3((n + 255u) / 256u), dim3(256), 0, L.stream, tris, n, sorted ? 1 : 0, skip, root.min[0], root.min[1], root.min[2], s[0], s[1],
                       s[2], root.centre[0], root.centre[1], root.centre[2], closest_diag(root.min, root.max), b.keys, b.idx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t temp_bytes = L.sort_temp_bytes;
    return hipcub::DeviceRadixSort::SortPairs(L.sort_temp, temp_bytes, (const unsigned int*)b.keys, b.keys2, (const unsigned int*)b.idx, b.order, (int)n, 0, end_bit,
                                              L.stream);
}

}  // namespace

// SR_MODE_BVH: a pass is ordered first (ot_order), the regular queries walk the tree, the tail runs the per-record loop (loop_all: every
// query does).  SR_MODE_BRUTE: the per-record loop in input order
hipError_t launch_overlap(const OverlapLaunch& L) {
    if (L.n <= 0) return hipSuccess;
    if (L.pass <= 0 || L.pass > kBatchMaxPass || L.max_hits < 0 || L.max_hits > kAllHitsMax) return hipErrorInvalidValue;
    if (L.mode != MODE_BVH && L.mode != MODE_BRUTE) return hipErrorInvalidValue;
    if (L.mode == MODE_BVH && stack_levels(L.sc, MODE_BVH) * 256 * 4 > 65536) return hipErrorInvalidValue;
    if (L.any && L.max_hits != 0) return hipErrorInvalidValue;
    OtArgs a{};
    a.tris = L.tris;
    a.K = (L.index || L.mask) ? L.max_hits : 0;                           // (nobody reads a row: the counting call)
    a.any = L.any ? 1 : 0;
    if (a.K > 0 && !L.index && !L.scratch_index) return hipErrorInvalidValue;
    a.out_count = L.count; a.out_index = L.index; a.out_mask = L.mask;
    a.s_index = L.scratch_index;
    a.stats = L.stats;
    return run_passes(
        L, L.mode == MODE_BVH, K_OVERLAP_SORT, K_OVERLAP,
        [&](int64_t first, unsigned int count, const PassBuffers& b) { return ot_order(L, L.sc.root, L.tris + 9 * first, count, b); },
        [&](const PassSlice& p, const PassBuffers&) {
            a.pass = p;
            if (L.mode != MODE_BVH || L.loop_all) return launch_ot_loop(L, a);
            a.pass.take = 0;
            const hipError_t e = launch_ot_walk(L, a);
            a.pass.take = 1;
            return e != hipSuccess ? e : launch_ot_loop(L, a);
        });
}

}  // namespace sr
