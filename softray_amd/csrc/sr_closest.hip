// sr_closest.hip -- sr_closest_points: the nearest point of the mesh, its triangle and its distance, for a batch of points (gfx950).
//
// The answer for q is the triangle j that minimises (d2_j, j) over every triangle whose d2_j is a number, with c_j = closest_point_triangle
// (sr_closest.h) on the FP64 vertices v9[j] and d2_j = closest_d2(q, c_j); it qualifies iff there is no limit or sqrt(d2_j) <= limit.
// A REGULAR point (closest_regular) walks the own BVH: one lane per point, a while-while walk in k_ah_walk's frame that prunes by an fp32
// LOWER bound of the squared distance to a child's box instead of a ray's slab interval, nearer child first.  Every other point of a pass,
// and every point of brute force, runs the per-record loop over v9 in index order with the same FP64 routine and no fp32 stage.
// The cull is exact: a box is skipped only when its deflated bound strictly exceeds the best squared distance found so far
// (or the squared limit, inflated), so a triangle that ties the answer with a lower index is always visited.
// The pass driver and the lane's pick are sr_batch.h's, shared with the other batch calls, and so are the bound, its cull value and the
// statistics epilogue, shared with sr_near.hip; the keys and the sort of a pass (cp_order, which sr_near.hip calls too), the walk's node
// step (its stack word carries a bound that a pop re-tests; sharing the leaf half cost the lattice 0.5 %: profiles/batch_refactor) and the
// two kernels are this file's.
#include <hipcub/hipcub.hpp>

#include "sr_batch.h"
#include "sr_closest.h"

namespace sr {

extern __shared__ __attribute__((aligned(16))) unsigned char lds_closest[];

__device__ __forceinline__ unsigned int cp_spread7(unsigned int v) {       // 7 bits -> every third bit (k_ray_keys' spread)
    v &= 0x7fu;
    v = (v | (v << 8)) & 0x700fu;
    v = (v | (v << 4)) & 0x430c3u;
    v = (v | (v << 2)) & 0x49249u;
    return v;
}

// Key of a pass's point: the 7-bit Morton cell of the point in the root box (points outside clamp to the edge cells), 21 bits; `skip`
// (point_order_skip_mask) marks an IRREGULAR point, which the walk never sees: the stable sort leaves those at the end of the pass in input
// order.  !sorted: the key is that bit alone (a deterministic compaction that keeps the input order).
__global__ __launch_bounds__(256) void k_cp_keys(const double* __restrict__ points, unsigned int n, int sorted, unsigned int skip, double lx, double ly,
                                                 double lz, double sx, double sy, double sz, double cx, double cy, double cz, double diag,
                                                 unsigned int* __restrict__ keys, unsigned int* __restrict__ idx) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double q[3] = {points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2]};
    const double centre[3] = {cx, cy, cz};
    unsigned int key = 0u;
    if (!closest_regular(q, centre, diag)) key = skip;
    else if (sorted) {
        const int kx = (int)fmin(127.0, fmax(0.0, (q[0] - lx) * sx)), ky = (int)fmin(127.0, fmax(0.0, (q[1] - ly) * sy)), kz = (int)fmin(127.0, fmax(0.0, (q[2] - lz) * sz));
        key = (cp_spread7((unsigned)kx) << 2) | (cp_spread7((unsigned)ky) << 1) | cp_spread7((unsigned)kz);
    }
    keys[i] = key;
    idx[i] = i;
}

struct CpArgs {
    const double* points; const double* limits;
    PassSlice pass;
    int32_t* out_tri; double* out_dist; double* out_pos; double* out_uv;
    unsigned long long* stats;
};

// The answer of point i once the best triangle is known: the routine runs once more for the winner (the loops keep (d2, j) only), the limit
// is applied to the rounded square root, a point without a qualifying answer gets -1 and zeros
__device__ __forceinline__ void cp_store(const DevScene& sc, const CpArgs& a, size_t i, const double q[3], int32_t bj, bool no_lim, double lim) {
    double c[3] = {0.0, 0.0, 0.0}, v = 0.0, w = 0.0, dist = 0.0;
    int32_t tri = -1;
    if (bj != INT32_MAX) {
        double cc[3], vv, ww;
        closest_point_triangle(q, sc.v9 + (size_t)bj * 9, cc, vv, ww);
        const double d = sqrt(closest_d2(q, cc));
        if (no_lim || d <= lim) { tri = bj; dist = d; c[0] = cc[0]; c[1] = cc[1]; c[2] = cc[2]; v = vv; w = ww; }
    }
    if (a.out_tri) a.out_tri[i] = tri;
    if (a.out_dist) a.out_dist[i] = dist;
    if (a.out_pos) { a.out_pos[3 * i] = c[0]; a.out_pos[3 * i + 1] = c[1]; a.out_pos[3 * i + 2] = c[2]; }
    if (a.out_uv) { a.out_uv[2 * i] = v; a.out_uv[2 * i + 1] = w; }
}

// The tree walk of the regular points.  Stack word = node | the bound's float bits with their low bnode_bits cleared (a lower bound still),
// one word per level per lane in LDS.
template <bool STATS>
__global__ __launch_bounds__(256) void k_cp_walk(DevScene sc, CpArgs a) {
    const int tid = threadIdx.x;
    Stack st{reinterpret_cast<int32_t*>(lds_closest) + tid, 256};
    unsigned int src;
    const bool live = pass_pick(a.pass, blockIdx.x * 256u + (unsigned int)tid, src);
    Ctr c = {0, 0, 0, 0};
    if (live) {
        const size_t i = (size_t)a.pass.first + (size_t)src;
        const double q[3] = {a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]};
        const bool no_lim = a.limits == nullptr;
        const double lim = no_lim ? (double)INFINITY : a.limits[i];
        // d2 > lim2 implies sqrt(d2) > lim: fl(lim lim) (1 + 2^-48) >= lim^2 (1 + 2^-49).  A NaN limit gives NaN: fmin ignores it (no cull)
        const double lim2 = (lim * lim) * (1.0 + 3.552713678800501e-15);
        c.rays = 1;
        double best = (double)INFINITY, trusted = (double)INFINITY;        // the answer's d2; the least d2 whose point lies in its triangle
        int32_t bj = INT32_MAX;
        float cullf = cp_cullf(fmin(trusted, lim2));
        const float px = (float)(q[0] - sc.root.centre[0]), py = (float)(q[1] - sc.root.centre[1]), pz = (float)(q[2] - sc.root.centre[2]);
        const float ex = fabsf(px) * 1.1920928955078125e-7f, ey = fabsf(py) * 1.1920928955078125e-7f, ez = fabsf(pz) * 1.1920928955078125e-7f;
        const int nbits = sc.bnode_bits;
        const uint32_t nmask = (1u << nbits) - 1u;
        int sp = 0;
        int32_t ni = 0, leafA = -1, leafB = -1;
        float boundB = 0.0f;
        for (;;) {
            while (ni >= 0 && leafA < 0) {
                const BvhNode n = sc.bnodes[ni];
                c.nodes++;
                const float b0 = cp_bound(n.lo0, n.hi0, px, py, pz, ex, ey, ez), b1 = cp_bound(n.lo1, n.hi1, px, py, pz, ex, ey, ez);
                const bool h0 = n.n0 >= 0 && !(b0 > cullf), h1 = n.n1 >= 0 && !(b1 > cullf);
                const bool first0 = b0 <= b1;                             // nearer child first
                const bool l0 = h0 && n.n0 > 0, l1 = h1 && n.n1 > 0;
                if (l0 && l1) {
                    leafA = (first0 ? n.c0 : n.c1) | ((first0 ? n.n0 : n.n1) << kLeafShift);
                    leafB = (first0 ? n.c1 : n.c0) | ((first0 ? n.n1 : n.n0) << kLeafShift);
                    boundB = first0 ? b1 : b0;
                } else if (l0) leafA = n.c0 | (n.n0 << kLeafShift);
                else if (l1) leafA = n.c1 | (n.n1 << kLeafShift);
                const bool i0 = h0 && n.n0 == 0, i1 = h1 && n.n1 == 0;
                if (i0 && i1) {
                    const uint32_t far_bits = __float_as_uint(first0 ? b1 : b0) & ~nmask;
                    st.put(sp++, (int32_t)(far_bits | (uint32_t)(first0 ? n.c1 : n.c0)));
                    ni = first0 ? n.c0 : n.c1;
                } else if (i0) ni = n.c0;
                else if (i1) ni = n.c1;
                else {
                    ni = -1;                                              // a popped node is re-tested against the best found since it was pushed
                    while (sp > 0) {
                        const uint32_t word = (uint32_t)st.get(--sp);
                        if (!(__uint_as_float(word & ~nmask) > cullf)) { ni = (int32_t)(word & nmask); break; }
                    }
                }
            }
            if (leafA < 0) break;
            while (leafA >= 0) {
                const int32_t lfirst = leafA & kLeafMask, cn = (leafA >> kLeafShift) & 15;
                leafA = (leafB >= 0 && !(boundB > cullf)) ? leafB : -1;
                leafB = -1;
                c.leaves++;
                for (int k = 0; k < cn; ++k) {
                    const int32_t j = sc.btris[lfirst + k].aux;
                    double cc[3], v, w;
                    c.geom++;
                    closest_point_triangle(q, sc.v9 + (size_t)j * 9, cc, v, w);
                    const double d2 = closest_d2(q, cc);
                    if (cp_better(d2, j, best, bj)) { best = d2; bj = j; }
                    // only a point inside its triangle may tighten the cull (the face region of a sliver can place it anywhere)
                    if (v >= 0.0 && w >= 0.0 && v + w <= 1.0 + 0x1p-40 && d2 < trusted) {
                        trusted = d2;
                        cullf = cp_cullf(fmin(trusted, lim2));
                    }
                }
            }
        }
        cp_store(sc, a, i, q, bj, no_lim, lim);
    }
    if (STATS) cp_stat_add(lds_closest, a.stats, c);                      // (every thread of the workgroup arrives here)
}

// The per-record loop over v9 in index order: brute force (every point, input order) and the irregular tail of a SR_MODE_BVH pass.
// O(triangles) per point.
template <bool STATS>
__global__ __launch_bounds__(256) void k_cp_loop(DevScene sc, CpArgs a) {
    unsigned int src;
    const bool live = pass_pick(a.pass, blockIdx.x * 256u + threadIdx.x, src);
    Ctr c = {0, 0, 0, 0};
    if (live) {
        const size_t i = (size_t)a.pass.first + (size_t)src;
        const double q[3] = {a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]};
        const bool no_lim = a.limits == nullptr;
        const double lim = no_lim ? (double)INFINITY : a.limits[i];
        c.rays = 1;
        double best = (double)INFINITY;
        int32_t bj = INT32_MAX;
        for (int32_t j = 0; j < sc.ntris; ++j) {
            double cc[3], v, w;
            c.geom++;
            closest_point_triangle(q, sc.v9 + (size_t)j * 9, cc, v, w);
            const double d2 = closest_d2(q, cc);
            if (cp_better(d2, j, best, bj)) { best = d2; bj = j; }
        }
        cp_store(sc, a, i, q, bj, no_lim, lim);
    }
    if (STATS) cp_stat_add(lds_closest, a.stats, c);
}

namespace {

hipError_t launch_cp_walk(const ClosestLaunch& L, const CpArgs& a) {
    const size_t lds = (size_t)stack_levels(L.sc, MODE_BVH) * 256 * 4;
    if (L.stats) hipLaunchKernelGGL((k_cp_walk<true>), lane_grid(a.pass), dim3(256), lds, L.stream, L.sc, a);
    else hipLaunchKernelGGL((k_cp_walk<false>), lane_grid(a.pass), dim3(256), lds, L.stream, L.sc, a);
    return hipGetLastError();
}

hipError_t launch_cp_loop(const ClosestLaunch& L, const CpArgs& a) {
    if (L.stats) hipLaunchKernelGGL((k_cp_loop<true>), lane_grid(a.pass), dim3(256), 16, L.stream, L.sc, a);    // (cp_stat_add's four words)
    else hipLaunchKernelGGL((k_cp_loop<false>), lane_grid(a.pass), dim3(256), 0, L.stream, L.sc, a);
    return hipGetLastError();
}

}  // namespace

// (sr_batch.h) the order of a pass: the regular points first -- sorted: by Morton cell, ties in input order; !sorted: in input order -- then the others
hipError_t cp_order(const BatchLaunch& L, const RootBox& root, const double* points, unsigned int n, const PassBuffers& b) {
    const bool sorted = !L.input_order;
    double s[3];
    for (int k = 0; k < 3; ++k) { const double e = root.max[k] - root.min[k]; s[k] = e > 0 ? 128.0 / e : 0.0; }
    const unsigned int skip = point_order_skip_mask(sorted);
    int end_bit = 0;
    while ((skip >> end_bit) != 0u) ++end_bit;                            // the skip bit is the key's highest
    hipLaunchKernelGGL(k_cp_keys, dim3((n + 255u) / 256u), dim3(256), 0, L.stream, points, n, sorted ? 1 : 0, skip, root.min[0], root.min[1], root.min[2], s[0],
                       s[1], s[2], root.centre[0], root.centre[1], root.centre[2], closest_diag(root.min, root.max), b.keys, b.idx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t temp_bytes = L.sort_temp_bytes;
    return hipcub::DeviceRadixSort::SortPairs(L.sort_temp, temp_bytes, (const unsigned int*)b.keys, b.keys2, (const unsigned int*)b.idx, b.order, (int)n, 0, end_bit,
                                              L.stream);
}

// SR_MODE_BVH: a pass is ordered first, the regular points walk the tree, the tail runs the per-record loop (loop_all: every point does).
// SR_MODE_BRUTE: the per-record loop in input order
hipError_t launch_closest(const ClosestLaunch& L) {
    if (L.n <= 0) return hipSuccess;
    if (L.pass <= 0 || L.pass > kBatchMaxPass) return hipErrorInvalidValue;
    if (L.mode != MODE_BVH && L.mode != MODE_BRUTE) return hipErrorInvalidValue;
    if (L.mode == MODE_BVH && stack_levels(L.sc, MODE_BVH) * 256 * 4 > 65536) return hipErrorInvalidValue;
    CpArgs a{};
    a.points = L.points; a.limits = L.limits;
    a.out_tri = L.tri; a.out_dist = L.dist; a.out_pos = L.pos; a.out_uv = L.uv;
    a.stats = L.stats;
    return run_passes(
        L, L.mode == MODE_BVH, K_CLOSEST_SORT, K_CLOSEST,
        [&](int64_t first, unsigned int count, const PassBuffers& b) { return cp_order(L, L.sc.root, L.points + 3 * first, count, b); },
        [&](const PassSlice& p, const PassBuffers&) {
            a.pass = p;
            if (L.mode != MODE_BVH || L.loop_all) return launch_cp_loop(L, a);
            a.pass.take = 0;
            const hipError_t e = launch_cp_walk(L, a);
            a.pass.take = 1;
            return e != hipSuccess ? e : launch_cp_loop(L, a);
        });
}

}  // namespace sr
