// sr_near.hip -- sr_near_triangles: the triangles within reach of a point, nearest first, with a count, for a batch of points (gfx950).
//
// For point q and triangle j, c_j, (v, w) and d2_j are sr_closest_points' values (closest_point_triangle and closest_d2, sr_closest.h, on the
// FP64 vertices v9[j]).  The set of q is every j whose d2_j is a number and, where there are limits, sqrt(d2_j) <= limit; count = its size,
// the row = its first min(count, K) members by (d2_j, j).  The list is sr_near_list.h's (one text for these kernels and the host check).
// A REGULAR point (closest_regular) walks the own BVH in k_cp_walk's frame (sr_closest.hip): one lane per point, a while-while walk that
// prunes by cp_bound, the fp32 LOWER bound of the squared distance to a child's box, nearer child first, the stack word carrying the bound
// that a pop re-tests.  Every other point of a pass, and every point of brute force, runs the per-record loop over v9 in index order.
// The cull: a box is skipped only when its bound strictly exceeds cp_cullf(min(lim2, kcut)) -- lim2 the inflated squared limit
// of k_cp_walk; kcut = +inf while the row is not full or the caller wants the count, otherwise max(worst kept d2, least trusted d2 seen).
// The limit per candidate is the exact test fl(sqrt(d2)) <= limit, reduced to d2 <= near_threshold(limit), found once per point.
// The pass driver and the lane's pick are sr_batch.h's, the keys and the sort of a pass are sr_closest.hip's (cp_order).
#include "sr_batch.h"
#include "sr_near_list.h"

namespace sr {

extern __shared__ __attribute__((aligned(16))) unsigned char lds_near[];

struct NtArgs {
    const double* points; const double* limits;
    PassSlice pass;
    int K, cull_k;
    uint32_t* out_count;         // [n] or nullptr
    int32_t*  out_index;         // [n][K] or nullptr: then the rows of s_index, [pass][K]
    double*   out_dist;          // [n][K] or nullptr: then the rows of s_dist
    double*   out_pos;           // [n][K][3] or nullptr
    double*   out_uv;            // [n][K][2] or nullptr
    int32_t*  s_index; double* s_dist;
    unsigned long long* stats;
};

__device__ __forceinline__ void nt_rows(const NtArgs& a, size_t i, unsigned int src, NearList& L) {
    int32_t* ir = nullptr;
    double* kr = nullptr;
    if (a.K > 0) {
        ir = a.out_index ? a.out_index + i * (size_t)a.K : a.s_index + (size_t)src * (size_t)a.K;
        kr = a.out_dist ? a.out_dist + i * (size_t)a.K : a.s_dist + (size_t)src * (size_t)a.K;
    }
    L.init(ir, kr, a.K);
}
// the end of a point: the sorted row, its distances, positions and weights, the count
__device__ __forceinline__ void nt_store(const DevScene& sc, const NtArgs& a, size_t i, const double q[3], NearList& L) {
    L.finish(q, sc.v9, (a.out_pos && a.K > 0) ? a.out_pos + i * (size_t)a.K * 3 : nullptr, (a.out_uv && a.K > 0) ? a.out_uv + i * (size_t)a.K * 2 : nullptr);
    if (a.out_count) a.out_count[i] = L.count;
}

// The tree walk of the regular points: k_cp_walk's frame with the list in place of the running best.
template <bool STATS>
__global__ __launch_bounds__(256) void k_nt_walk(DevScene sc, NtArgs a) {
    const int tid = threadIdx.x;
    Stack st{reinterpret_cast<int32_t*>(lds_near) + tid, 256};
    unsigned int src;
    const bool live = pass_pick(a.pass, blockIdx.x * 256u + (unsigned int)tid, src);
    Ctr c = {0, 0, 0, 0};
    if (live) {
        const size_t i = (size_t)a.pass.first + (size_t)src;
        const double q[3] = {a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]};
        const bool no_lim = a.limits == nullptr;
        const double lim = no_lim ? (double)INFINITY : a.limits[i];
        const double thr = near_threshold(lim);                            // d2 <= thr <=> fl(sqrt(d2)) <= lim
        // d2 > lim2 implies sqrt(d2) > lim (k_cp_walk's bound).  A NaN limit gives NaN: fmin ignores it (no cull; nothing is admitted)
        const double lim2 = (lim * lim) * (1.0 + 3.552713678800501e-15);
        const bool cull_k = a.cull_k != 0;
        c.rays = 1;
        NearList L;
        nt_rows(a, i, src, L);
        double trusted = (double)INFINITY;                                 // the least d2 whose point lies in its triangle
        float cullf = cp_cullf(fmin((double)INFINITY, lim2));
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
                    ni = -1;                                              // a popped node is re-tested against the bound as it is now
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
                    bool moved = false;
                    if (d2 == d2 && (no_lim || d2 <= thr)) moved = L.offer(d2, j);
                    // only a point inside its triangle may tighten the cull (the face region of a sliver can place it anywhere)
                    if (v >= 0.0 && w >= 0.0 && v + w <= 1.0 + 0x1p-40 && d2 < trusted) { trusted = d2; moved = true; }
                    if (cull_k && moved && L.full()) cullf = cp_cullf(fmin(fmax(L.wkey, trusted), lim2));
                }
            }
        }
        nt_store(sc, a, i, q, L);
    }
    if (STATS) cp_stat_add(lds_near, a.stats, c);                         // (every thread of the workgroup arrives here)
}

// The per-record loop over v9 in index order: brute force (every point, input order) and the irregular tail of a SR_MODE_BVH pass.
// O(triangles) per point.
template <bool STATS>
__global__ __launch_bounds__(256) void k_nt_loop(DevScene sc, NtArgs a) {
    unsigned int src;
    const bool live = pass_pick(a.pass, blockIdx.x * 256u + threadIdx.x, src);
    Ctr c = {0, 0, 0, 0};
    if (live) {
        const size_t i = (size_t)a.pass.first + (size_t)src;
        const double q[3] = {a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]};
        const bool no_lim = a.limits == nullptr;
        const double thr = near_threshold(no_lim ? (double)INFINITY : a.limits[i]);
        c.rays = 1;
        NearList L;
        nt_rows(a, i, src, L);
        for (int32_t j = 0; j < sc.ntris; ++j) {
            double cc[3], v, w;
            c.geom++;
            closest_point_triangle(q, sc.v9 + (size_t)j * 9, cc, v, w);
            const double d2 = closest_d2(q, cc);
            if (d2 == d2 && (no_lim || d2 <= thr)) L.offer(d2, j);
        }
        nt_store(sc, a, i, q, L);
    }
    if (STATS) cp_stat_add(lds_near, a.stats, c);
}

namespace {

hipError_t launch_nt_walk(const NearLaunch& L, const NtArgs& a) {
    const size_t lds = (size_t)stack_levels(L.sc, MODE_BVH) * 256 * 4;
    if (L.stats) hipLaunchKernelGGL((k_nt_walk<true>), lane_grid(a.pass), dim3(256), lds, L.stream, L.sc, a);
    else hipLaunchKernelGGL((k_nt_walk<false>), lane_grid(a.pass), dim3(256), lds, L.stream, L.sc, a);
    return hipGetLastError();
}

hipError_t launch_nt_loop(const NearLaunch& L, const NtArgs& a) {
    if (L.stats) hipLaunchKernelGGL((k_nt_loop<true>), lane_grid(a.pass), dim3(256), 16, L.stream, L.sc, a);    // (cp_stat_add's four words)
    else hipLaunchKernelGGL((k_nt_loop<false>), lane_grid(a.pass), dim3(256), 0, L.stream, L.sc, a);
    return hipGetLastError();
}

}  // namespace

// SR_MODE_BVH: a pass is ordered first (cp_order), the regular points walk the tree, the tail runs the per-record loop (loop_all: every
// point does).  SR_MODE_BRUTE: the per-record loop in input order
hipError_t launch_near(const NearLaunch& L) {
    if (L.n <= 0) return hipSuccess;
    if (L.pass <= 0 || L.pass > kBatchMaxPass || L.max_hits < 0 || L.max_hits > kAllHitsMax) return hipErrorInvalidValue;
    if (L.mode != MODE_BVH && L.mode != MODE_BRUTE) return hipErrorInvalidValue;
    if (L.mode == MODE_BVH && stack_levels(L.sc, MODE_BVH) * 256 * 4 > 65536) return hipErrorInvalidValue;
    if (L.max_hits > 0 && ((!L.index && !L.scratch_index) || (!L.dist && !L.scratch_dist))) return hipErrorInvalidValue;
    NtArgs a{};
    a.points = L.points; a.limits = L.limits;
    a.K = L.max_hits; a.cull_k = (!L.count && L.max_hits > 0) ? 1 : 0;
    a.out_count = L.count; a.out_index = L.index; a.out_dist = L.dist; a.out_pos = L.pos; a.out_uv = L.uv;
    a.s_index = L.scratch_index; a.s_dist = L.scratch_dist;
    a.stats = L.stats;
    return run_passes(
        L, L.mode == MODE_BVH, K_NEAR_SORT, K_NEAR,
        [&](int64_t first, unsigned int count, const PassBuffers& b) { return cp_order(L, L.sc.root, L.points + 3 * first, count, b); },
        [&](const PassSlice& p, const PassBuffers&) {
            a.pass = p;
            if (L.mode != MODE_BVH || L.loop_all) return launch_nt_loop(L, a);
            a.pass.take = 0;
            const hipError_t e = launch_nt_walk(L, a);
            a.pass.take = 1;
            return e != hipSuccess ? e : launch_nt_loop(L, a);
        });
}

}  // namespace sr
