// sr_allhits.hip -- sr_all_hits_rays: every hit along a ray, nearest first, with a count, for a batch of arbitrary rays (gfx950).
//
// The hit set of a ray on the own BVH is every record that passes the per-record test of bvh_intersect (sr_trace.h): the start clipped to the
// root box, offset = |original - s| / |d|, tri_hit && inside(root box), ray_frac = fl(t + offset); in brute force the per-record loop of
// GeometryCollection (unclipped start, ray_frac = t).  A hit qualifies iff ray_frac <= limit (IEEE <=).  count = the qualifying hits, the row
// = the first min(count, K) of them by (ray_frac, extra elements before triangles, element / TriangleIndex).
// A REGULAR ray (occl_order, sr_device.h) walks the tree -- bvh_intersect<false>'s while-while walk without the early exit -- every other ray
// of the own BVH and every ray of brute force runs the per-record loop with the same FP64 predicate and no fp32 stage.
// The list of a ray lives in the lane's own ROW of memory (the caller's index / ray_frac rows, or rows of the scene's scratch where the
// caller passed NULL): the fill count and the worst kept key stay in registers, no array is indexed in private memory.
// The pass driver, the lane's pick, the ray fetch and the walk's ray frame and node step are sr_batch.h's, shared with the other batch calls;
// the list, the cull at the K-th hit, the two kernels and the walk / loop split of a pass are this file's.
#include "sr_batch.h"

namespace sr {

extern __shared__ __attribute__((aligned(16))) unsigned char lds_allhits[];

// the order's second key from a reported index: extra element e (index -2 - e) -> e, TriangleIndex j -> 2^31 + j
__device__ __forceinline__ uint32_t ah_sec(int32_t index) { return index >= 0 ? (0x80000000u | (uint32_t)index) : (uint32_t)(-2 - index); }
// (a NaN ray_frac -- possible only without limits, for an irregular ray whose offset is 0 / 0 -- sorts behind every number)
__device__ __forceinline__ bool ah_precedes(double fa, uint32_t sa, double fb, uint32_t sb) {
    const bool na = fa != fa, nb = fb != fb;
    if (na || nb) return nb && (!na || sa < sb);
    return fa < fb || (fa == fb && sa < sb);
}

// One lane's list.  K slots per row; every slot index used below is < K: `fill` only grows while fill < K, `wslot` is either a former `fill`
// or comes out of a scan over [0, K).
struct AhList {
    int32_t* idx;        // the lane's rows (K == 0: never dereferenced)
    double*  frac;
    int      K, fill, wslot;
    double   wfrac;      // the worst kept key (valid when fill > 0)
    uint32_t wsec;
    uint32_t count;      // every qualifying hit, kept or not

    __device__ __forceinline__ void init(int32_t* idx_row, double* frac_row, int k) {
        idx = idx_row; frac = frac_row; K = k; fill = 0; wslot = 0; wfrac = 0.0; wsec = 0u; count = 0u;
    }
    __device__ __forceinline__ bool full() const { return fill >= K; }
    // a qualifying hit.  Returns true when the worst kept key changed while the row is full (the caller's cull bound follows it)
    __device__ __forceinline__ bool offer(double f, int32_t index) {
        count++;
        if (K <= 0) return false;
        const uint32_t sec = ah_sec(index);
        if (fill < K) {
            idx[fill] = index; frac[fill] = f;
            if (fill == 0 || !ah_precedes(f, sec, wfrac, wsec)) { wfrac = f; wsec = sec; wslot = fill; }
            fill++;
            return fill == K;
        }
        if (!ah_precedes(f, sec, wfrac, wsec)) return false;
        idx[wslot] = index; frac[wslot] = f;                 // displaces the worst; one rescan of the K slots finds the new worst
        int ws = 0;
        double wf = frac[0];
        uint32_t wq = ah_sec(idx[0]);
        for (int q = 1; q < K; ++q) {
            const double fq = frac[q];
            const uint32_t sq = ah_sec(idx[q]);
            if (ah_precedes(wf, wq, fq, sq)) { wf = fq; wq = sq; ws = q; }
        }
        wslot = ws; wfrac = wf; wsec = wq;
        return true;
    }
    // sort the kept entries (insertion sort, K <= 64), pad the rest of the row
    __device__ __forceinline__ void finish() {
        for (int a = 1; a < fill; ++a) {
            const double f = frac[a];
            const int32_t ix = idx[a];
            const uint32_t sec = ah_sec(ix);
            int b = a - 1;
            while (b >= 0) {
                const double fb = frac[b];
                const int32_t ib = idx[b];
                if (!ah_precedes(f, sec, fb, ah_sec(ib))) break;
                frac[b + 1] = fb; idx[b + 1] = ib;           // (b + 1 <= a < fill <= K)
                --b;
            }
            frac[b + 1] = f; idx[b + 1] = ix;
        }
        for (int q = fill; q < K; ++q) { idx[q] = -1; frac[q] = 0.0; }
    }
};

// the fp32 cull bound of a walk from an FP64 bound on ray_frac: as bvh_intersect<true> derives tlim from a limit, with the FP64 room widened
// by 2^-51 (bound + offset) first -- fl(t + offset) == bound is possible for a t up to half an ulp of the sum beyond bound - offset, and the
// subtraction rounds too; where offset is large against bound - offset the 2^-20 inflation of the fp32 value does not cover that
__device__ __forceinline__ float ah_tlim(double bound, double offset) {
    const double room = (bound - offset) + (fabs(bound) + offset) * 4.440892098500626e-16;
    if (!(room < 3.0e38)) return FLT_MAX;                    // (+inf, 1e300: no bound)
    return cull_tlim(room);
}

struct AhArgs {
    BatchRays rays;
    PassSlice pass;
    int K, cull_k;
    uint32_t* out_count;         // [n] or nullptr
    int32_t*  out_index;         // [n][K] or nullptr: then the rows of s_index, [pass][K]
    double*   out_frac;          // [n][K] or nullptr: then the rows of s_frac
    int32_t*  s_index; double* s_frac;
    unsigned long long* stats;
};

__device__ __forceinline__ void ah_rows(const AhArgs& a, size_t i, unsigned int src, AhList& L) {
    int32_t* ir = nullptr;
    double* fr = nullptr;
    if (a.K > 0) {
        ir = a.out_index ? a.out_index + i * (size_t)a.K : a.s_index + (size_t)src * (size_t)a.K;
        fr = a.out_frac ? a.out_frac + i * (size_t)a.K : a.s_frac + (size_t)src * (size_t)a.K;
    }
    L.init(ir, fr, a.K);
}
// the extra geometry: every element's own IntersectRay answer from the unclipped start (a rayFrac of DBL_MAX or more does not count)
__device__ __forceinline__ void ah_extra(const DevScene& sc, D3 s, D3 d, bool no_lim, double lim, AhList& L, Ctr& c) {
    for (int k = 0; k < sc.nextra; ++k) {
        double t; D3 pos, nrm;
        uint32_t tests;
        const bool ok = extra_hit(&sc.extra[k], s, d, t, pos, nrm, tests);
        c.geom += tests;
        if (ok && t < DBL_MAX && (no_lim || t <= lim)) L.offer(t, -2 - k);
    }
}

// The tree walk of the regular rays: bvh_intersect<false>'s frame (per-lane while-while walk, LDS stack, leaf_survivors before the FP64
// record) with no early exit.  The boxes are culled at the limit, or -- cull_k: the caller wants no count -- at the K-th kept hit once the row
// is full: a hit beyond fl(t + offset) = worst.ray_frac can neither enter the row nor, without `count`, be observed.
template <bool EXTRA, bool STATS>
__global__ __launch_bounds__(256) void k_ah_walk(DevScene sc, AhArgs a) {
    const int tid = threadIdx.x;
    Stack st{reinterpret_cast<int32_t*>(lds_allhits) + tid, 256};
    unsigned int src;
    const bool live = pass_pick(a.pass, blockIdx.x * 256u + (unsigned int)tid, src);
    Ctr c = {0, 0, 0, 0};
    if (live) {
        const size_t i = (size_t)a.pass.first + (size_t)src;
        D3 s, d;
        double lim;
        fetch_ray(a.rays, i, (double)INFINITY, s, d, lim);
        const bool no_lim = a.rays.limits == nullptr;                     // no limit: no comparison is made (a NaN ray_frac counts)
        c.rays = 1;
        AhList L;
        ah_rows(a, i, src, L);
        if (EXTRA) ah_extra(sc, s, d, no_lim, lim, L, c);
        D3 end = s + d * 10000.0;
        const D3 original = s;
        bool walk = clip_segment<false>(sc.root, s, end);
        double offset = 0.0;
        if (walk) {
            offset = length(original - s) / length(d);
            walk = !(lim - offset < 0.0);
        }
        if (walk) {
            const bool cull_k = a.cull_k != 0 && a.K > 0;
            float tlim = ah_tlim((cull_k && L.full()) ? fmin(lim, L.wfrac) : lim, offset);
            SlabRay ray;
            set_slab_ray(sc, s, d, ray);
            int sp = 0;
            int32_t ni = 0, leafA = -1, leafB = -1;
            for (;;) {
                while (ni >= 0 && leafA < 0) {
                    const BvhNode n = sc.bnodes[ni];
                    c.nodes++;
                    bool h0, h1, first0;
                    ray_node_hits(n, ray, tlim, h0, h1, first0);
                    walk_step(n, h0, h1, first0, st, sp, ni, leafA, leafB);
                }
                if (leafA < 0) break;
                while (leafA >= 0) {
                    const int32_t lfirst = leafA & kLeafMask, cn = (leafA >> kLeafShift) & 15;
                    leafA = leafB;
                    leafB = -1;
                    c.leaves++;
                    for (uint32_t m = leaf_survivors(sc, lfirst, cn, ray.rf, tlim); m; m &= m - 1u) {
                        const Rec128* r = &sc.btris[lfirst + (__ffs((int)m) - 1)];
                        double t; D3 pos;
                        c.geom++;
                        if (tri_hit(r->p, s, d, t, pos) && inside(sc.root.lo, sc.root.hi, pos)) {
                            const double f = t + offset;
                            if ((no_lim || f <= lim) && L.offer(f, r->aux) && cull_k) tlim = ah_tlim(fmin(lim, L.wfrac), offset);
                        }
                    }
                }
            }
        }
        L.finish();
        if (a.out_count) a.out_count[i] = L.count;
    }
    if (STATS) block_stat_add(a.stats, c);                            // (every thread of the workgroup arrives here)
}

// The per-record loop.  CLIP = false, brute force: GeometryCollection's loop, tri_hit from the unclipped start, ray_frac = t, no box test.
// CLIP = true, the irregular rays of the own BVH: bvh_intersect's per-record predicate over every record of the model, no fp32 stage -- a
// zero, NaN or infinite direction only ever fails FP64 comparisons.  O(triangles) per ray.
template <bool CLIP, bool EXTRA, bool STATS>
__global__ __launch_bounds__(256) void k_ah_loop(DevScene sc, AhArgs a) {
    unsigned int src;
    const bool live = pass_pick(a.pass, blockIdx.x * 256u + threadIdx.x, src);
    Ctr c = {0, 0, 0, 0};
    if (live) {
        const size_t i = (size_t)a.pass.first + (size_t)src;
        D3 s, d;
        double lim;
        fetch_ray(a.rays, i, (double)INFINITY, s, d, lim);
        const bool no_lim = a.rays.limits == nullptr;                     // no limit: no comparison is made (a NaN ray_frac counts)
        c.rays = 1;
        AhList L;
        ah_rows(a, i, src, L);
        if (EXTRA) ah_extra(sc, s, d, no_lim, lim, L, c);
        bool loop = true;
        double offset = 0.0;
        if (CLIP) {
            D3 end = s + d * 10000.0;
            const D3 original = s;
            loop = clip_segment<false>(sc.root, s, end);
            if (loop) offset = length(original - s) / length(d);
        }
        if (loop) {
            for (int k = 0; k < sc.ntris; ++k) {
                const Rec128* r = &sc.tris[k];
                double t; D3 pos;
                c.geom++;
                if (!tri_hit(r->p, s, d, t, pos)) continue;
                if (CLIP && !inside(sc.root.lo, sc.root.hi, pos)) continue;
                const double f = CLIP ? t + offset : t;
                if (no_lim || f <= lim) L.offer(f, r->aux);
            }
        }
        L.finish();
        if (a.out_count) a.out_count[i] = L.count;
    }
    if (STATS) block_stat_add(a.stats, c);
}

namespace {

template <bool EXTRA>
hipError_t launch_ah_walk(const AllHitsLaunch& L, const DevScene& sc, const AhArgs& a) {
    const size_t lds = (size_t)stack_levels(sc, MODE_BVH) * 256 * 4;
    if (L.stats) hipLaunchKernelGGL((k_ah_walk<EXTRA, true>), lane_grid(a.pass), dim3(256), lds, L.stream, sc, a);
    else hipLaunchKernelGGL((k_ah_walk<EXTRA, false>), lane_grid(a.pass), dim3(256), lds, L.stream, sc, a);
    return hipGetLastError();
}

template <bool CLIP, bool EXTRA>
hipError_t launch_ah_loop(const AllHitsLaunch& L, const DevScene& sc, const AhArgs& a) {
    if (L.stats) hipLaunchKernelGGL((k_ah_loop<CLIP, EXTRA, true>), lane_grid(a.pass), dim3(256), 0, L.stream, sc, a);
    else hipLaunchKernelGGL((k_ah_loop<CLIP, EXTRA, false>), lane_grid(a.pass), dim3(256), 0, L.stream, sc, a);
    return hipGetLastError();
}

// SR_MODE_BVH: a pass is ordered first (occl_order), the regular rays walk the tree, the tail runs the per-record loop (loop_all: every ray
// does).  SR_MODE_BRUTE: the per-record loop in input order
template <bool EXTRA>
hipError_t launch_all_hits_t(const AllHitsLaunch& L) {
    DevScene sc = L.sc;
    if (!EXTRA) { sc.extra = nullptr; sc.nextra = 0; }                                  // the model alone, whatever the scene's extra geometry
    AhArgs a{};
    a.rays = batch_rays(L.starts, L.dirs, L.limits, L.endpoints);
    a.K = L.max_hits; a.cull_k = (!L.count && L.max_hits > 0) ? 1 : 0;
    a.out_count = L.count; a.out_index = L.index; a.out_frac = L.ray_frac;
    a.s_index = L.scratch_index; a.s_frac = L.scratch_frac;
    a.stats = L.stats;
    return run_passes(
        L, L.mode == MODE_BVH, K_ALL_HITS_SORT, K_ALL_HITS,
        [&](int64_t first, unsigned int count, const PassBuffers& b) { return order_ray_pass(L, a.rays, sc.root, first, count, b); },
        [&](const PassSlice& p, const PassBuffers&) {
            a.pass = p;
            if (L.mode != MODE_BVH) return launch_ah_loop<false, EXTRA>(L, sc, a);
            if (L.loop_all) return launch_ah_loop<true, EXTRA>(L, sc, a);
            a.pass.take = 0;
            const hipError_t e = launch_ah_walk<EXTRA>(L, sc, a);
            a.pass.take = 1;
            return e != hipSuccess ? e : launch_ah_loop<true, EXTRA>(L, sc, a);
        });
}

}  // namespace

hipError_t launch_all_hits(const AllHitsLaunch& L) {
    if (L.n <= 0) return hipSuccess;
    if (L.pass <= 0 || L.pass > kBatchMaxPass || L.max_hits < 0 || L.max_hits > kAllHitsMax) return hipErrorInvalidValue;
    if (L.mode != MODE_BVH && L.mode != MODE_BRUTE) return hipErrorInvalidValue;
    if (L.max_hits > 0 && ((!L.index && !L.scratch_index) || (!L.ray_frac && !L.scratch_frac))) return hipErrorInvalidValue;
    return L.with_extra ? launch_all_hits_t<true>(L) : launch_all_hits_t<false>(L);
}

}  // namespace sr
