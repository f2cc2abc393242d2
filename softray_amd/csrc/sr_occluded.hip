// sr_occluded.hip -- sr_occluded_rays: "is anything in the way before distance L" for a batch of arbitrary rays (gfx950).
//
// The answer per ray is sr_trace_rays' hit && ray_frac <= limit.  On the own BVH a REGULAR ray (occl_order, sr_device.h) takes the any-hit
// walk bvh_intersect<true>(.., limit): the nearest hit's rayFrac is min over the hits of fl(t + offset), fl(t + offset) is monotone in t and
// plane_hit never returns a negative t, so "the nearest qualifies" is "some hit qualifies" and the walk may stop at the first one it meets
// (and cull everything beyond t = limit - offset).  Every other ray, and every ray of the reference tree and of brute force, is answered by
// the function k_trace calls (root_intersect<MODE, false, EXTRA>) plus the comparison: equal to sr_trace_rays by construction.
// The pass driver, the lane's pick, the ray fetch and the refill form's node step are sr_batch.h's, shared with the other batch calls; the
// kernels, the any-hit / nearest-hit split of a pass and the refill form are this file's.
#include "sr_batch.h"

namespace sr {

extern __shared__ __attribute__((aligned(16))) unsigned char lds_occl[];

// One lane per ray of the pass's slice (pass_pick).  ANYHIT (SR_MODE_BVH only): extra primitives first with the reference arithmetic against the ray's limit (as k_ao_probe against
// 2.0; a primitive's rayFrac of DBL_MAX or more never becomes root_intersect's nearest hit, so it does not count here either), then the
// any-hit walk.  One byte store per ray at the ray's input index; nothing else is written (but the statistics).
// LDS: the per-lane traversal stacks, stack levels x 256 lanes x 4 bytes, as k_trace.
template <int MODE, bool EXTRA, bool ANYHIT, bool STATS>
__global__ __launch_bounds__(256) void k_occluded(DevScene sc, const double* __restrict__ starts, const double* __restrict__ dirs, const double* __restrict__ limits,
                                                  long long first, unsigned int count, const unsigned int* __restrict__ order, const unsigned int* __restrict__ keys,
                                                  unsigned int skip_mask, int take, int endpoints, uint8_t* __restrict__ occluded, unsigned long long* stats) {
    const BatchRays rays{starts, dirs, limits, endpoints};                              // (scalar arguments: as structs they cost 12 instructions per lane)
    const PassSlice p{first, count, order, keys, skip_mask, take};
    static_assert(!ANYHIT || MODE == MODE_BVH, "the any-hit walk is the own BVH's");
    const int tid = threadIdx.x;
    Stack st{reinterpret_cast<int32_t*>(lds_occl) + tid, 256};
    unsigned int src;
    const bool live = pass_pick(p, blockIdx.x * 256u + (unsigned int)tid, src);
    Ctr c = {0, 0, 0, 0};
    if (live) {
        const size_t i = (size_t)p.first + (size_t)src;
        D3 s, d;
        double lim;
        fetch_ray(rays, i, 1.0, s, d, lim);
        bool occ = false;
        c.rays = 1;
        Hit h;
        if constexpr (ANYHIT) {
            if (EXTRA) {
                for (int k = 0; k < sc.nextra && !occ; ++k) {
                    double t; D3 pos, nrm;
                    uint32_t tests;
                    const bool ok = extra_hit(&sc.extra[k], s, d, t, pos, nrm, tests);
                    c.geom += tests;
                    occ = ok && t < DBL_MAX && t <= lim;
                }
            }
            if (!occ) occ = bvh_intersect<true>(sc, st, s, d, h, c, lim);
        } else {
            h.t = 0;
            const bool ok = root_intersect<MODE, false, EXTRA>(sc, sc.tris, sc.extra, st, s, d, h, c);
            occ = ok && h.t <= lim;                                                     // IEEE <=: a NaN limit is "not occluded"
        }
        occluded[i] = occ ? 1 : 0;
    }
    if (STATS) block_stat_add(stats, c);                                                // (every thread of the workgroup arrives here)
}

// The any-hit launch with PERSISTENT lanes (hook 100 + T): any-hit walks end at very different times, so a wave whose busy lanes have dropped
// to `refill_at` hands its idle lanes the next rays of the pass's order (one atomicAdd per wave on `head`), the way k_bounce_walk does.  The
// walk is bvh_intersect<true>'s, as a per-lane state machine: same clip, same offset, same boxes culled, same predicate at the same records.
// Not the default: at 1 M triangles it wins 5 - 27 % where walks are long and uneven and loses 25 % where every walk ends after a few nodes
// (profiles/occluded_rays).  Launched with 4 workgroups per CU; `head` is zeroed before every pass.
// The kernel sits at the SGPR limit: it keeps scalar arguments and its own pick of the regular rays (order is never nullptr here) -- the slice
// as a struct and pass_pick both cost it SGPR spills (profiles/batch_refactor).
template <bool EXTRA, bool STATS>
__global__ __launch_bounds__(256) void k_occluded_refill(DevScene sc, const double* __restrict__ starts, const double* __restrict__ dirs,
                                                         const double* __restrict__ limits, long long first, unsigned int count,
                                                         const unsigned int* __restrict__ order, const unsigned int* __restrict__ keys, unsigned int skip_mask,
                                                         int endpoints, uint8_t* __restrict__ occluded, unsigned int* __restrict__ head,
                                                         unsigned long long* stats, int refill_at) {
    const BatchRays rays{starts, dirs, limits, endpoints};
    const int tid = threadIdx.x, lane = tid & 63;
    Stack st{reinterpret_cast<int32_t*>(lds_occl) + tid, 256};
    Ctr c = {0, 0, 0, 0};
    // ---- per ray ----
    size_t mine = 0;                           // the ray's input index
    D3 s = mk(0, 0, 0), d = mk(0, 0, 1);
    double offset = 0.0, lim = 0.0;
    SlabRay ray = {};
    float tlim = FLT_MAX;
    int sp = 0;
    int32_t ni = -1, leafA = -1, leafB = -1;
    bool active = false, drained = false;
    for (;;) {
        const unsigned long long busy = __ballot(active);
        if (!drained && (int)__popcll(busy) <= refill_at) {
            const unsigned long long m = ~busy;
            unsigned int base = 0;
            const int leader = __ffsll((long long)m) - 1;
            if (lane == leader) base = atomicAdd(head, (unsigned int)__popcll(m));
            base = __shfl(base, leader, 64);
            drained = base + (unsigned int)__popcll(m) >= count;
            if (!active) {
                const unsigned int j = base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
                if (j < count && (keys[j] & skip_mask) == 0u) {
                    mine = (size_t)first + (size_t)order[j];
                    fetch_ray(rays, mine, 1.0, s, d, lim);
                    c.rays++;
                    bool occ = false;
                    if (EXTRA) {
                        for (int k = 0; k < sc.nextra && !occ; ++k) {
                            double t; D3 pos, nrm;
                            uint32_t tests;
                            const bool ok = extra_hit(&sc.extra[k], s, d, t, pos, nrm, tests);
                            c.geom += tests;
                            occ = ok && t < DBL_MAX && t <= lim;
                        }
                    }
                    bool walk = !occ;
                    if (walk) {
                        D3 end = s + d * 10000.0;
                        const D3 original = s;
                        walk = clip_segment<false>(sc.root, s, end);
                        if (walk) {
                            offset = length(original - s) / length(d);
                            const double room = lim - offset;
                            walk = !(room < 0.0);
                            tlim = cull_tlim(room);
                        }
                    }
                    if (walk) {
                        set_slab_ray(sc, s, d, ray);
                        sp = 0; ni = 0; leafA = -1; leafB = -1;
                        active = true;
                    } else occluded[mine] = occ ? 1 : 0;
                }
            }
        }
        if (!__any(active)) {
            if (drained) break;
            continue;
        }
        if (active) {
            while (ni >= 0 && leafA < 0) {
                const BvhNode n = sc.bnodes[ni];
                c.nodes++;
                bool h0, h1, first0;
                ray_node_hits(n, ray, tlim, h0, h1, first0);
                walk_step(n, h0, h1, first0, st, sp, ni, leafA, leafB);
            }
            bool occ = false;
            while (leafA >= 0 && !occ) {
                const int32_t lfirst = leafA & kLeafMask, cn = (leafA >> kLeafShift) & 15;
                leafA = leafB;
                leafB = -1;
                c.leaves++;
                for (uint32_t m = leaf_survivors(sc, lfirst, cn, ray.rf, tlim); m && !occ; m &= m - 1u) {
                    const int k = lfirst + (__ffs((int)m) - 1);
                    const Rec128* r = &sc.btris[k];
                    double t; D3 pos;
                    c.geom++;
                    occ = tri_hit(r->p, s, d, t, pos) && inside(sc.root.lo, sc.root.hi, pos) && t + offset <= lim;
                }
            }
            if (occ || (ni < 0 && leafA < 0)) {                    // a hit that counts, or the walk is over
                occluded[mine] = occ ? 1 : 0;
                active = false;
            }
        }
    }
    if (STATS) {
        uint32_t a = wave_sum(c.rays), b = wave_sum(c.geom), c2 = wave_sum(c.nodes), d2 = wave_sum(c.leaves);
        if (lane == 0) { stat_add(&stats[0], a); stat_add(&stats[1], b); stat_add(&stats[2], c2); stat_add(&stats[3], d2); }
    }
}

namespace {

template <int MODE, bool EXTRA, bool ANYHIT>
hipError_t launch_occluded_k(const OccludedLaunch& L, const DevScene& sc, const BatchRays& rays, PassSlice p, int take) {
    p.take = take;
    const size_t lds = (size_t)stack_levels(sc, MODE) * 256 * 4;
    const auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, lane_grid(p), dim3(256), lds, L.stream, sc, rays.starts, rays.dirs, rays.limits, p.first, p.count, p.order, p.keys, p.skip_mask, p.take,
                           rays.endpoints, L.occluded, L.stats);
    };
    if (L.stats) go(k_occluded<MODE, EXTRA, ANYHIT, true>); else go(k_occluded<MODE, EXTRA, ANYHIT, false>);
    return hipGetLastError();
}

template <bool EXTRA>
hipError_t launch_occluded_refill(const OccludedLaunch& L, const DevScene& sc, const BatchRays& rays, const PassSlice& p, unsigned int* head) {
    hipError_t e = hipMemsetAsync(head, 0, sizeof(unsigned int), L.stream);
    if (e != hipSuccess) return e;
    const dim3 grid(std::max(1u, std::min((p.count + 255u) / 256u, (unsigned int)std::max(1, L.persistent_blocks))));
    const size_t lds = (size_t)stack_levels(sc, MODE_BVH) * 256 * 4;
    const int refill_at = std::min(63, std::max(0, L.refill_at));
    const auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, L.stream, sc, rays.starts, rays.dirs, rays.limits, p.first, p.count, p.order, p.keys, p.skip_mask, rays.endpoints,
                           L.occluded, head, L.stats, refill_at);
    };
    if (L.stats) go(k_occluded_refill<EXTRA, true>); else go(k_occluded_refill<EXTRA, false>);
    return hipGetLastError();
}

// SR_MODE_BVH: a pass is ordered first (occl_order: by the start's cell and the direction's octant, or -- input_order -- only its irregular
// rays moved to the end); the regular rays take the any-hit form, the tail the nearest-hit one (nearest_walks: one nearest-hit launch over
// the whole order).  The other modes walk in input order: every ray takes the nearest-hit form
template <int MODE, bool EXTRA>
hipError_t launch_occluded_t(const OccludedLaunch& L) {
    DevScene sc = L.sc;
    if (!EXTRA) { sc.extra = nullptr; sc.nextra = 0; }                                  // the model alone, whatever the scene's extra geometry
    const BatchRays rays = batch_rays(L.starts, L.dirs, L.limits, L.endpoints);
    return run_passes(
        L, MODE == MODE_BVH, K_OCCL_SORT, K_OCCLUDED,
        [&](int64_t first, unsigned int count, const PassBuffers& b) { return order_ray_pass(L, rays, sc.root, first, count, b); },
        [&](const PassSlice& p, const PassBuffers& b) {
            if constexpr (MODE == MODE_BVH) {
                if (L.nearest_walks) return launch_occluded_k<MODE, EXTRA, false>(L, sc, rays, p, 2);
                const hipError_t e = L.refill_at >= 0 ? launch_occluded_refill<EXTRA>(L, sc, rays, p, b.head) : launch_occluded_k<MODE, EXTRA, true>(L, sc, rays, p, 0);
                return e != hipSuccess ? e : launch_occluded_k<MODE, EXTRA, false>(L, sc, rays, p, 1);
            } else {
                return launch_occluded_k<MODE, EXTRA, false>(L, sc, rays, p, 2);
            }
        });
}

}  // namespace

hipError_t launch_occluded(const OccludedLaunch& L) {
    if (L.n <= 0) return hipSuccess;
    if (L.pass <= 0 || L.pass > kBatchMaxPass) return hipErrorInvalidValue;
    switch (L.mode) {
        case MODE_REF: return L.with_extra ? launch_occluded_t<MODE_REF, true>(L) : launch_occluded_t<MODE_REF, false>(L);
        case MODE_BRUTE: return L.with_extra ? launch_occluded_t<MODE_BRUTE, true>(L) : launch_occluded_t<MODE_BRUTE, false>(L);
        case MODE_BVH: return L.with_extra ? launch_occluded_t<MODE_BVH, true>(L) : launch_occluded_t<MODE_BVH, false>(L);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace sr
