// sr_occluded.hip -- sr_occluded_rays: "is anything in the way before distance L" for a batch of arbitrary rays (gfx950).
//
// The answer per ray is sr_trace_rays' hit && ray_frac <= limit.  On the own BVH a REGULAR ray (occl_order, sr_device.h) takes the any-hit
// walk bvh_intersect<true>(.., limit): the nearest hit's rayFrac is min over the hits of fl(t + offset), fl(t + offset) is monotone in t and
// plane_hit never returns a negative t, so "the nearest qualifies" is "some hit qualifies" and the walk may stop at the first one it meets
// (and cull everything beyond t = limit - offset).  Every other ray, and every ray of the reference tree and of brute force, is answered by
// the function k_trace calls (root_intersect<MODE, false, EXTRA>) plus the comparison: equal to sr_trace_rays by construction.
// A kernel of its own translation unit: nothing in sr_kernels.hip / sr_pipeline.hip is touched.
#include "sr_trace.h"

#include <algorithm>

namespace sr {

extern __shared__ __attribute__((aligned(16))) unsigned char lds_occl[];

// One lane per ray of the pass's order: lane j takes ray order[j] (order == nullptr: ray j) of the pass that starts at ray `first`.
// keys[j] is the sorted key of the j-th ray: its bit skip_mask marks an irregular ray.  take 0: the lanes without the bit, 1: those with it,
// 2: all.  ANYHIT (SR_MODE_BVH only): extra primitives first with the reference arithmetic against the ray's limit (as k_ao_probe against
// 2.0; a primitive's rayFrac of DBL_MAX or more never becomes root_intersect's nearest hit, so it does not count here either), then the
// any-hit walk.  One byte store per ray at the ray's input index; nothing else is written (but the statistics).
// LDS: the per-lane traversal stacks, stack levels x 256 lanes x 4 bytes, as k_trace.
template <int MODE, bool EXTRA, bool ANYHIT, bool STATS>
__global__ __launch_bounds__(256) void k_occluded(DevScene sc, const double* __restrict__ starts, const double* __restrict__ dirs, const double* __restrict__ limits,
                                                  long long first, unsigned int count, const unsigned int* __restrict__ order, const unsigned int* __restrict__ keys,
                                                  unsigned int skip_mask, int take, int endpoints, uint8_t* __restrict__ occluded, unsigned long long* stats) {
    static_assert(!ANYHIT || MODE == MODE_BVH, "the any-hit walk is the own BVH's");
    const int tid = threadIdx.x;
    Stack st{reinterpret_cast<int32_t*>(lds_occl) + tid, 256};
    const unsigned int j = blockIdx.x * 256u + (unsigned int)tid;                       // (a pass has at most 2^22 rays)
    bool live = j < count;
    unsigned int src = j;
    if (order && live) {
        src = order[j];
        if (take != 2) live = ((keys[j] & skip_mask) != 0u) == (take == 1);
    }
    Ctr c = {0, 0, 0, 0};
    if (live) {
        const size_t i = (size_t)first + (size_t)src;                                   // 64-bit from here on: n x 24 bytes may pass 2^32
        const D3 s = mk(starts[3 * i], starts[3 * i + 1], starts[3 * i + 2]);
        const D3 e = mk(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
        const D3 d = endpoints ? e - s : e;                                             // ShadowMethod.cs:157: one FP64 subtraction per component
        const double lim = limits ? limits[i] : 1.0;
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
    if (STATS) {                                                                        // (every thread of the workgroup arrives here)
        uint32_t a = wave_sum(c.rays), b = wave_sum(c.geom), c2 = wave_sum(c.nodes), d2 = wave_sum(c.leaves);
        block_stat_add(&stats[0], &stats[1], &stats[2], &stats[3], a, b, c2, d2);
    }
}

// The any-hit launch with PERSISTENT lanes (hook 100 + T): any-hit walks end at very different times, so a wave whose busy lanes have dropped
// to `refill_at` hands its idle lanes the next rays of the pass's order (one atomicAdd per wave on `head`), the way k_bounce_walk does.  The
// walk is bvh_intersect<true>'s, as a per-lane state machine: same clip, same offset, same boxes culled, same predicate at the same records.
// Not the default: at 1 M triangles it wins 5 - 27 % where walks are long and uneven and loses 25 % where every walk ends after a few nodes
// (profiles/occluded_rays).  Launched with 4 workgroups per CU; `head` is zeroed before every pass.
template <bool EXTRA, bool STATS>
__global__ __launch_bounds__(256) void k_occluded_refill(DevScene sc, const double* __restrict__ starts, const double* __restrict__ dirs,
                                                         const double* __restrict__ limits, long long first, unsigned int count,
                                                         const unsigned int* __restrict__ order, const unsigned int* __restrict__ keys, unsigned int skip_mask,
                                                         int endpoints, uint8_t* __restrict__ occluded, unsigned int* __restrict__ head,
                                                         unsigned long long* stats, int refill_at) {
    const int tid = threadIdx.x, lane = tid & 63;
    Stack st{reinterpret_cast<int32_t*>(lds_occl) + tid, 256};
    const float kInfl = 1.0f + 9.5367431640625e-7f;          // 1 + 2^-20
    Ctr c = {0, 0, 0, 0};
    // ---- per ray ----
    size_t mine = 0;                           // the ray's input index
    D3 s = mk(0, 0, 0), d = mk(0, 0, 1);
    double offset = 0.0, lim = 0.0;
    f2 I01 = splat(0.0f), I20 = I01, I12 = I01, B0 = I01, B1 = I01, B2 = I01;
    RayF rf = {};
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
                    s = mk(starts[3 * mine], starts[3 * mine + 1], starts[3 * mine + 2]);
                    const D3 e = mk(dirs[3 * mine], dirs[3 * mine + 1], dirs[3 * mine + 2]);
                    d = endpoints ? e - s : e;
                    lim = limits ? limits[mine] : 1.0;
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
                            tlim = (float)room * kInfl + 1e-30f;
                        }
                    }
                    if (walk) {
                        const float ox = (float)(s.x - sc.root.centre[0]), oy = (float)(s.y - sc.root.centre[1]), oz = (float)(s.z - sc.root.centre[2]);
                        const float ix = slab_inv((float)d.x), iy = slab_inv((float)d.y), iz = slab_inv((float)d.z);
                        I01 = (f2){ix, iy}; I20 = (f2){iz, ix}; I12 = (f2){iy, iz};
                        B0 = (f2){-ox * ix, -oy * iy}; B1 = (f2){-oz * iz, -ox * ix}; B2 = (f2){-oy * iy, -oz * iz};
                        rf = make_ray_f(sc, s, d);
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
                float t0, x0, t1, x1;
                node_slabs(n, I01, I20, I12, B0, B1, B2, t0, x0, t1, x1);
                const bool h0 = n.n0 >= 0 && t0 <= x0 && x0 >= 0.0f && t0 <= tlim;
                const bool h1 = n.n1 >= 0 && t1 <= x1 && x1 >= 0.0f && t1 <= tlim;
                const bool l0 = h0 && n.n0 > 0, l1 = h1 && n.n1 > 0;
                if (l0 && l1) {
                    const bool first0 = t0 <= t1;
                    leafA = (first0 ? n.c0 : n.c1) | ((first0 ? n.n0 : n.n1) << kLeafShift);
                    leafB = (first0 ? n.c1 : n.c0) | ((first0 ? n.n1 : n.n0) << kLeafShift);
                } else if (l0) leafA = n.c0 | (n.n0 << kLeafShift);
                else if (l1) leafA = n.c1 | (n.n1 << kLeafShift);
                const bool i0 = h0 && n.n0 == 0, i1 = h1 && n.n1 == 0;
                if (i0 && i1) {
                    const bool first0 = t0 <= t1;
                    st.put(sp++, first0 ? n.c1 : n.c0);
                    ni = first0 ? n.c0 : n.c1;
                } else if (i0) ni = n.c0;
                else if (i1) ni = n.c1;
                else ni = (sp > 0) ? st.get(--sp) : -1;
            }
            bool occ = false;
            while (leafA >= 0 && !occ) {
                const int32_t lfirst = leafA & kLeafMask, cn = (leafA >> kLeafShift) & 15;
                leafA = leafB;
                leafB = -1;
                c.leaves++;
                for (uint32_t m = leaf_survivors(sc, lfirst, cn, rf, tlim); m && !occ; m &= m - 1u) {
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

int occl_stack_levels(const DevScene& sc, int mode) {
    if (mode == MODE_REF) return sc.rdepth + 2;
    if (mode == MODE_BVH) return sc.bdepth + 2;
    return 1;
}

template <int MODE, bool EXTRA, bool ANYHIT>
hipError_t launch_occluded_k(const OccludedLaunch& L, const DevScene& sc, long long first, unsigned int count, const unsigned int* order, const unsigned int* keys,
                             unsigned int skip_mask, int take) {
    const dim3 grid((count + 255u) / 256u);
    const size_t lds = (size_t)occl_stack_levels(sc, MODE) * 256 * 4;
    const auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, L.stream, sc, L.starts, L.dirs, L.limits, first, count, order, keys, skip_mask, take, L.endpoints ? 1 : 0,
                           L.occluded, L.stats);
    };
    if (L.stats) go(k_occluded<MODE, EXTRA, ANYHIT, true>); else go(k_occluded<MODE, EXTRA, ANYHIT, false>);
    return hipGetLastError();
}

template <bool EXTRA>
hipError_t launch_occluded_refill(const OccludedLaunch& L, const DevScene& sc, long long first, unsigned int count, const unsigned int* order, const unsigned int* keys,
                                  unsigned int skip_mask, unsigned int* head) {
    hipError_t e = hipMemsetAsync(head, 0, sizeof(unsigned int), L.stream);
    if (e != hipSuccess) return e;
    const dim3 grid(std::max(1u, std::min((count + 255u) / 256u, (unsigned int)std::max(1, L.persistent_blocks))));
    const size_t lds = (size_t)occl_stack_levels(sc, MODE_BVH) * 256 * 4;
    const int refill_at = std::min(63, std::max(0, L.refill_at));
    const auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, L.stream, sc, L.starts, L.dirs, L.limits, first, count, order, keys, skip_mask, L.endpoints ? 1 : 0, L.occluded,
                           head, L.stats, refill_at);
    };
    if (L.stats) go(k_occluded_refill<EXTRA, true>); else go(k_occluded_refill<EXTRA, false>);
    return hipGetLastError();
}

// pass by pass, back to back on the stream.  SR_MODE_BVH: a pass is ordered first (occl_order: by the start's cell and the direction's octant,
// or -- input_order -- only its irregular rays moved to the end); the regular rays take the any-hit form, the tail the nearest-hit one
// (nearest_walks: one nearest-hit launch over the whole order).  The other modes walk in input order: every ray takes the nearest-hit form
template <int MODE, bool EXTRA>
hipError_t launch_occluded_t(const OccludedLaunch& L) {
    DevScene sc = L.sc;
    if (!EXTRA) { sc.extra = nullptr; sc.nextra = 0; }                                  // the model alone, whatever the scene's extra geometry
    const unsigned int cap = (unsigned int)((L.pass + 255) / 256 * 256);
    unsigned int* keys = L.sort_buf;
    unsigned int* keys2 = keys + cap;
    unsigned int* idx = keys2 + cap;
    unsigned int* order = idx + cap;
    const unsigned int skip = point_order_skip_mask(!L.input_order);
    for (int64_t first = 0; first < L.n; first += L.pass) {
        const unsigned int count = (unsigned int)std::min<int64_t>(L.pass, L.n - first);
        hipError_t e;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (MODE == MODE_BVH) {
            if (L.get_events) L.get_events(L.user, K_OCCL_SORT, &e0, &e1);
            if (e0 && (e = hipEventRecord(e0, L.stream)) != hipSuccess) return e;
            if ((e = occl_order(L.starts + 3 * first, L.dirs + 3 * first, L.limits ? L.limits + first : nullptr, count, L.endpoints, !L.input_order, sc.root, keys,
                                keys2, idx, order, L.sort_temp, L.sort_temp_bytes, L.stream)) != hipSuccess)
                return e;
            if (e1 && (e = hipEventRecord(e1, L.stream)) != hipSuccess) return e;
        }
        e0 = e1 = nullptr;
        if (L.get_events) L.get_events(L.user, K_OCCLUDED, &e0, &e1);
        if (e0 && (e = hipEventRecord(e0, L.stream)) != hipSuccess) return e;
        if constexpr (MODE == MODE_BVH) {
            if (L.nearest_walks) e = launch_occluded_k<MODE, EXTRA, false>(L, sc, first, count, order, keys2, skip, 2);
            else {
                if (L.refill_at >= 0) e = launch_occluded_refill<EXTRA>(L, sc, first, count, order, keys2, skip, order + cap);
                else e = launch_occluded_k<MODE, EXTRA, true>(L, sc, first, count, order, keys2, skip, 0);
                if (e == hipSuccess) e = launch_occluded_k<MODE, EXTRA, false>(L, sc, first, count, order, keys2, skip, 1);
            }
        } else {
            e = launch_occluded_k<MODE, EXTRA, false>(L, sc, first, count, nullptr, nullptr, 0u, 2);
        }
        if (e != hipSuccess) return e;
        if (e1 && (e = hipEventRecord(e1, L.stream)) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_occluded(const OccludedLaunch& L) {
    if (L.n <= 0) return hipSuccess;
    if (L.pass <= 0 || L.pass > kOcclMaxPass) return hipErrorInvalidValue;
    switch (L.mode) {
        case MODE_REF: return L.with_extra ? launch_occluded_t<MODE_REF, true>(L) : launch_occluded_t<MODE_REF, false>(L);
        case MODE_BRUTE: return L.with_extra ? launch_occluded_t<MODE_BRUTE, true>(L) : launch_occluded_t<MODE_BRUTE, false>(L);
        case MODE_BVH: return L.with_extra ? launch_occluded_t<MODE_BVH, true>(L) : launch_occluded_t<MODE_BVH, false>(L);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace sr
