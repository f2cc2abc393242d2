// sr_nearest.hip -- sr_nearest_rays: the nearest hit of a batch of arbitrary rays, with a per-ray distance limit (gfx950).
//
// The answer per ray is sr_trace_rays' when that is a hit with ray_frac <= limit, and sr_trace_rays' miss otherwise.  If the nearest hit does
// not qualify no hit does (fl(t + offset) is monotone in t), so "the nearest hit, if it qualifies" is "the nearest qualifying hit" and a walk
// may cull every box beyond t = limit - offset, inflated as bvh_intersect<true> does it; the test best + offset <= limit itself is FP64.
// On the own BVH a REGULAR ray (occl_order, sr_device.h) takes the route of a mirror level's rays (sr_pipeline.hip k_bounce_prep / _walk /
// _finish): k_nr_prep (FP64 clip, offset, cull bound), k_nr_walk (persistent lanes on the four-wide tree, the stack split between LDS and
// global memory), k_nr_finish (extra geometry, the limit, the outputs).  Every other ray, and every ray of the reference tree and of brute
// force, is answered by the function k_trace calls (root_intersect<MODE, false, EXTRA>) plus the comparison: equal to sr_trace_rays by
// construction.  The pass driver, the lane's pick, the ray fetch, the walk's ray frame and its binary node step are sr_batch.h's, shared with
// the other batch calls; the three-kernel route, the four-wide walk, the split stack and the per-lane tail are this file's.
#include "sr_batch.h"

namespace sr {

extern __shared__ __attribute__((aligned(16))) unsigned char lds_nr[];

struct alignas(16) NrRay {
    double   s[3], d[3];         // clipped start (SpatialSubdivision.cs:394), direction D
    double   offset;             // rayFracOffset (:401); < 0: no walk (the ray misses the root box, its limit lies before the box, or it is irregular)
    uint32_t index;              // the ray's input index within the pass
    float    tlim;               // fp32 cull bound of the walk: limit - offset, inflated (FLT_MAX: no limit)
};
static_assert(sizeof(NrRay) == 64, "NrRay must be 64 bytes");
struct alignas(16) NrHit {
    double  best;                // rayFrac from the clipped start of the nearest triangle hit (DBL_MAX: none)
    int32_t bestK, pad;          // its record (-1: none)
};
static_assert(sizeof(NrHit) == 16, "NrHit must be 16 bytes");

struct NrOut {
    uint8_t* hit; double* ray_frac; double* pos; double* normal; uint32_t* color; int32_t* tri;       // device [n] each, or nullptr
};

// sr_trace_rays' stores (k_trace) for ray i
__device__ __forceinline__ void nr_store(const NrOut& o, size_t i, bool ok, const Hit& h) {
    if (o.hit) o.hit[i] = ok ? 1 : 0;
    if (o.ray_frac) o.ray_frac[i] = ok ? h.t : 0.0;
    if (o.pos) { o.pos[3 * i] = ok ? h.pos.x : 0.0; o.pos[3 * i + 1] = ok ? h.pos.y : 0.0; o.pos[3 * i + 2] = ok ? h.pos.z : 0.0; }
    if (o.normal) { o.normal[3 * i] = ok ? h.nrm.x : 0.0; o.normal[3 * i + 1] = ok ? h.nrm.y : 0.0; o.normal[3 * i + 2] = ok ? h.nrm.z : 0.0; }
    if (o.color) o.color[i] = ok ? h.color : 0u;
    if (o.tri) o.tri[i] = ok ? h.tri : -1;
}

// lane = position j in the pass's order (p.take is 0, the order is never nullptr here): an irregular ray gets a record without a walk
// (k_nr_lane answers it).
__global__ __launch_bounds__(256) void k_nr_prep(DevScene sc, BatchRays rays, PassSlice p, NrRay* __restrict__ prep, NrHit* __restrict__ res) {
    const unsigned int j = blockIdx.x * 256u + threadIdx.x;
    if (j >= p.count) return;
    unsigned int src;
    const bool regular = pass_pick(p, j, src);
    NrRay o;
    o.s[0] = o.s[1] = o.s[2] = 0.0; o.d[0] = o.d[1] = o.d[2] = 0.0;
    o.offset = -1.0; o.index = src; o.tlim = 0.0f;
    if (regular) {
        D3 s0, d;
        double lim;
        fetch_ray(rays, (size_t)p.first + (size_t)src, 0.0, s0, d, lim);                // (no limits: lim is not read)
        D3 s = s0;
        D3 end = s + d * 10000.0;
        bool walking = clip_segment<false>(sc.root, s, end);
        float tlim = FLT_MAX;
        double offset = -1.0;
        if (walking) {
            offset = length(s0 - s) / length(d);
            if (rays.limits) {
                const double room = lim - offset;
                walking = !(room < 0.0);
                tlim = cull_tlim(room);
            }
        }
        o.s[0] = s.x; o.s[1] = s.y; o.s[2] = s.z;
        o.d[0] = d.x; o.d[1] = d.y; o.d[2] = d.z;
        o.offset = walking ? offset : -1.0;
        o.tlim = tlim;
    }
    prep[j] = o;
    NrHit h;
    h.best = DBL_MAX; h.bestK = -1; h.pad = 0;
    res[j] = h;
}

// k_bounce_walk's loop (sr_pipeline.hip) for the records of k_nr_prep: persistent lanes that fetch the next records of the pass at `refill_at`
// busy lanes (one atomicAdd per refill on `head`, zeroed per pass), the four-wide tree with the sorting network and up to eight pending
// leaves (WIDE; the binary tree otherwise), the fp32 pre-test, then the reference's FP64 test on the survivors with the lowest-index tie
// rule.  What differs: the cull bound starts at the record's tlim instead of FLT_MAX and never grows, and the counters go to [1..3].
// LDS: lds_levels x 256 lanes x 4 bytes of stack; the deeper levels in `deep`, [level][lane of the grid].
// (WIDE: 105 VGPRs, 108 with STATS = 4 waves/SIMD, no scratch.  Bounded to 96 for 5 waves, as k_bounce_walk is, it spills 18 / 21 VGPRs to
// 52 / 64 bytes of scratch per lane; the binary form takes 84 / 86 and runs at 5 waves either way: profiles/nearest_rays/kernel_resources.txt)
template <bool STATS, bool WIDE>
__global__ __launch_bounds__(256, 4) void k_nr_walk(DevScene sc, const NrRay* __restrict__ prep, unsigned int total, unsigned int* __restrict__ head,
                                                    NrHit* __restrict__ res, unsigned long long* stats, int refill_at, int32_t* __restrict__ deep, int lds_levels) {
    const int tid = threadIdx.x, lane = tid & 63;
    SplitStack st{reinterpret_cast<int32_t*>(lds_nr) + tid, deep + (size_t)blockIdx.x * 256u + (unsigned)tid, lds_levels, (int32_t)(gridDim.x * 256u)};
    Ctr c = {0, 0, 0, 0};
    // ---- per ray ----
    unsigned int mine = 0;                     // position of the lane's ray in prep / res
    double best = DBL_MAX;
    int32_t bestIdx = 0x7fffffff, bestK = -1;
    SlabRay ray = {};
    float tlim = FLT_MAX;
    int sp = 0;
    int32_t ni = -1, leafA = -1, leafB = -1, leafC = -1, leafD = -1, leafE = -1, leafF = -1, leafG = -1, leafH = -1;
    bool active = false;
    bool drained = false;
    for (;;) {
        const unsigned long long busy = __ballot(active);
        if (!drained && (int)__popcll(busy) <= refill_at) {
            const unsigned long long m = ~busy;
            unsigned int base = 0;
            const int leader = __ffsll((long long)m) - 1;
            if (lane == leader) base = atomicAdd(head, (unsigned int)__popcll(m));
            base = __shfl(base, leader, 64);
            drained = base + (unsigned int)__popcll(m) >= total;
            if (!active) {
                const unsigned int r = base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
                if (r < total) {
                    const NrRay q = prep[r];
                    if (q.offset >= 0.0) {
                        mine = r;
                        const D3 s = mk(q.s[0], q.s[1], q.s[2]), d = mk(q.d[0], q.d[1], q.d[2]);   // (not carried through the walk: see the FP64 tests)
                        best = DBL_MAX; bestIdx = 0x7fffffff; bestK = -1;
                        set_slab_ray(sc, s, d, ray);
                        tlim = q.tlim;
                        sp = 0; ni = 0; leafA = -1; leafB = -1; leafC = -1; leafD = -1; leafE = leafF = leafG = leafH = -1;
                        active = true;
                    }
                }
            }
        }
        if (!__any(active)) {
            if (drained) break;
            continue;
        }
        if (active) {
            // (the speculative walk of k_bounce_walk: up to eight pending leaves, on while at most four wait)
            while (WIDE && ni >= 0 && leafE < 0) {
                const Bvh4Node n = sc.b4[ni];
                c.nodes++;
                float tk[4];
                int32_t ck[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float t, x;
                    child_slabs(n.ch[k], ray.I01, ray.I20, ray.I12, ray.B0, ray.B1, ray.B2, t, x);
                    const bool h = n.ch[k].n >= 0 && t <= x && x >= 0.0f && t <= tlim;
                    tk[k] = (h && n.ch[k].n == 0) ? t : FLT_MAX;
                    ck[k] = n.ch[k].c;
                    if (h && n.ch[k].n > 0) {
                        const int32_t v = n.ch[k].c | (n.ch[k].n << kLeafShift);
                        if (leafA < 0) leafA = v; else if (leafB < 0) leafB = v; else if (leafC < 0) leafC = v; else if (leafD < 0) leafD = v; else if (leafE < 0) leafE = v; else if (leafF < 0) leafF = v; else if (leafG < 0) leafG = v; else leafH = v;
                    }
                }
#define SR_CE(a, b) { const bool sw = tk[b] < tk[a]; const float ta = tk[a]; const int32_t ca = ck[a]; \
                      tk[a] = sw ? tk[b] : ta; ck[a] = sw ? ck[b] : ca; tk[b] = sw ? ta : tk[b]; ck[b] = sw ? ca : ck[b]; }
                SR_CE(0, 1) SR_CE(2, 3) SR_CE(0, 2) SR_CE(1, 3) SR_CE(1, 2)
#undef SR_CE
                if (tk[3] < FLT_MAX) st.put(sp++, ck[3]);
                if (tk[2] < FLT_MAX) st.put(sp++, ck[2]);
                if (tk[1] < FLT_MAX) st.put(sp++, ck[1]);
                ni = tk[0] < FLT_MAX ? ck[0] : ((sp > 0) ? st.get(--sp) : -1);
            }
            while (!WIDE && ni >= 0 && leafA < 0) {
                const BvhNode n = sc.bnodes[ni];
                c.nodes++;
                bool h0, h1, first0;
                ray_node_hits(n, ray, tlim, h0, h1, first0);
                walk_step(n, h0, h1, first0, st, sp, ni, leafA, leafB);
            }
            while (leafA >= 0) {
                const int32_t first = leafA & kLeafMask, cn = (leafA >> kLeafShift) & 15;
                leafA = leafB;
                leafB = WIDE ? leafC : -1;
                if (WIDE) { leafC = leafD; leafD = leafE; leafE = leafF; leafF = leafG; leafG = leafH; leafH = -1; }
                c.leaves++;
                uint32_t m = leaf_survivors(sc, first, cn, ray.rf, tlim);
                if (m) {
                    // As k_bounce_walk: the FP64 record and the FP64 ray are the register peak, so the ray is read from the prepared array
                    // here and the fp32 frames -- dead while the test runs -- are made again from it with the refill's expressions.
                    const NrRay* pq = &prep[mine];
                    const D3 s = mk(pq->s[0], pq->s[1], pq->s[2]), d = mk(pq->d[0], pq->d[1], pq->d[2]);
                    for (; m; m &= m - 1u) {
                        const int k = first + (__ffs((int)m) - 1);
                        const Rec128* r = &sc.btris[k];
                        double t; D3 pos;
                        c.geom++;
                        if (tri_hit(r->p, s, d, t, pos) && inside(sc.root.lo, sc.root.hi, pos)) {
                            const int32_t idx = r->aux;
                            if (t < best || (t == best && idx < bestIdx)) {
                                best = t; bestIdx = idx; bestK = k;
                                tlim = fminf(tlim, cull_tlim(best));                       // (never beyond the ray's limit)
                            }
                        }
                    }
                    set_slab_ray(sc, s, d, ray);
                }
            }
            if (ni < 0 && leafA < 0) {                            // the walk is over
                NrHit h;
                h.best = best; h.bestK = bestK; h.pad = 0;
                res[mine] = h;
                active = false;
            }
        }
    }
    if (STATS) {
        uint32_t b = wave_sum(c.geom), c2 = wave_sum(c.nodes), d2 = wave_sum(c.leaves);
        if (lane == 0) { stat_add(&stats[1], b); stat_add(&stats[2], c2); stat_add(&stats[3], d2); }
    }
}

// lane = position j in the pass's order, regular rays only: root_intersect's choice between the extra geometry (from the UNCLIPPED start, in
// collection order, strict '<') and the walk's triangle, the limit, and sr_trace_rays' stores at the ray's input index.
template <bool EXTRA, bool STATS>
__global__ __launch_bounds__(256) void k_nr_finish(DevScene sc, const double* __restrict__ starts, const double* __restrict__ limits, PassSlice p,
                                                   const NrRay* __restrict__ prep, const NrHit* __restrict__ res, NrOut out, unsigned long long* stats) {
    const unsigned int j = blockIdx.x * 256u + threadIdx.x;
    uint32_t n_rays = 0, n_geom = 0;
    if (j < p.count && (p.keys[j] & p.skip_mask) == 0u) {
        const NrRay q = prep[j];
        const NrHit w = res[j];
        const size_t i = (size_t)p.first + (size_t)q.index;
        const D3 s = mk(q.s[0], q.s[1], q.s[2]), d = mk(q.d[0], q.d[1], q.d[2]);
        n_rays = 1;
        Hit h;
        h.t = 0; h.pos = mk(0, 0, 0); h.nrm = mk(0, 0, 0); h.color = 0; h.tri = -1;
        bool ok = false;
        double ex_t = DBL_MAX;
        if (EXTRA) {
            const D3 s0 = mk(starts[3 * i], starts[3 * i + 1], starts[3 * i + 2]);
            for (int k = 0; k < sc.nextra; ++k) {
                const Rec128* e = &sc.extra[k];
                double t; D3 pos, nrm;
                uint32_t tests;
                const bool hit = extra_hit(e, s0, d, t, pos, nrm, tests);
                n_geom += tests;
                if (hit && t < ex_t) { ex_t = t; ok = true; h.t = t; h.pos = pos; h.nrm = nrm; h.color = e->color; h.tri = -1; }
            }
        }
        if (q.offset >= 0.0 && w.bestK >= 0 && (w.best + q.offset) < ex_t) {
            const Rec128* t = &sc.btris[w.bestK];
            ok = true;
            h.t = w.best + q.offset;
            h.pos = s + d * w.best;          // the expression plane_hit evaluated for the winning triangle (pos = start + dir * rayFrac)
            h.nrm = mk(t->p[0], t->p[1], t->p[2]);
            h.color = t->color;
            h.tri = t->aux;
        }
        if (limits) ok = ok && h.t <= limits[i];                                        // IEEE <=
        nr_store(out, i, ok, h);
    }
    if (STATS) {                                                                        // (every thread of the workgroup arrives here)
        uint32_t a = wave_sum(n_rays), b = wave_sum(n_geom);
        block_stat_add(&stats[0], &stats[1], &stats[2], &stats[3], a, b, 0u, 0u);
    }
}

// One lane per ray, the function k_trace calls plus the comparison: the irregular rays of a SR_MODE_BVH pass (take 1), and every ray of the
// other modes and of hook 49 (input order).
// LDS: the per-lane traversal stacks, stack levels x 256 lanes x 4 bytes, as k_trace.
template <int MODE, bool EXTRA, bool STATS>
__global__ __launch_bounds__(256) void k_nr_lane(DevScene sc, BatchRays rays, PassSlice p, NrOut out, unsigned long long* stats) {
    const int tid = threadIdx.x;
    Stack st{reinterpret_cast<int32_t*>(lds_nr) + tid, 256};
    unsigned int src;
    const bool live = pass_pick(p, blockIdx.x * 256u + (unsigned int)tid, src);
    Ctr c = {0, 0, 0, 0};
    if (live) {
        const size_t i = (size_t)p.first + (size_t)src;
        D3 s, d;
        fetch_ray(rays, i, s, d);                                                       // (the limit is read after the walk: held across it, it costs two VGPRs)
        c.rays = 1;
        Hit h;
        h.t = 0; h.pos = mk(0, 0, 0); h.nrm = mk(0, 0, 0); h.color = 0; h.tri = -1;
        bool ok = root_intersect<MODE, false, EXTRA>(sc, sc.tris, sc.extra, st, s, d, h, c);
        if (rays.limits) ok = ok && h.t <= rays.limits[i];                              // IEEE <=: a NaN limit is a miss
        nr_store(out, i, ok, h);
    }
    if (STATS) block_stat_add(stats, c);                                                // (every thread of the workgroup arrives here)
}

namespace {

NrOut nr_out(const NearestLaunch& L) { return NrOut{L.hit, L.ray_frac, L.pos, L.normal, L.color, L.tri}; }

template <int MODE, bool EXTRA>
hipError_t launch_nr_lane(const NearestLaunch& L, const DevScene& sc, const BatchRays& rays, PassSlice p) {
    p.take = 1;
    const size_t lds = (size_t)stack_levels(sc, MODE) * 256 * 4;
    const auto go = [&](auto kern) { hipLaunchKernelGGL(kern, lane_grid(p), dim3(256), lds, L.stream, sc, rays, p, nr_out(L), L.stats); };
    if (L.stats) go(k_nr_lane<MODE, EXTRA, true>); else go(k_nr_lane<MODE, EXTRA, false>);
    return hipGetLastError();
}

// prep, walk, finish of a pass's regular rays; `head`: the walk's work head
template <bool EXTRA>
hipError_t launch_nr_walked(const NearestLaunch& L, const DevScene& sc, const BatchRays& rays, PassSlice p, unsigned int* head) {
    p.take = 0;
    hipError_t e = hipMemsetAsync(head, 0, sizeof(unsigned int), L.stream);
    if (e != hipSuccess) return e;
    const unsigned int blocks = (p.count + 255u) / 256u;
    NrRay* prep = (NrRay*)L.prep;
    NrHit* res = (NrHit*)L.res;
    hipLaunchKernelGGL(k_nr_prep, dim3(blocks), dim3(256), 0, L.stream, sc, rays, p, prep, res);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const bool wide = sc.b4 != nullptr && !L.bvh2;
    const int levels_all = wide ? 3 * sc.b4depth + 2 : stack_levels(sc, MODE_BVH);
    const unsigned int wblocks = std::max(1u, std::min(blocks, (unsigned int)std::max(1, L.persistent_blocks)));
    // stack levels in LDS: L.lds_levels when the rest of the worst case fits the overflow buffer, all of them otherwise
    int lds_levels = std::max(1, std::min(L.lds_levels, levels_all));
    if (!L.deep || (size_t)(levels_all - lds_levels) * (size_t)wblocks * 256 * 4 > L.deep_bytes) lds_levels = levels_all;
    const int refill_at = std::min(63, std::max(0, L.refill_at));
    const auto walk = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(wblocks), dim3(256), (size_t)lds_levels * 256 * 4, L.stream, sc, (const NrRay*)prep, p.count, head, res, L.stats, refill_at, L.deep,
                           lds_levels);
    };
    if (wide) { if (L.stats) walk(k_nr_walk<true, true>); else walk(k_nr_walk<false, true>); }
    else { if (L.stats) walk(k_nr_walk<true, false>); else walk(k_nr_walk<false, false>); }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const auto fin = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, L.stream, sc, rays.starts, rays.limits, p, (const NrRay*)prep, (const NrHit*)res, nr_out(L), L.stats);
    };
    if (L.stats) fin(k_nr_finish<EXTRA, true>); else fin(k_nr_finish<EXTRA, false>);
    return hipGetLastError();
}

// SR_MODE_BVH: a pass is ordered first (occl_order: by the start's cell and the direction's octant, or -- input_order -- only its irregular
// rays moved to the end); the regular rays take prep / walk / finish, the tail the per-lane form (lane_walks: one per-lane launch over the
// pass in input order, no sort).  The other modes walk per lane in input order
template <int MODE, bool EXTRA>
hipError_t launch_nearest_t(const NearestLaunch& L) {
    DevScene sc = L.sc;
    if (!EXTRA) { sc.extra = nullptr; sc.nextra = 0; }                                  // the model alone, whatever the scene's extra geometry
    const BatchRays rays = batch_rays(L.starts, L.dirs, L.limits, L.endpoints);
    return run_passes(
        L, MODE == MODE_BVH && !L.lane_walks, K_NEAREST_SORT, K_NEAREST,
        [&](int64_t first, unsigned int count, const PassBuffers& b) { return order_ray_pass(L, rays, sc.root, first, count, b); },
        [&](const PassSlice& p, const PassBuffers& b) {
            if constexpr (MODE == MODE_BVH) {
                if (!L.lane_walks) {
                    const hipError_t e = launch_nr_walked<EXTRA>(L, sc, rays, p, b.head);
                    if (e != hipSuccess) return e;
                }
            }
            return launch_nr_lane<MODE, EXTRA>(L, sc, rays, p);
        });
}

}  // namespace

hipError_t launch_nearest(const NearestLaunch& L) {
    if (L.n <= 0) return hipSuccess;
    if (L.pass <= 0 || L.pass > kBatchMaxPass) return hipErrorInvalidValue;
    switch (L.mode) {
        case MODE_REF: return L.with_extra ? launch_nearest_t<MODE_REF, true>(L) : launch_nearest_t<MODE_REF, false>(L);
        case MODE_BRUTE: return L.with_extra ? launch_nearest_t<MODE_BRUTE, true>(L) : launch_nearest_t<MODE_BRUTE, false>(L);
        case MODE_BVH: return L.with_extra ? launch_nearest_t<MODE_BVH, true>(L) : launch_nearest_t<MODE_BVH, false>(L);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace sr
