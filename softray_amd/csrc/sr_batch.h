// sr_batch.h -- what the batch calls without a frame share (sr_occluded.hip, sr_nearest.hip, sr_allhits.hip, sr_closest.hip, sr_near.hip, sr_overlap.hip; nothing else
// includes it).  Device side: which item a lane of a pass takes, an item's ray, the fp32 frame of a ray for the private binary walk and that
// walk's node step, the statistics epilogue.  Host side: the pass driver.  A call keeps what is its own: its kernels, how a pass is
// ordered and what is launched for one.
#pragma once
#include "sr_trace.h"

#include <algorithm>

namespace sr {

// ---- device ----------------------------------------------------------------------------------------------------------------------------
// The items of one pass, `count` (<= 2^22) from item `first` of the call.  Lane j takes item order[j] (order == nullptr: item j); keys[j] is
// the sorted key of that item, its bit skip_mask marks an irregular one.  take 0: the regular items, 1: the others, 2: all
struct PassSlice {
    long long first; unsigned int count;
    const unsigned int* order; const unsigned int* keys; unsigned int skip_mask; int take;
};
// does lane j have an item, and which (src, within the pass: valid whenever j < count)
__device__ __forceinline__ bool pass_pick(const PassSlice& p, unsigned int j, unsigned int& src) {
    bool live = j < p.count;
    src = j;
    if (p.order && live) {
        src = p.order[j];
        if (p.take != 2) live = ((p.keys[j] & p.skip_mask) != 0u) == (p.take == 1);
    }
    return live;
}

// the rays of a call; item i (64-bit: n x 24 bytes may pass 2^32) starts at s with direction d -- endpoints: dirs holds end points, one FP64
// subtraction per component (ShadowMethod.cs:157) -- and limit lim; no_limits: the call's own value where the caller passed no limits
struct BatchRays { const double* starts; const double* dirs; const double* limits; int endpoints; };
__device__ __forceinline__ void fetch_ray(const BatchRays& r, size_t i, D3& s, D3& d) {
    s = mk(r.starts[3 * i], r.starts[3 * i + 1], r.starts[3 * i + 2]);
    const D3 e = mk(r.dirs[3 * i], r.dirs[3 * i + 1], r.dirs[3 * i + 2]);
    d = r.endpoints ? e - s : e;
}
__device__ __forceinline__ void fetch_ray(const BatchRays& r, size_t i, double no_limits, D3& s, D3& d, double& lim) {
    fetch_ray(r, i, s, d);
    lim = r.limits ? r.limits[i] : no_limits;
}

// the fp32 frame of a ray (start already clipped to the root box) for the private binary walk: the slab terms and the records' pre-test
// (filled in place: a returned struct costs k_nr_walk two VGPRs)
struct SlabRay { f2 I01, I20, I12, B0, B1, B2; RayF rf; };
__device__ __forceinline__ void set_slab_ray(const DevScene& sc, D3 s, D3 d, SlabRay& r) {
    const float ox = (float)(s.x - sc.root.centre[0]), oy = (float)(s.y - sc.root.centre[1]), oz = (float)(s.z - sc.root.centre[2]);
    const float ix = slab_inv((float)d.x), iy = slab_inv((float)d.y), iz = slab_inv((float)d.z);
    r.I01 = (f2){ix, iy}; r.I20 = (f2){iz, ix}; r.I12 = (f2){iy, iz};
    r.B0 = (f2){-ox * ix, -oy * iy}; r.B1 = (f2){-oz * iz, -ox * ix}; r.B2 = (f2){-oy * iy, -oz * iz};
    r.rf = make_ray_f(sc, s, d);
}
// the fp32 cull bound of a walk from the FP64 room = bound - offset: a hit counts <=> fl(t + offset) <= bound, nothing beyond t = room,
// inflated by 2^-20, can (bvh_intersect<true>)
__device__ __forceinline__ float cull_tlim(double room) { return (float)room * (1.0f + 9.5367431640625e-7f) + 1e-30f; }

// The node step of the private binary walk ("while-while": two pending leaves, the far inner child pushed, a pop when neither is hit).
// The one other copy is bvh_intersect's own (sr_trace.h).  h0 / h1: the child is hit; first0: child 0 is the nearer one.  The children that
// are hit leaves become the pending leaves, nearer first (leafA < 0 and leafB < 0 on entry); ni: the next inner node (-1: the walk is over);
// a far child is re-tested against the bound when it is popped.  (k_cp_walk, sr_closest.hip, has its own step: its stack word carries a bound)
template <class StackT>
__device__ __forceinline__ void walk_step(const BvhNode& n, bool h0, bool h1, bool first0, StackT& st, int& sp, int32_t& ni, int32_t& leafA, int32_t& leafB) {
    const bool l0 = h0 && n.n0 > 0, l1 = h1 && n.n1 > 0;
    if (l0 && l1) {
        leafA = (first0 ? n.c0 : n.c1) | ((first0 ? n.n0 : n.n1) << kLeafShift);
        leafB = (first0 ? n.c1 : n.c0) | ((first0 ? n.n1 : n.n0) << kLeafShift);
    } else if (l0) leafA = n.c0 | (n.n0 << kLeafShift);
    else if (l1) leafA = n.c1 | (n.n1 << kLeafShift);
    const bool i0 = h0 && n.n0 == 0, i1 = h1 && n.n1 == 0;
    if (i0 && i1) {
        st.put(sp++, first0 ? n.c1 : n.c0);
        ni = first0 ? n.c0 : n.c1;
    } else if (i0) ni = n.c0;
    else if (i1) ni = n.c1;
    else ni = (sp > 0) ? st.get(--sp) : -1;
}
// what walk_step wants to know of a ray at node n: its children's boxes against the ray's slabs and the cull bound tlim
__device__ __forceinline__ void ray_node_hits(const BvhNode& n, const SlabRay& r, float tlim, bool& h0, bool& h1, bool& first0) {
    float t0, x0, t1, x1;
    node_slabs(n, r.I01, r.I20, r.I12, r.B0, r.B1, r.B2, t0, x0, t1, x1);
    h0 = n.n0 >= 0 && t0 <= x0 && x0 >= 0.0f && t0 <= tlim;
    h1 = n.n1 >= 0 && t1 <= x1 && x1 >= 0.0f && t1 <= tlim;
    first0 = t0 <= t1;
}

// the statistics epilogue of a kernel with one lane per item: every thread of the workgroup must call it
__device__ __forceinline__ void block_stat_add(unsigned long long* stats, const Ctr& c) {
    const uint32_t r = wave_sum(c.rays), g = wave_sum(c.geom), n = wave_sum(c.nodes), l = wave_sum(c.leaves);
    block_stat_add(&stats[0], &stats[1], &stats[2], &stats[3], r, g, n, l);
}

// ---- the point calls (sr_closest.hip, sr_near.hip; sr_overlap.hip takes cp_stat_add): what their walks and loops share
// (d2, j) of one triangle against the running best: a NaN d2 fails both comparisons, equal d2 goes to the lower TriangleIndex
__device__ __forceinline__ bool cp_better(double d2, int32_t j, double best, int32_t bj) { return d2 < best || (d2 == best && j < bj); }

// block_stat_add's sums (sr_trace.h) in the first four words of the kernel's DYNAMIC LDS (`lds`: its base) instead of a static array: the
// walk's stacks are dead once every lane has arrived, and at the depth limit they are the whole 64 KiB a workgroup may ask for.  Every
// thread must call it.
__device__ __forceinline__ void cp_stat_add(unsigned char* lds, unsigned long long* stats, const Ctr& c) {
    unsigned int* acc = reinterpret_cast<unsigned int*>(lds);
    const uint32_t r = wave_sum(c.rays), g = wave_sum(c.geom), n2 = wave_sum(c.nodes), l2 = wave_sum(c.leaves);
    __syncthreads();                                                      // no lane reads its stack any more
    if (threadIdx.x < 4) acc[threadIdx.x] = 0u;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        if (r) atomicAdd(&acc[0], r);
        if (g) atomicAdd(&acc[1], g);
        if (n2) atomicAdd(&acc[2], n2);
        if (l2) atomicAdd(&acc[3], l2);
    }
    __syncthreads();
    if (threadIdx.x == 0) { stat_add(&stats[0], acc[0]); stat_add(&stats[1], acc[1]); stat_add(&stats[2], acc[2]); stat_add(&stats[3], acc[3]); }
}

// fp32 lower bound of the squared distance from the point (p = (float)(q - centre), e = 2^-23 |p| per axis) to the stored box [lo, hi]:
// per axis the gap max(lo - p, p - hi, 0) less e, squared and summed, times (1 - 2^-19).  DESIGN 5.32 proves that it is at most the FP64
// d2 of every triangle below the box whose closest point the routine placed inside the triangle.
__device__ __forceinline__ float cp_bound(const float lo[3], const float hi[3], float px, float py, float pz, float ex, float ey, float ez) {
    const float gx = fmaxf(fmaxf(fmaxf(lo[0] - px, px - hi[0]), 0.0f) - ex, 0.0f);
    const float gy = fmaxf(fmaxf(fmaxf(lo[1] - py, py - hi[1]), 0.0f) - ey, 0.0f);
    const float gz = fmaxf(fmaxf(fmaxf(lo[2] - pz, pz - hi[2]), 0.0f) - ez, 0.0f);
    return (gx * gx + gy * gy + gz * gz) * (1.0f - 1.9073486328125e-6f);
}
// the fp32 value a bound must EXCEED to cull: at least `cull` whatever the rounding (an overflow gives +inf: nothing is culled)
__device__ __forceinline__ float cp_cullf(double cull) { return (float)cull * (1.0f + 2.384185791015625e-7f) + 1e-30f; }

// ---- host ------------------------------------------------------------------------------------------------------------------------------
// per-lane traversal stack levels of a private walk in `mode` (x 256 lanes x 4 bytes of LDS)
inline int stack_levels(const DevScene& sc, int mode) {
    if (mode == MODE_REF) return sc.rdepth + 2;
    if (mode == MODE_BVH) return sc.bdepth + 2;
    return 1;
}

inline BatchRays batch_rays(const double* starts, const double* dirs, const double* limits, bool endpoints) { return BatchRays{starts, dirs, limits, endpoints ? 1 : 0}; }

// L.sort_buf of an ordered pass: the sort's keys, the sorted keys, the indices, the order, and the work head of a persistent walk
struct PassBuffers { unsigned int *keys, *keys2, *idx, *order, *head; };

// The passes of a call, back to back on the stream.  ordered: order_pass(first, count, buffers) orders a pass first (timed as sort_id) and
// the slice carries that order; otherwise a pass runs in input order with take 2.  walk_pass(slice, buffers) launches the pass (walk_id)
template <class Order, class Walk>
hipError_t run_passes(const BatchLaunch& L, bool ordered, int sort_id, int walk_id, Order order_pass, Walk walk_pass) {
    const unsigned int cap = (unsigned int)((L.pass + 255) / 256 * 256);
    PassBuffers b{};
    if (ordered) { b.keys = L.sort_buf; b.keys2 = b.keys + cap; b.idx = b.keys2 + cap; b.order = b.idx + cap; b.head = b.order + cap; }
    for (int64_t first = 0; first < L.n; first += L.pass) {
        PassSlice p{first, (unsigned int)std::min<int64_t>(L.pass, L.n - first), nullptr, nullptr, 0u, 2};
        hipError_t e;
        if (ordered) {
            if ((e = timed(L, sort_id, [&] { return order_pass(first, p.count, b); })) != hipSuccess) return e;
            p.order = b.order; p.keys = b.keys2; p.skip_mask = point_order_skip_mask(!L.input_order);
        }
        if ((e = timed(L, walk_id, [&] { return walk_pass(p, b); })) != hipSuccess) return e;
    }
    return hipSuccess;
}

// occl_order for a pass of a ray call
inline hipError_t order_ray_pass(const BatchLaunch& L, const BatchRays& r, const RootBox& root, int64_t first, unsigned int count, const PassBuffers& b) {
    return occl_order(r.starts + 3 * first, r.dirs + 3 * first, r.limits ? r.limits + first : nullptr, count, r.endpoints != 0, !L.input_order, root, b.keys, b.keys2,
                      b.idx, b.order, L.sort_temp, L.sort_temp_bytes, L.stream);
}

// The order of a pass of a point call (sr_closest.hip defines it: k_cp_keys + the radix sort): the regular points (closest_regular) first --
// sorted by the Morton cell in `root`, or in input order (L.input_order) -- then the others in input order
hipError_t cp_order(const BatchLaunch& L, const RootBox& root, const double* points, unsigned int n, const PassBuffers& b);

// a launch with one lane per item of the slice
inline dim3 lane_grid(const PassSlice& p) { return dim3((p.count + 255u) / 256u); }

}  // namespace sr
