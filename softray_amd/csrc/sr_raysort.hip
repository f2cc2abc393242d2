// sr_raysort.hip -- coherence for the incoherent: the ray queue of a bounce level is ordered by (cell of the origin, direction
// octant) before k_bounce walks it, so that the lanes of a wave start in the same part of the tree and head the same way
// (neighbouring lanes then fetch the same nodes and records: cache hits instead of HBM round trips).  The order is a
// permutation of queue indices (the queue itself stays where it is); which lane traces which ray changes nothing a pixel
// depends on.  Key = 7 bits per axis of the origin's cell in the root box, Morton-interleaved, with the 3 bits of direction signs between the coarse 15 and the fine 6 cell bits
// (24 bits: three 8-bit radix passes of rocPRIM's device sort through hipCUB).  Entries beyond the queue's device-side count
// get the largest key and stay at the end.
#include <hipcub/hipcub.hpp>

#include "sr_device.h"

namespace sr {
namespace {

__device__ __forceinline__ unsigned int spread7(unsigned int v) {          // 7 bits -> every third bit
    v &= 0x7fu;
    v = (v | (v << 8)) & 0x700fu;
    v = (v | (v << 4)) & 0x430c3u;
    v = (v | (v << 2)) & 0x49249u;
    return v;
}

// queue records are 64 bytes: double origin[3], double direction[3], ... (HitRec of sr_pipeline.hip)
__global__ __launch_bounds__(256) void k_ray_keys(const double* __restrict__ queue, const unsigned int* __restrict__ count, unsigned int cap,
                                                  double lx, double ly, double lz, double sx, double sy, double sz,
                                                  unsigned int* __restrict__ keys, unsigned int* __restrict__ idx) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= cap) return;
    unsigned int key = 0xffffffffu;
    if (i < *count) {
        const double* q = queue + (size_t)i * 8;
        const int cx = min(127, max(0, (int)((q[0] - lx) * sx))), cy = min(127, max(0, (int)((q[1] - ly) * sy))), cz = min(127, max(0, (int)((q[2] - lz) * sz)));
        const unsigned int oct = (q[3] < 0.0 ? 1u : 0u) | (q[4] < 0.0 ? 2u : 0u) | (q[5] < 0.0 ? 4u : 0u);
        // the direction octant sits between the coarse cell bits (32^3 cells) and the fine ones: rays of a coarse cell that head the same way
        // come first together, then spread over the cell (against octant-last: -1 %, against octant-first: -6 % at C5)
        const unsigned int mort = (spread7((unsigned)cx) << 2) | (spread7((unsigned)cy) << 1) | spread7((unsigned)cz);
        key = ((mort >> 6) << 9) | (oct << 6) | (mort & 63u);
    }
    keys[i] = key;
    idx[i] = i;
}

// sr_shadow_points: the records of a pass lie where their points do (record i = point i, 64 bytes: position, normal, then the sample word);
// a point that is not queued has the sample word 0xffffffff.  sorted: the key of k_ray_keys from position and normal; in both cases bit
// kPointSkipBit marks the records that are not queued, so that a STABLE sort leaves the queued ones first -- by key, ties in input order
// (sorted), or simply in input order (!sorted: the one-bit sort is a deterministic compaction)
constexpr int kPointSkipBit = 24;
__global__ __launch_bounds__(256) void k_point_keys(const double* __restrict__ recs, unsigned int n, int sorted, double lx, double ly, double lz,
                                                    double sx, double sy, double sz, unsigned int* __restrict__ keys, unsigned int* __restrict__ idx) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double* q = recs + (size_t)i * 8;
    const bool queued = reinterpret_cast<const unsigned int*>(q + 6)[0] != 0xffffffffu;
    unsigned int key = 0u;
    if (queued && sorted) {
        const int cx = min(127, max(0, (int)((q[0] - lx) * sx))), cy = min(127, max(0, (int)((q[1] - ly) * sy))), cz = min(127, max(0, (int)((q[2] - lz) * sz)));
        const unsigned int oct = (q[3] < 0.0 ? 1u : 0u) | (q[4] < 0.0 ? 2u : 0u) | (q[5] < 0.0 ? 4u : 0u);
        const unsigned int mort = (spread7((unsigned)cx) << 2) | (spread7((unsigned)cy) << 1) | spread7((unsigned)cz);
        key = ((mort >> 6) << 9) | (oct << 6) | (mort & 63u);
    }
    if (!queued) key = sorted ? (1u << kPointSkipBit) : 1u;
    keys[i] = key;
    idx[i] = i;
}

__device__ __forceinline__ unsigned int spread12(unsigned int v) {         // 12 bits -> every second bit
    v &= 0xfffu;
    v = (v | (v << 8)) & 0x00ff00ffu;
    v = (v | (v << 4)) & 0x0f0f0f0fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

// sr_trace_origin_rays: the rays of a pass share their origin, so a ray's place among its neighbours is its direction alone.  Key = the cell
// of d / (|dx| + |dy| + |dz|) in the octahedral map (the lower hemisphere folded over the diagonals), 2^12 cells per axis, Morton-interleaved:
// 24 bits.  Bit kPointSkipBit (sorted) / bit 0 (!sorted) marks an IRREGULAR ray -- a component that is not finite, or max |d_k| outside
// [2^-40, 2^40] -- which the packet walk never sees: the stable sort leaves those at the end of the pass, in input order.
__global__ __launch_bounds__(256) void k_dir_keys(const double* __restrict__ dirs, unsigned int n, int sorted, unsigned int* __restrict__ keys,
                                                  unsigned int* __restrict__ idx) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double dx = dirs[(size_t)i * 3], dy = dirs[(size_t)i * 3 + 1], dz = dirs[(size_t)i * 3 + 2];
    const double ax = fabs(dx), ay = fabs(dy), az = fabs(dz);
    const double m = fmax(fmax(ax, ay), az);
    // (a NaN component fails the first three comparisons, an infinite one the fifth)
    const bool regular = ax == ax && ay == ay && az == az && m >= 0x1p-40 && m <= 0x1p40;
    unsigned int key = 0u;
    if (regular && sorted) {
        const double inv = 1.0 / (ax + ay + az);
        double u = dx * inv, v = dy * inv;
        if (dz < 0.0) {
            const double fu = (1.0 - fabs(v)) * (u < 0.0 ? -1.0 : 1.0), fv = (1.0 - fabs(u)) * (v < 0.0 ? -1.0 : 1.0);
            u = fu; v = fv;
        }
        const int cu = min(4095, max(0, (int)((u + 1.0) * 2048.0))), cv = min(4095, max(0, (int)((v + 1.0) * 2048.0)));
        key = (spread12((unsigned)cu) << 1) | spread12((unsigned)cv);
    }
    if (!regular) key = sorted ? (1u << kPointSkipBit) : 1u;
    keys[i] = key;
    idx[i] = i;
}

// sr_occluded_rays: arbitrary rays as three arrays (starts, dirs or end points, limits).  Key = k_ray_keys' key of (start, direction): the
// 7-bit Morton cell of the start in the root box with the direction's octant between the coarse and the fine bits.  Bit kPointSkipBit (sorted)
// / bit 0 (!sorted) marks an IRREGULAR ray -- a start that is not finite or beyond 2^100, a limit that is NaN or -inf, a direction that is
// irregular by k_dir_keys' rule (a zero-length segment among them) -- which the any-hit walk never sees: the stable sort leaves those at the
// end of the pass, in input order.
__global__ __launch_bounds__(256) void k_occl_keys(const double* __restrict__ starts, const double* __restrict__ dirs, const double* __restrict__ limits,
                                                   unsigned int n, int endpoints, int sorted, double lx, double ly, double lz, double sx, double sy, double sz,
                                                   unsigned int* __restrict__ keys, unsigned int* __restrict__ idx) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double px = starts[(size_t)i * 3], py = starts[(size_t)i * 3 + 1], pz = starts[(size_t)i * 3 + 2];
    double dx = dirs[(size_t)i * 3], dy = dirs[(size_t)i * 3 + 1], dz = dirs[(size_t)i * 3 + 2];
    if (endpoints) { dx = dx - px; dy = dy - py; dz = dz - pz; }                    // the subtraction k_occluded does
    const double lim = limits ? limits[i] : 1.0;
    const double ax = fabs(dx), ay = fabs(dy), az = fabs(dz);
    const double m = fmax(fmax(ax, ay), az);
    // (a NaN component fails the comparison with itself, an infinite one the upper bound; a NaN limit fails lim >= -DBL_MAX, and so does -inf)
    const bool dir_ok = ax == ax && ay == ay && az == az && m >= 0x1p-40 && m <= 0x1p40;
    const bool start_ok = fabs(px) <= 0x1p100 && fabs(py) <= 0x1p100 && fabs(pz) <= 0x1p100;
    const bool regular = dir_ok && start_ok && lim >= -1.7976931348623157e308;
    unsigned int key = 0u;
    if (regular && sorted) {
        const int cx = (int)fmin(127.0, fmax(0.0, (px - lx) * sx)), cy = (int)fmin(127.0, fmax(0.0, (py - ly) * sy)), cz = (int)fmin(127.0, fmax(0.0, (pz - lz) * sz));
        const unsigned int oct = (dx < 0.0 ? 1u : 0u) | (dy < 0.0 ? 2u : 0u) | (dz < 0.0 ? 4u : 0u);
        const unsigned int mort = (spread7((unsigned)cx) << 2) | (spread7((unsigned)cy) << 1) | spread7((unsigned)cz);
        key = ((mort >> 6) << 9) | (oct << 6) | (mort & 63u);
    }
    if (!regular) key = sorted ? (1u << kPointSkipBit) : 1u;
    keys[i] = key;
    idx[i] = i;
}

}  // namespace

hipError_t occl_order(const double* starts, const double* dirs, const double* limits, unsigned int n, bool endpoints, bool sorted, const RootBox& root,
                      unsigned int* keys, unsigned int* keys2, unsigned int* idx, unsigned int* order_out, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    double s[3];
    for (int a = 0; a < 3; ++a) { const double e = root.max[a] - root.min[a]; s[a] = e > 0 ? 128.0 / e : 0.0; }
    hipLaunchKernelGGL(k_occl_keys, dim3((n + 255u) / 256u), dim3(256), 0, stream, starts, dirs, limits, n, endpoints ? 1 : 0, sorted ? 1 : 0, root.min[0], root.min[1],
                       root.min[2], s[0], s[1], s[2], keys, idx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, (const unsigned int*)keys, keys2, (const unsigned int*)idx, order_out, (int)n, 0,
                                              sorted ? kPointSkipBit + 1 : 1, stream);
}

hipError_t dir_order(const double* dirs, unsigned int n, bool sorted, unsigned int* keys, unsigned int* keys2, unsigned int* idx, unsigned int* order_out,
                     void* temp, size_t temp_bytes, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dir_keys, dim3((n + 255u) / 256u), dim3(256), 0, stream, dirs, n, sorted ? 1 : 0, keys, idx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, (const unsigned int*)keys, keys2, (const unsigned int*)idx, order_out, (int)n, 0,
                                              sorted ? kPointSkipBit + 1 : 1, stream);
}

unsigned int point_order_skip_mask(bool sorted) { return sorted ? (1u << kPointSkipBit) : 1u; }

size_t point_order_temp_bytes(unsigned int cap) {
    size_t a = 0, b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const unsigned int*)nullptr, (unsigned int*)nullptr, (const unsigned int*)nullptr,
                                             (unsigned int*)nullptr, (int)cap, 0, kPointSkipBit + 1);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const unsigned int*)nullptr, (unsigned int*)nullptr, (const unsigned int*)nullptr,
                                             (unsigned int*)nullptr, (int)cap, 0, 1);
    return a > b ? a : b;
}

// order_out[j] = the point whose record is the j-th of the pass's queue, keys2[j] its key; keys / idx: scratch of n entries each
hipError_t point_order(const void* recs, unsigned int n, bool sorted, const RootBox& root, unsigned int* keys, unsigned int* keys2, unsigned int* idx,
                       unsigned int* order_out, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    double s[3];
    for (int a = 0; a < 3; ++a) { const double e = root.max[a] - root.min[a]; s[a] = e > 0 ? 128.0 / e : 0.0; }
    hipLaunchKernelGGL(k_point_keys, dim3((n + 255u) / 256u), dim3(256), 0, stream, (const double*)recs, n, sorted ? 1 : 0, root.min[0], root.min[1], root.min[2],
                       s[0], s[1], s[2], keys, idx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, (const unsigned int*)keys, keys2, (const unsigned int*)idx, order_out, (int)n, 0,
                                              sorted ? kPointSkipBit + 1 : 1, stream);
}

size_t ray_sort_temp_bytes(unsigned int cap) {
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const unsigned int*)nullptr, (unsigned int*)nullptr, (const unsigned int*)nullptr,
                                             (unsigned int*)nullptr, (int)cap, 0, 24);
    return bytes;
}

// order_out[j] = index of the j-th ray in key order; keys / keys2 / idx: scratch of `cap` entries each
hipError_t ray_sort(const void* queue, const unsigned int* d_count, unsigned int cap, const RootBox& root, unsigned int* keys, unsigned int* keys2,
                    unsigned int* idx, unsigned int* order_out, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (cap == 0) return hipSuccess;
    double s[3];
    for (int a = 0; a < 3; ++a) { const double e = root.max[a] - root.min[a]; s[a] = e > 0 ? 128.0 / e : 0.0; }
    hipLaunchKernelGGL(k_ray_keys, dim3((cap + 255u) / 256u), dim3(256), 0, stream, (const double*)queue, d_count, cap, root.min[0], root.min[1], root.min[2],
                       s[0], s[1], s[2], keys, idx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // sorting all 32 key bits' low 24 keeps the 0xffffffff padding last as well (its low 24 bits are all ones, the largest digit in every pass)
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, (const unsigned int*)keys, keys2, (const unsigned int*)idx, order_out, (int)cap, 0, 24, stream);
}

}  // namespace sr
