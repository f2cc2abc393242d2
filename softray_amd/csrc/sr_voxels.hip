// sr_voxels.hip -- rayTraceVoxels (SR_F_VOXELS): the model as a 64^3 grid of coloured cells (Raytrace/TriMeshToVoxelGrid.cs,
// Raytrace/VoxelGrid.cs, Raytrace/LineWalker3D.cs).
//
//   voxeliser   count the cells of every triangle's box of cells -> exclusive scan -> (cell, triangle) pairs in triangle order -> STABLE
//               radix sort by cell (18 key bits): every cell's list is contiguous and in ascending triangle index -> one lane per cell adds
//               the channels in list order.  No atomic's arrival order decides a sum; the work is O(pairs), not O(cells x triangles).
//   k_voxel_walk  one lane per camera sample: ray generation of k_primary, the reference's fixed-step walk with `pos += delta` accumulated
//               step by step, ShadingMethod on the hit's normal with pos = (0, 0, 0).  The 64^3 occupancy bits (32 KB) are staged in LDS,
//               so a step is three FP64 adds, three conversions and one LDS bit test; the colour and normal tables are read once per hit.
//   k_voxel_trace the same walk for a batch of rays (SR_TARGET_VOXELS).
//
// FP64 throughout, compiled with -ffp-contract=off: the cells a walk visits depend on every rounding.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "sr_trace.h"

namespace sr {
namespace {

constexpr int kG = kVoxelGrid;                       // 64
constexpr int kCells = kG * kG * kG;
constexpr int kMaskWords = kCells / 32;              // 8192 words = 32 KB
static_assert(kG == 64, "the cell index packs three 6-bit coordinates");

// plane k of an axis: k / 64 - 0.5, exact in FP64 (TriMeshToVoxelGrid.cs:28-29)
__device__ __forceinline__ double cell_plane(int k) { return (double)k / (double)kG - 0.5; }

// The cells [lo, hi] of one axis that a triangle with vertex range [mn, mx] is in: max >= k/64 - 0.5 and min <= (k+1)/64 - 0.5
// (FindTrianglesInsidePlanes with axis normals: v.n >= d, exact, no epsilon).  An estimate from the scaled coordinate, then corrected
// with the exact comparisons, so the result is the one a test of all 64 cells gives.
__device__ __forceinline__ void axis_cells(double mn, double mx, int& lo, int& hi) {
    double e = floor((mx + 0.5) * (double)kG);
    hi = e < -1.0 ? -1 : (e > (double)(kG - 1) ? kG - 1 : (int)e);           // (a NaN compares false twice: (int)NaN is not reached for finite models)
    while (hi + 1 <= kG - 1 && cell_plane(hi + 1) <= mx) ++hi;
    while (hi >= 0 && !(cell_plane(hi) <= mx)) --hi;
    e = ceil((mn + 0.5) * (double)kG) - 1.0;
    lo = e < 0.0 ? 0 : (e > (double)kG ? kG : (int)e);
    while (lo - 1 >= 0 && cell_plane(lo) >= mn) --lo;
    while (lo <= kG - 1 && !(cell_plane(lo + 1) >= mn)) ++lo;
}

struct CellBox { int lo[3], hi[3]; };
__device__ __forceinline__ unsigned int tri_cells(const double* __restrict__ v, CellBox& b) {
    unsigned int n = 1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double p = v[a], q = v[3 + a], r = v[6 + a];
        const double mn = fmin(p, fmin(q, r)), mx = fmax(p, fmax(q, r));
        axis_cells(mn, mx, b.lo[a], b.hi[a]);
        n *= b.hi[a] >= b.lo[a] ? (unsigned int)(b.hi[a] - b.lo[a] + 1) : 0u;
    }
    return n;
}

__global__ __launch_bounds__(256) void k_vox_count(const double* __restrict__ v9, int ntris, unsigned long long* __restrict__ counts) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= ntris) return;
    CellBox b;
    counts[t] = tri_cells(v9 + (size_t)t * 9, b);
}

// one wave per triangle: its lanes write the (cell, triangle) pairs of the triangle's box, x outer, z inner
__global__ __launch_bounds__(256) void k_vox_emit(const double* __restrict__ v9, int ntris, const unsigned long long* __restrict__ offsets,
                                                  unsigned int* __restrict__ keys, unsigned int* __restrict__ vals) {
    const int lane = threadIdx.x & 63;
    const int waves = gridDim.x * 4;
    for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < ntris; t += waves) {
        CellBox b;
        const unsigned int n = tri_cells(v9 + (size_t)t * 9, b);
        if (n == 0) continue;
        const unsigned int ny = (unsigned)(b.hi[1] - b.lo[1] + 1), nz = (unsigned)(b.hi[2] - b.lo[2] + 1);
        const unsigned int base = (unsigned int)offsets[t];           // (the caller refuses totals beyond 2^30)
        for (unsigned int j = (unsigned)lane; j < n; j += 64u) {
            const unsigned int x = j / (ny * nz), r = j - x * ny * nz, y = r / nz, z = r - y * nz;
            keys[base + j] = (((unsigned)b.lo[0] + x) * kG + ((unsigned)b.lo[1] + y)) * kG + ((unsigned)b.lo[2] + z);
            vals[base + j] = (unsigned int)t;
        }
    }
}

// first / one-past-last position of every cell's run in the sorted pairs (both tables zeroed before: an empty cell keeps 0, 0)
__global__ __launch_bounds__(256) void k_vox_bounds(const unsigned int* __restrict__ keys, unsigned int npairs, unsigned int* __restrict__ first,
                                                    unsigned int* __restrict__ last) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npairs) return;
    const unsigned int k = keys[i];
    if (k >= (unsigned)kCells) return;
    if (i == 0 || keys[i - 1] != k) first[k] = i;
    if (i + 1 == npairs || keys[i + 1] != k) last[k] = i + 1;
}

// one lane per cell (TriMeshToVoxelGrid.cs:60-87): Color.Black += Color(argb) over the cell's triangles in ascending index, /= count, ToARGB;
// the normal of the lowest-index triangle; the occupancy bit (colour != 0) of 64 consecutive cells = one ballot
__global__ __launch_bounds__(256) void k_vox_reduce(const Rec128* __restrict__ tris, const unsigned int* __restrict__ vals, const unsigned int* __restrict__ first,
                                                    const unsigned int* __restrict__ last, uint32_t* __restrict__ colors, double* __restrict__ normals,
                                                    uint32_t* __restrict__ mask) {
    const unsigned int cell = blockIdx.x * 256u + threadIdx.x;               // grid = kCells / 256 exactly
    const unsigned int a = first[cell], b = last[cell];
    uint32_t color = 0u;
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (b > a) {
        double r = 0.0, g = 0.0, bl = 0.0;
        for (unsigned int i = a; i < b; ++i) {
            const uint32_t c = tris[vals[i]].color;
            r = r + (double)((c >> 16) & 0xffu) / 255.0;                       // Color(uint), Color.cs:31-36
            g = g + (double)((c >> 8) & 0xffu) / 255.0;
            bl = bl + (double)(c & 0xffu) / 255.0;
        }
        const double n = (double)(int)(b - a);
        r = r / n; g = g / n; bl = bl / n;
        color = (255u << 24) + (((uint32_t)(int)(r * 255.0) & 0xffu) << 16) + (((uint32_t)(int)(g * 255.0) & 0xffu) << 8) + ((uint32_t)(int)(bl * 255.0) & 0xffu);
        const Rec128* t0 = &tris[vals[a]];
        nx = t0->p[0]; ny = t0->p[1]; nz = t0->p[2];
    }
    colors[cell] = color;
    normals[(size_t)cell * 3] = nx; normals[(size_t)cell * 3 + 1] = ny; normals[(size_t)cell * 3 + 2] = nz;
    const unsigned long long m = __ballot(color != 0u);
    if ((threadIdx.x & 63) == 0) { mask[cell >> 5] = (uint32_t)m; mask[(cell >> 5) + 1] = (uint32_t)(m >> 32); }
}

// ---------------------------------------------------------------------------------------------------------------------
// the walk (VoxelGrid.IntersectRay :125-177, LineWalker3D.WalkLine :17-35)
// ---------------------------------------------------------------------------------------------------------------------
// LDSMASK: `occ` points to the occupancy bits in LDS; otherwise it is nullptr and a step reads the colour table itself
template <bool LDSMASK>
__device__ __forceinline__ bool voxel_walk(const RootBox& box, const uint32_t* occ, const uint32_t* __restrict__ colors, D3 start, D3 dir, int& cell_out) {
    D3 end = start + dir * 10.0;
    if (!clip_segment<true>(box, start, end)) return false;              // AxisAlignedBox((-1,-1,-1), (1,1,1)).ClipLineSegment
    const double scale = (double)kG - 0.001;
    const D3 half = mk(0.5, 0.5, 0.5);
    start = (start * 0.5 + half) * scale;
    end = (end * 0.5 + half) * scale;
    D3 delta = end - start;
    const double eps = 1e-10;                                              // Vector.IsZeroVector
    if (-eps < delta.x && delta.x < eps && -eps < delta.y && delta.y < eps && -eps < delta.z && delta.z < eps) return false;
    const double ax = fabs(delta.x), ay = fabs(delta.y), az = fabs(delta.z);
    const double axy = ax > ay ? ax : ay, max_dim = axy > az ? axy : az;
    int steps = (int)(max_dim / 0.1);
    steps = steps > 1 ? steps : 1;
    delta = delta * (0.1 / max_dim);
    D3 pos = start;
    for (int s = 0; s < steps; ++s) {
        int x = (int)pos.x, y = (int)pos.y, z = (int)pos.z;
        x = min(kG - 1, max(0, x)); y = min(kG - 1, max(0, y)); z = min(kG - 1, max(0, z));
        const int cell = (x * kG + y) * kG + z;
        // (`x != oldX && y != oldY && z != oldZ` is always true: old* stay -1, VoxelGrid.cs:142-153)
        const bool filled = LDSMASK ? ((occ[cell >> 5] >> (cell & 31)) & 1u) != 0u : colors[cell] != 0u;
        if (filled) { cell_out = cell; return true; }
        pos = pos + delta;
    }
    return false;
}

__device__ __forceinline__ void stage_mask(uint32_t* lds, const uint32_t* __restrict__ mask) {
    const uint4* src = reinterpret_cast<const uint4*>(mask);
    uint4* dst = reinterpret_cast<uint4*>(lds);
    for (int i = threadIdx.x; i < kMaskWords / 4; i += 256) dst[i] = src[i];
    __syncthreads();
}

// A persistent grid: every workgroup stages the mask once and then takes 16x16-pixel tiles blockIdx.x, blockIdx.x + gridDim.x, ...;
// a wave is an 8x8-pixel quadrant, as in k_primary.
template <bool LDSMASK, bool STATS>
__global__ __launch_bounds__(256) void k_voxel_walk(FrameConst fc, RootBox box, VoxelGridDev grid, const int32_t* __restrict__ row_map, int row_begin,
                                                    int row_count, uint32_t* __restrict__ samples, unsigned long long* stats) {
    __shared__ __attribute__((aligned(16))) uint32_t occ_lds[LDSMASK ? kMaskWords : 4];
    if (LDSMASK) stage_mask(occ_lds, grid.mask);
    const uint32_t* occ = LDSMASK ? occ_lds : nullptr;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tiles_x = (fc.width + 15) >> 4, tiles_y = (row_count + 15) >> 4;
    const int n = fc.sub_pixel_res, n2 = n * n;
    const int width = fc.width, height = fc.height;
    const bool blur = (fc.flags & 4u) != 0;
    const D3 start = mk(fc.start_world[0], fc.start_world[1], fc.start_world[2]);
    uint32_t rays = 0;
    for (int tile = blockIdx.x; tile < tiles_x * tiles_y; tile += gridDim.x) {
        const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
        const int col = tile_x * 16 + (wave & 1) * 8 + (lane & 7);
        const int brow = tile_y * 16 + (wave >> 1) * 8 + (lane >> 3);        // row inside this band
        if (!(col < width && brow < row_count)) continue;
        const int crow = row_begin + brow;                                   // compact row of the frame
        const int row = row_map[crow];
        // sample buffer: n == 1 -> the frame itself (final pixel position); n > 1 -> band-local [brow][col][n2] (k_resolve)
        const int out_row = (fc.strip_count > 0) ? crow : row;
        const size_t sbase = (n == 1) ? ((size_t)out_row * width + col) : (((size_t)brow * width + col) * n2);
        D3 focal = mk(0, 0, 0);
        if (n > 1 && blur) {
            D3 dv = mk(-((double)col / width - 0.5), -((double)row / height - 0.5) * fc.aspect, fc.fov_depth);
            focal = mul3x3(fc.it, dv) * fc.focal_depth + start;
        }
        for (int si = 0; si < n2; ++si) {                                    // subX outer, subY inner (Renderer.cs:1761-1763)
            const int sx = si / n, sy = si - sx * n;
            D3 ss = start, dw;
            if (n == 1) {                                                    // Renderer.cs:1722-1743
                D3 dv = mk(-((double)col / width - 0.5), -((double)row / height - 0.5) * fc.aspect, fc.fov_depth);
                dw = mul3x3(fc.it, dv);
            } else {
                double fx = (double)sx / (n - 1) - 0.5;
                double fy = (double)sy / (n - 1) - 0.5;
                if (blur) {
                    D3 sv = mk(fx / width * fc.focal_blur_strength, fy / height * fc.focal_blur_strength, -fc.position_z);
                    ss = mul3x3(fc.it, sv);
                    dw = focal - ss;
                } else {
                    D3 dv = mk(-((col + fx) / width - 0.5), -((row + fy) / height - 0.5) * fc.aspect, fc.fov_depth);
                    dw = mul3x3(fc.it, dv);
                }
            }
            rays++;
            int cell = 0;
            uint32_t color = fc.background;
            if (voxel_walk<LDSMASK>(box, occ, grid.colors, ss, dw, cell)) {
                color = grid.colors[cell];
                if (fc.flags & 1u) {                                         // ShadingMethod: pos = (0, 0, 0), the cell's normal
                    const double* nr = grid.normals + (size_t)cell * 3;
                    color = shade(fc, mk(0.0, 0.0, 0.0), mk(nr[0], nr[1], nr[2]), color);
                }
            }
            samples[sbase + si] = color;
        }
    }
    if (STATS) {
        // NumRaysFired per camera ray, NumGeometryTests += VoxelGrid.NumRayTests == 1; no nodes, no leaves
        const uint32_t a = wave_sum(rays);
        block_stat_add(&stats[0], &stats[1], &stats[2], &stats[3], a, a, 0u, 0u);
    }
}

__global__ __launch_bounds__(256) void k_voxel_trace(RootBox box, VoxelGridDev grid, long long n, const double* __restrict__ starts, const double* __restrict__ dirs,
                                                     uint8_t* hit, double* ray_frac, double* pos, double* normal, uint32_t* color, int32_t* tri, int32_t* counters) {
    __shared__ __attribute__((aligned(16))) uint32_t occ_lds[kMaskWords];
    stage_mask(occ_lds, grid.mask);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const D3 s = mk(starts[3 * i], starts[3 * i + 1], starts[3 * i + 2]);
        const D3 d = mk(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
        int cell = 0;
        const bool ok = voxel_walk<true>(box, occ_lds, grid.colors, s, d, cell);
        if (hit) hit[i] = ok ? 1 : 0;
        if (ray_frac) ray_frac[i] = 0.0;                                     // IntersectionInfo's defaults: the reference fills neither
        if (pos) { pos[3 * i] = 0.0; pos[3 * i + 1] = 0.0; pos[3 * i + 2] = 0.0; }
        if (normal) {
            const double* nr = grid.normals + (size_t)cell * 3;
            normal[3 * i] = ok ? nr[0] : 0.0; normal[3 * i + 1] = ok ? nr[1] : 0.0; normal[3 * i + 2] = ok ? nr[2] : 0.0;
        }
        if (color) color[i] = ok ? grid.colors[cell] : 0u;
        if (tri) tri[i] = -1;
        if (counters) { counters[3 * i] = 1; counters[3 * i + 1] = 0; counters[3 * i + 2] = 0; }
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------------
hipError_t voxel_count_cells(const double* d_v9, int ntris, unsigned long long* d_counts, unsigned long long* d_offsets, void* d_temp, size_t* temp_bytes, hipStream_t stream) {
    if (!d_temp) return hipcub::DeviceScan::ExclusiveSum(nullptr, *temp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, ntris);
    hipLaunchKernelGGL(k_vox_count, dim3((unsigned)((ntris + 255) / 256)), dim3(256), 0, stream, d_v9, ntris, d_counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceScan::ExclusiveSum(d_temp, *temp_bytes, (const unsigned long long*)d_counts, d_offsets, ntris, stream);
}

size_t voxel_sort_temp_bytes(unsigned int npairs) {
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const unsigned int*)nullptr, (unsigned int*)nullptr, (const unsigned int*)nullptr,
                                             (unsigned int*)nullptr, (int)npairs, 0, 18);
    return bytes;
}

hipError_t voxel_fill_grid(const double* d_v9, const Rec128* d_tris, int ntris, const unsigned long long* d_offsets, unsigned int npairs, unsigned int* d_pairs,
                           void* d_temp, size_t temp_bytes, unsigned int* d_first_last, const VoxelGridDev& grid, hipStream_t stream) {
    unsigned int* keys = d_pairs, *vals = d_pairs + (size_t)npairs, *keys2 = d_pairs + 2 * (size_t)npairs, *vals2 = d_pairs + 3 * (size_t)npairs;
    unsigned int* first = d_first_last, *last = d_first_last + kCells;
    hipError_t e = hipMemsetAsync(d_first_last, 0, (size_t)kCells * 2 * sizeof(unsigned int), stream);
    if (e != hipSuccess) return e;
    if (npairs > 0) {
        const unsigned int blocks = (unsigned)std::min<long long>(((long long)ntris + 3) / 4, 1 << 16);
        hipLaunchKernelGGL(k_vox_emit, dim3(blocks), dim3(256), 0, stream, d_v9, ntris, d_offsets, keys, vals);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        // a radix sort is stable: pairs of one cell keep the order they were emitted in, ascending triangle index
        e = hipcub::DeviceRadixSort::SortPairs(d_temp, temp_bytes, (const unsigned int*)keys, keys2, (const unsigned int*)vals, vals2, (int)npairs, 0, 18, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_vox_bounds, dim3((npairs + 255u) / 256u), dim3(256), 0, stream, (const unsigned int*)keys2, npairs, first, last);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_vox_reduce, dim3(kCells / 256), dim3(256), 0, stream, d_tris, (const unsigned int*)vals2, (const unsigned int*)first,
                       (const unsigned int*)last, grid.colors, grid.normals, grid.mask);
    return hipGetLastError();
}

hipError_t launch_voxel_frame(const VoxelLaunch& L) {
    const int n2 = L.fc.sub_pixel_res * L.fc.sub_pixel_res;
    for (int row_begin = 0; row_begin < L.fc.num_rows; row_begin += L.band_rows) {
        const int row_count = std::min(L.band_rows, L.fc.num_rows - row_begin);
        uint32_t* samples = (n2 == 1) ? L.pixels : L.samples;
        const long long tiles = (long long)((L.fc.width + 15) / 16) * ((row_count + 15) / 16);
        const unsigned int blocks = (unsigned)std::max<long long>(1, std::min<long long>(tiles, (long long)L.persistent_blocks));
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (L.get_events) L.get_events(L.user, K_VOXEL_WALK, &e0, &e1);
        hipError_t e;
        if (e0 && (e = hipEventRecord(e0, L.stream)) != hipSuccess) return e;
        const auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, L.stream, L.fc, L.box, L.grid, L.row_map, row_begin, row_count, samples, L.stats);
        };
        if (L.global_table) { if (L.stats) go(k_voxel_walk<false, true>); else go(k_voxel_walk<false, false>); }
        else { if (L.stats) go(k_voxel_walk<true, true>); else go(k_voxel_walk<true, false>); }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (e1 && (e = hipEventRecord(e1, L.stream)) != hipSuccess) return e;
        if (n2 > 1 && (e = launch_resolve_rows(L.fc, L.row_map, row_begin, row_count, L.samples, L.pixels, L.stream)) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_voxel_trace(const TraceLaunch& L, const RootBox& box, const VoxelGridDev& grid, int max_blocks) {
    if (L.n <= 0) return hipSuccess;
    const unsigned int blocks = (unsigned)std::max<long long>(1, std::min<long long>((L.n + 255) / 256, (long long)max_blocks));
    hipLaunchKernelGGL(k_voxel_trace, dim3(blocks), dim3(256), 0, L.stream, box, grid, (long long)L.n, L.starts, L.dirs, L.hit, L.ray_frac, L.pos, L.normal,
                       L.color, L.tri, L.counters);
    return hipGetLastError();
}

}  // namespace sr
