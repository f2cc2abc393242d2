// sr_voxels.hip -- rayTraceVoxels (SR_F_VOXELS): the model as an N^3 grid of coloured cells, N = sr_set_voxel_res in 1..256, default 64
// (Raytrace/TriMeshToVoxelGrid.cs, Raytrace/VoxelGrid.cs, Raytrace/LineWalker3D.cs).
//
//   voxeliser   count the cells of every triangle's box of cells -> exclusive scan -> (cell, triangle) pairs in triangle order -> STABLE
//               radix sort by cell (ceil(log2 N^3) key bits, 18 at N = 64): every cell's list is contiguous and in ascending triangle index
//               -> one lane per cell adds the channels in list order.  No atomic's arrival order decides a sum; the work is O(pairs), not
//               O(cells x triangles).  N > 64: k_vox_bricks packs the occupancy into one 64-bit word per brick of 4x4x4 cells + one bit per brick.
//   k_voxel_walk  one lane per camera sample: ray generation of k_primary, the reference's fixed-step walk with `pos += delta` accumulated
//               step by step, ShadingMethod on the hit's normal with pos = (0, 0, 0).  N <= 64: the N^3 occupancy bits (<= 32 KB) are staged
//               in LDS, so a step is three FP64 adds, three conversions and one LDS bit test; the colour and normal tables are read once per
//               hit.  N = 64 is its own instantiation with the grid size a compile-time constant.
//   k_voxel_walk2 N > 64: the brick bits (<= 64^3 = 32 KB) are staged in LDS; a step tests its brick's bit there and reads the brick's word
//               from global memory only when it enters a non-empty brick.  Every step is still taken, only its test is cheaper.
//   k_voxel_trace / k_voxel_trace2  the same walks for a batch of rays (SR_TARGET_VOXELS).
//
// FP64 throughout, compiled with -ffp-contract=off: the cells a walk visits depend on every rounding.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "sr_trace.h"

namespace sr {
namespace {

constexpr int kG = kVoxelGrid;                       // 64: the compile-time instantiation
constexpr int kMaskWords = kG * kG * kG / 32;        // 8192 words = 32 KB: the LDS mask of every walk (cells at N <= 64, bricks above)
static_assert(kVoxelGridMax <= 4 * kG, "the brick bits of the largest grid must fit the LDS mask");

// plane k of an axis: k / N - 0.5 as TriMeshToVoxelGrid.cs:28-29 writes it: a division, then a subtraction; both round unless N is a power of two
__device__ __forceinline__ double cell_plane(int k, int n) { return (double)k / (double)n - 0.5; }

// The cells [lo, hi] of one axis that a triangle with vertex range [mn, mx] is in: max >= plane(k) and min <= plane(k + 1)
// (FindTrianglesInsidePlanes with axis normals: v.n >= d, exact, no epsilon).  An estimate from the scaled coordinate, then corrected
// with the exact comparisons, so the result is the one a test of all N cells gives.
__device__ __forceinline__ void axis_cells(double mn, double mx, int n, int& lo, int& hi) {
    double e = floor((mx + 0.5) * (double)n);
    hi = e < -1.0 ? -1 : (e > (double)(n - 1) ? n - 1 : (int)e);             // (a NaN compares false twice: (int)NaN is not reached for finite models)
    while (hi + 1 <= n - 1 && cell_plane(hi + 1, n) <= mx) ++hi;
    while (hi >= 0 && !(cell_plane(hi, n) <= mx)) --hi;
    e = ceil((mn + 0.5) * (double)n) - 1.0;
    lo = e < 0.0 ? 0 : (e > (double)n ? n : (int)e);
    while (lo - 1 >= 0 && cell_plane(lo, n) >= mn) --lo;
    while (lo <= n - 1 && !(cell_plane(lo + 1, n) >= mn)) ++lo;
}

struct CellBox { int lo[3], hi[3]; };
__device__ __forceinline__ unsigned int tri_cells(const double* __restrict__ v, int g, CellBox& b) {
    unsigned int n = 1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double p = v[a], q = v[3 + a], r = v[6 + a];
        const double mn = fmin(p, fmin(q, r)), mx = fmax(p, fmax(q, r));
        axis_cells(mn, mx, g, b.lo[a], b.hi[a]);
        n *= b.hi[a] >= b.lo[a] ? (unsigned int)(b.hi[a] - b.lo[a] + 1) : 0u;
    }
    return n;
}

__global__ __launch_bounds__(256) void k_vox_count(const double* __restrict__ v9, int ntris, int g, unsigned long long* __restrict__ counts) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= ntris) return;
    CellBox b;
    counts[t] = tri_cells(v9 + (size_t)t * 9, g, b);
}

// one wave per triangle: its lanes write the (cell, triangle) pairs of the triangle's box, x outer, z inner
__global__ __launch_bounds__(256) void k_vox_emit(const double* __restrict__ v9, int ntris, int g, const unsigned long long* __restrict__ offsets,
                                                  unsigned int* __restrict__ keys, unsigned int* __restrict__ vals) {
    const int lane = threadIdx.x & 63;
    const int waves = gridDim.x * 4;
    for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < ntris; t += waves) {
        CellBox b;
        const unsigned int n = tri_cells(v9 + (size_t)t * 9, g, b);
        if (n == 0) continue;
        const unsigned int ny = (unsigned)(b.hi[1] - b.lo[1] + 1), nz = (unsigned)(b.hi[2] - b.lo[2] + 1);
        const unsigned int base = (unsigned int)offsets[t];           // (the caller refuses totals beyond 2^30)
        for (unsigned int j = (unsigned)lane; j < n; j += 64u) {
            const unsigned int x = j / (ny * nz), r = j - x * ny * nz, y = r / nz, z = r - y * nz;
            keys[base + j] = (((unsigned)b.lo[0] + x) * (unsigned)g + ((unsigned)b.lo[1] + y)) * (unsigned)g + ((unsigned)b.lo[2] + z);
            vals[base + j] = (unsigned int)t;
        }
    }
}

// first / one-past-last position of every cell's run in the sorted pairs (both tables zeroed before: an empty cell keeps 0, 0)
__global__ __launch_bounds__(256) void k_vox_bounds(const unsigned int* __restrict__ keys, unsigned int npairs, unsigned int cells,
                                                    unsigned int* __restrict__ first, unsigned int* __restrict__ last) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npairs) return;
    const unsigned int k = keys[i];
    if (k >= cells) return;
    if (i == 0 || keys[i - 1] != k) first[k] = i;
    if (i + 1 == npairs || keys[i + 1] != k) last[k] = i + 1;
}

// one lane per cell (TriMeshToVoxelGrid.cs:60-87): Color.Black += Color(argb) over the cell's triangles in ascending index, /= count, ToARGB;
// the normal of the lowest-index triangle; the occupancy bit (colour != 0) of 64 consecutive cells = one ballot.  N^3 is no multiple of 64
// for most N: the lanes past the last cell vote 0 and store nothing, and the mask has whole 64-bit words (voxel_mask_words).
__global__ __launch_bounds__(256) void k_vox_reduce(const Rec128* __restrict__ tris, const unsigned int* __restrict__ vals, const unsigned int* __restrict__ first,
                                                    const unsigned int* __restrict__ last, unsigned int cells, uint32_t* __restrict__ colors,
                                                    double* __restrict__ normals, uint32_t* __restrict__ mask) {
    const unsigned int cell = blockIdx.x * 256u + threadIdx.x;               // grid = ceil(cells / 256)
    const bool in = cell < cells;
    const unsigned int a = in ? first[cell] : 0u, b = in ? last[cell] : 0u;
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
    if (in) {
        colors[cell] = color;
        normals[(size_t)cell * 3] = nx; normals[(size_t)cell * 3 + 1] = ny; normals[(size_t)cell * 3 + 2] = nz;
    }
    const unsigned long long m = __ballot(color != 0u);
    if ((threadIdx.x & 63) == 0 && in) { mask[cell >> 5] = (uint32_t)m; mask[(cell >> 5) + 1] = (uint32_t)(m >> 32); }
}

// N > 64, after k_vox_reduce: a wave = a brick of 4x4x4 cells, the ballot = the brick's word (lane = (x&3)*16 + (y&3)*4 + (z&3); a cell
// beyond N votes 0), one bit per non-empty brick into the brick mask (zeroed before; an OR of bits has no order)
__global__ __launch_bounds__(256) void k_vox_bricks(const uint32_t* __restrict__ colors, int n, int nb, unsigned long long* __restrict__ bricks,
                                                    uint32_t* __restrict__ coarse) {
    const unsigned int b = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (b >= (unsigned)(nb * nb * nb)) return;                               // (a whole wave)
    const int lane = threadIdx.x & 63;
    const int bz = (int)(b % (unsigned)nb), by = (int)((b / (unsigned)nb) % (unsigned)nb), bx = (int)(b / (unsigned)(nb * nb));
    const int x = bx * 4 + (lane >> 4), y = by * 4 + ((lane >> 2) & 3), z = bz * 4 + (lane & 3);
    bool filled = false;
    if (x < n && y < n && z < n) filled = colors[((size_t)x * n + y) * n + z] != 0u;
    const unsigned long long w = __ballot(filled);
    if (lane == 0) {
        bricks[b] = w;
        if (w) atomicOr(&coarse[b >> 5], 1u << (b & 31u));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the walk (VoxelGrid.IntersectRay :125-177, LineWalker3D.WalkLine :17-35)
// ---------------------------------------------------------------------------------------------------------------------
// How a step learns whether its cell is filled.  All four visit the same positions and stop at the same first filled cell.
enum WalkMode {
    W_LDS = 0,      // N <= 64: `occ` = the occupancy bits of the cells in LDS
    W_TABLE = 1,    // SR_DBG_KERNEL_SWITCH 41: a step reads the colour table itself
    W_TWO = 2,      // N > 64: `occ` = the brick bits in LDS; the brick's 64-bit word is read on entering a non-empty brick and kept in registers
    W_FLAT = 3,     // SR_DBG_KERNEL_SWITCH 42: a step reads the row-major occupancy bits in global memory
};

// GC: the grid size as a compile-time constant (64), or 0 = grid.n
template <int GC, int MODE>
__device__ __forceinline__ bool voxel_walk(const RootBox& box, const uint32_t* occ, const VoxelGridDev& grid, D3 start, D3 dir, int& cell_out) {
    const int G = GC ? GC : grid.n;
    D3 end = start + dir * 10.0;
    if (!clip_segment<true>(box, start, end)) return false;              // AxisAlignedBox((-1,-1,-1), (1,1,1)).ClipLineSegment
    const double scale = (double)G - 0.001;
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
    int brick = -1;                                                        // W_TWO: the brick of `word`
    unsigned long long word = 0ull;
    const int nb = grid.nb;
    for (int s = 0; s < steps; ++s) {
        int x = (int)pos.x, y = (int)pos.y, z = (int)pos.z;
        x = min(G - 1, max(0, x)); y = min(G - 1, max(0, y)); z = min(G - 1, max(0, z));
        const int cell = (x * G + y) * G + z;
        // (`x != oldX && y != oldY && z != oldZ` is always true: old* stay -1, VoxelGrid.cs:142-153)
        bool filled;
        if (MODE == W_LDS) filled = ((occ[cell >> 5] >> (cell & 31)) & 1u) != 0u;
        else if (MODE == W_TABLE) filled = grid.colors[cell] != 0u;
        else if (MODE == W_FLAT) filled = ((grid.mask[cell >> 5] >> (cell & 31)) & 1u) != 0u;
        else {
            const int b = ((x >> 2) * nb + (y >> 2)) * nb + (z >> 2);
            if (b != brick) {                                              // about 40 steps in a row stay in one brick
                brick = b;
                word = ((occ[b >> 5] >> (b & 31)) & 1u) ? grid.bricks[b] : 0ull;
            }
            filled = ((word >> (((x & 3) << 4) | ((y & 3) << 2) | (z & 3))) & 1ull) != 0ull;
        }
        if (filled) { cell_out = cell; return true; }
        pos = pos + delta;
    }
    return false;
}

// `nvec` uint4 of a mask (voxel_mask_words / 4 <= kMaskWords / 4) into LDS
__device__ __forceinline__ void stage_mask(uint32_t* lds, const uint32_t* __restrict__ mask, int nvec) {
    const uint4* src = reinterpret_cast<const uint4*>(mask);
    uint4* dst = reinterpret_cast<uint4*>(lds);
    for (int i = threadIdx.x; i < nvec; i += 256) dst[i] = src[i];
    __syncthreads();
}
template <int GC, int MODE>
__device__ __forceinline__ const uint32_t* stage_for(uint32_t* lds, const VoxelGridDev& grid) {
    if (MODE == W_LDS) { stage_mask(lds, grid.mask, GC ? kMaskWords / 4 : (int)(voxel_mask_words(grid.n) / 4)); return lds; }
    if (MODE == W_TWO) { stage_mask(lds, grid.coarse, (int)(voxel_mask_words(grid.nb) / 4)); return lds; }
    return nullptr;
}

// A persistent grid: every workgroup stages the mask once and then takes 16x16-pixel tiles blockIdx.x, blockIdx.x + gridDim.x, ...;
// a wave is an 8x8-pixel quadrant, as in k_primary.
template <int GC, int MODE, bool STATS>
__device__ __forceinline__ void voxel_frame(const FrameConst& fc, const RootBox& box, const VoxelGridDev& grid, const uint32_t* occ,
                                            const int32_t* __restrict__ row_map, int row_begin, int row_count, uint32_t* __restrict__ samples,
                                            unsigned long long* stats) {
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
            if (voxel_walk<GC, MODE>(box, occ, grid, ss, dw, cell)) {
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

template <int GC, int MODE, bool STATS>
__global__ __launch_bounds__(256) void k_voxel_walk(FrameConst fc, RootBox box, VoxelGridDev grid, const int32_t* __restrict__ row_map, int row_begin,
                                                    int row_count, uint32_t* __restrict__ samples, unsigned long long* stats) {
    __shared__ __attribute__((aligned(16))) uint32_t occ_lds[MODE == W_LDS ? kMaskWords : 4];
    const uint32_t* occ = stage_for<GC, MODE>(occ_lds, grid);
    voxel_frame<GC, MODE, STATS>(fc, box, grid, occ, row_map, row_begin, row_count, samples, stats);
}

// N > 64: the two-level walk
template <bool STATS>
__global__ __launch_bounds__(256) void k_voxel_walk2(FrameConst fc, RootBox box, VoxelGridDev grid, const int32_t* __restrict__ row_map, int row_begin,
                                                     int row_count, uint32_t* __restrict__ samples, unsigned long long* stats) {
    __shared__ __attribute__((aligned(16))) uint32_t occ_lds[kMaskWords];
    const uint32_t* occ = stage_for<0, W_TWO>(occ_lds, grid);
    voxel_frame<0, W_TWO, STATS>(fc, box, grid, occ, row_map, row_begin, row_count, samples, stats);
}

template <int GC, int MODE>
__device__ __forceinline__ void voxel_trace(const RootBox& box, const VoxelGridDev& grid, const uint32_t* occ, long long n, const double* __restrict__ starts,
                                            const double* __restrict__ dirs, uint8_t* hit, double* ray_frac, double* pos, double* normal, uint32_t* color,
                                            int32_t* tri, int32_t* counters) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const D3 s = mk(starts[3 * i], starts[3 * i + 1], starts[3 * i + 2]);
        const D3 d = mk(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
        int cell = 0;
        const bool ok = voxel_walk<GC, MODE>(box, occ, grid, s, d, cell);
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

template <int GC, int MODE>
__global__ __launch_bounds__(256) void k_voxel_trace(RootBox box, VoxelGridDev grid, long long n, const double* __restrict__ starts, const double* __restrict__ dirs,
                                                     uint8_t* hit, double* ray_frac, double* pos, double* normal, uint32_t* color, int32_t* tri, int32_t* counters) {
    __shared__ __attribute__((aligned(16))) uint32_t occ_lds[MODE == W_LDS ? kMaskWords : 4];
    const uint32_t* occ = stage_for<GC, MODE>(occ_lds, grid);
    voxel_trace<GC, MODE>(box, grid, occ, n, starts, dirs, hit, ray_frac, pos, normal, color, tri, counters);
}

__global__ __launch_bounds__(256) void k_voxel_trace2(RootBox box, VoxelGridDev grid, long long n, const double* __restrict__ starts, const double* __restrict__ dirs,
                                                      uint8_t* hit, double* ray_frac, double* pos, double* normal, uint32_t* color, int32_t* tri, int32_t* counters) {
    __shared__ __attribute__((aligned(16))) uint32_t occ_lds[kMaskWords];
    const uint32_t* occ = stage_for<0, W_TWO>(occ_lds, grid);
    voxel_trace<0, W_TWO>(box, grid, occ, n, starts, dirs, hit, ray_frac, pos, normal, color, tri, counters);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------------
int voxel_key_bits(int n) {
    const unsigned int cells = (unsigned)n * n * n;                          // <= 2^24
    int bits = 1;
    while (bits < 32 && (1u << bits) < cells) ++bits;
    return bits;
}

hipError_t voxel_count_cells(const double* d_v9, int ntris, int g, unsigned long long* d_counts, unsigned long long* d_offsets, void* d_temp, size_t* temp_bytes, hipStream_t stream) {
    if (!d_temp) return hipcub::DeviceScan::ExclusiveSum(nullptr, *temp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, ntris);
    hipLaunchKernelGGL(k_vox_count, dim3((unsigned)((ntris + 255) / 256)), dim3(256), 0, stream, d_v9, ntris, g, d_counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceScan::ExclusiveSum(d_temp, *temp_bytes, (const unsigned long long*)d_counts, d_offsets, ntris, stream);
}

size_t voxel_sort_temp_bytes(unsigned int npairs, int key_bits) {
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const unsigned int*)nullptr, (unsigned int*)nullptr, (const unsigned int*)nullptr,
                                             (unsigned int*)nullptr, (int)npairs, 0, key_bits);
    return bytes;
}

hipError_t voxel_fill_grid(const double* d_v9, const Rec128* d_tris, int ntris, const unsigned long long* d_offsets, unsigned int npairs, unsigned int* d_pairs,
                           void* d_temp, size_t temp_bytes, unsigned int* d_first_last, const VoxelGridDev& grid, hipStream_t stream) {
    const int g = grid.n;
    const unsigned int cells = (unsigned)g * g * g;
    unsigned int* keys = d_pairs, *vals = d_pairs + (size_t)npairs, *keys2 = d_pairs + 2 * (size_t)npairs, *vals2 = d_pairs + 3 * (size_t)npairs;
    unsigned int* first = d_first_last, *last = d_first_last + cells;
    hipError_t e = hipMemsetAsync(d_first_last, 0, (size_t)cells * 2 * sizeof(unsigned int), stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(grid.mask, 0, voxel_mask_words(g) * sizeof(uint32_t), stream)) != hipSuccess) return e;     // the tail past N^3 stays 0
    if (npairs > 0) {
        const unsigned int blocks = (unsigned)std::min<long long>(((long long)ntris + 3) / 4, 1 << 16);
        hipLaunchKernelGGL(k_vox_emit, dim3(blocks), dim3(256), 0, stream, d_v9, ntris, g, d_offsets, keys, vals);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        // a radix sort is stable: pairs of one cell keep the order they were emitted in, ascending triangle index
        e = hipcub::DeviceRadixSort::SortPairs(d_temp, temp_bytes, (const unsigned int*)keys, keys2, (const unsigned int*)vals, vals2, (int)npairs, 0,
                                               voxel_key_bits(g), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_vox_bounds, dim3((npairs + 255u) / 256u), dim3(256), 0, stream, (const unsigned int*)keys2, npairs, cells, first, last);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_vox_reduce, dim3((cells + 255u) / 256u), dim3(256), 0, stream, d_tris, (const unsigned int*)vals2, (const unsigned int*)first,
                       (const unsigned int*)last, cells, grid.colors, grid.normals, grid.mask);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (g > kG) {
        const unsigned int bricks = (unsigned)grid.nb * grid.nb * grid.nb;
        if ((e = hipMemsetAsync(grid.coarse, 0, voxel_mask_words(grid.nb) * sizeof(uint32_t), stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_vox_bricks, dim3((bricks + 3u) / 4u), dim3(256), 0, stream, (const uint32_t*)grid.colors, g, grid.nb, grid.bricks, grid.coarse);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_voxel_frame(const VoxelLaunch& L) {
    const int n2 = L.fc.sub_pixel_res * L.fc.sub_pixel_res;
    const int g = L.grid.n;
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
        // the kernel follows from N: 64 = the compile-time grid, below = the same walk with N read from the grid, above = two levels
        if (g > kG) {
            if (L.flat_mask) { if (L.stats) go(k_voxel_walk<0, W_FLAT, true>); else go(k_voxel_walk<0, W_FLAT, false>); }
            else { if (L.stats) go(k_voxel_walk2<true>); else go(k_voxel_walk2<false>); }
        } else if (g == kG) {
            if (L.global_table) { if (L.stats) go(k_voxel_walk<kG, W_TABLE, true>); else go(k_voxel_walk<kG, W_TABLE, false>); }
            else { if (L.stats) go(k_voxel_walk<kG, W_LDS, true>); else go(k_voxel_walk<kG, W_LDS, false>); }
        } else {
            if (L.global_table) { if (L.stats) go(k_voxel_walk<0, W_TABLE, true>); else go(k_voxel_walk<0, W_TABLE, false>); }
            else { if (L.stats) go(k_voxel_walk<0, W_LDS, true>); else go(k_voxel_walk<0, W_LDS, false>); }
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (e1 && (e = hipEventRecord(e1, L.stream)) != hipSuccess) return e;
        if (n2 > 1 && (e = launch_resolve_rows(L.fc, L.row_map, row_begin, row_count, L.samples, L.pixels, L.stream)) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_voxel_trace(const TraceLaunch& L, const RootBox& box, const VoxelGridDev& grid, int max_blocks, bool flat_mask) {
    if (L.n <= 0) return hipSuccess;
    const unsigned int blocks = (unsigned)std::max<long long>(1, std::min<long long>((L.n + 255) / 256, (long long)max_blocks));
    const auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, L.stream, box, grid, (long long)L.n, L.starts, L.dirs, L.hit, L.ray_frac, L.pos, L.normal,
                           L.color, L.tri, L.counters);
    };
    if (grid.n > kG) { if (flat_mask) go(k_voxel_trace<0, W_FLAT>); else go(k_voxel_trace2); }
    else if (grid.n == kG) go(k_voxel_trace<kG, W_LDS>);
    else go(k_voxel_trace<0, W_LDS>);
    return hipGetLastError();
}

}  // namespace sr
