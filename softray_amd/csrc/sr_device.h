// sr_device.h -- interface between the C-ABI layer (sr_api.cpp) and the gfx950 kernels (sr_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "sr_types.h"

namespace sr {

// Device-resident scene (all pointers are HBM addresses on the scene's device).
struct DevScene {
    const Rec128*  tris;        // model triangles in TriangleIndex order
    int32_t        ntris;
    const Rec128*  extra;       // ExtraGeometryToRaytrace, insertion order
    int32_t        nextra;
    // reference tree
    const RefNode* rnodes;
    const LeafBox* rboxes;
    const int32_t* rleaf;
    int32_t        rdepth;      // TreeDepth (stack bound)
    // own BVH
    const BvhNode* bnodes;
    const Rec128*  btris;       // triangle records gathered in leaf order (aux = TriangleIndex)
    const TriSlab* bslab;       // fp32 shaft-prefilter records, same order as btris
    const CamCone* bcam;        // fp32 camera-cone records of the current frame's ray origin, same order (nullptr: none)
    const LightCone* blight;    // fp32 penumbra-plane records of the current frame's light ball, same order (nullptr: k_shaft_pkt4 filters with bslab)
    const double*  v9;          // model vertices [ntris][3][3], TriangleIndex order
    int32_t        bdepth;
    int32_t        bnode_bits;  // bits needed for a BVH node index (stack words pack node | bound)
    // the same tree with four children per node (packet walks), children sorted per frame: front to back for the camera rays'
    // origin / back to front for the point light (nullptr: not made -> the BVH2 packet walks run)
    const Bvh4Node* b4;         // build order (private walks: every lane orders the children for its own ray)
    const Bvh4Node* b4cam;
    const Bvh4Node* b4light;
    int32_t        b4depth;
    // axes (bit a) on which the ordered copy stores (near, far) instead of (lo, hi): the camera origin / the light lies outside the
    // root box's slab on that axis, so every ray of the frame has the same sign there (child_slabs<KNOWN>, sr_trace.h)
    int32_t        b4cam_known, b4light_known;
    RootBox        root;
    uint8_t*       shadow_cache; // static soft-shadow cache, 128^3 bytes, 0 = empty cell (SR_F_STATIC_SHADOWS frames)
    const uint8_t* binter;      // 1: the record's triangle lies inside the shrunk root box (k_interior_flags), same order as btris
};

constexpr int kShaftRounds = 2;
enum KernelId { K_RENDER = 0, K_TRACE = 1, K_PRIMARY = 2, K_SHADOW = 3, K_RESOLVE = 4, K_SHAFT = 5, K_FALLBACK = 6, K_SHAFT2 = 7, K_SHADOW2 = 8, K_POST = 9, K_ANTI_ALIAS = 10, K_BOUNCE = 11, K_PATHTRACE = 12, K_PT_COUNT = 13, K_PT_EXCHANGE = 14, K_VOXEL_WALK = 15, K_VOXELISE = 16, K_AO = 17, K_AO_PROBE = 18, K_LF_LOOKUP = 19, K_LF_FILL = 20, K_LF_APPLY = 21, K_LF_BAKE = 22, K_TRI_RECORDS = 23, K_TRI_BOUNDS = 24, K_REFIT_LEAVES = 25, K_REFIT_NODES = 26, K_PTS_INGEST = 27, K_PTS_SORT = 28, K_LFI_LOOKUP = 29, K_LFI_APPLY = 30, K_LFT_FILL = 31, K_LFT_HIT = 32, K_LFT_TRACE = 33, K_LFT_BAKE = 34, K_HITS = 35, K_DRAWS = 36, K_AOP_PROBE = 37, K_PP_TRACE = 38, K_SSP_CLAIM = 39, K_SSP_APPLY = 40, K_TIGHT_BOXES = 41, K_ORIGIN_RAYS = 42, K_ORIGIN_SORT = 43, K_OCCLUDED = 44, K_OCCL_SORT = 45, K_LFR_LOOKUP = 46, K_LFR_FINISH = 47, K_LFRI_LOOKUP = 48, K_LFRI_FINISH = 49, K_NEAREST = 50, K_NEAREST_SORT = 51, K_ALL_HITS = 52, K_ALL_HITS_SORT = 53, K_CLOSEST = 54, K_CLOSEST_SORT = 55, K_NEAR = 56, K_NEAR_SORT = 57, K_OVERLAP = 58, K_OVERLAP_SORT = 59, K_COUNT = 60 };
const char* kernel_name(int id);

struct RenderLaunch {
    DevScene    sc;
    FrameConst  fc;
    int32_t     mode;           // SR_MODE_*
    const double* offsets;      // device [shadow_samples][3]
    const int32_t* row_map;     // device [num_rows]: image row of each compact row
    uint32_t*   pixels;         // device output
    unsigned long long* stats;  // device [8] or nullptr: primary {rays, tri tests, nodes, leaves}, secondary {same}
    hipStream_t stream;
};

// The one-kernel renderer: ray generation, traversal, shading, inline shadow rays, sub-pixel resolve.
hipError_t launch_render(const RenderLaunch& L);

// sr_render_hits: the caller's device arrays, one entry per camera sample in scan order ([S][3] doubles, [S] scalars); any may be nullptr
struct HitsOut {
    double*   starts;
    double*   dirs;
    uint8_t*  hit;
    double*   ray_frac;
    double*   pos;
    double*   normal;
    uint32_t* color;
    int32_t*  tri;
};

// The default path: k_primary -> k_shadow -> k_resolve (sr_pipeline.hip).
struct PipelineLaunch {
    DevScene    sc;
    FrameConst  fc;
    int32_t     mode;
    const double*  offsets;     // device [shadow_samples][3]
    const int32_t* row_map;     // device [num_rows]
    uint32_t*   pixels;         // device output frame (full surface or compact strips)
    uint32_t*   samples;        // device [band_rows * width * n^2] sample colours (sub_pixel_res > 1 only)
    void*       hits;           // device hit queue, band_rows * width * n^2 records of pipeline_hit_record_bytes()
    unsigned int* counters;     // device uint[8]: hits, k_shadow head, items entering round 1.., fallback count, fallback head
    // shaft path (own BVH + point light), kShaftRounds rounds of (k_shaft, k_shadow_test); round 0 covers every hit
    unsigned int  round_items[kShaftRounds];      // capacity (hits) of the round's buffers (round 0: band samples)
    int           round_cap[kShaftRounds];        // candidate-list length (stride) of the round
    unsigned int* round_list[kShaftRounds];       // device hit indices entering the round (round 0: hits k_shaft left undecided)
    void*         round_state[kShaftRounds];      // device RoundState per item (round 0: nullptr)
    unsigned int* round_cand_count[kShaftRounds]; // device per-item candidate count | truncated flag
    int32_t*      round_cand[kShaftRounds];       // device [items][pipeline_round_cap(round)] (round_cand[0] == nullptr: no shaft path)
    void*         hits2;        // second ray queue of the mirror-bounce pipeline (same size as hits)
    unsigned int* ray_sort_buf; // mirror-bounce pipeline: 4 x band samples of scratch for the per-level ray order (nullptr: rays walk in queue order)
    void*         ray_sort_temp;
    size_t        ray_sort_temp_bytes;
    uint32_t*     bounce_levels; // device [band samples][max_bounces + 1]: colour of every level of a sample's mirror chain
    uint8_t*      bounce_nlev;  // device [band samples]: levels stored | 0x80 when the deepest level is a surface
    void*         bounce_prep;  // device [band samples] x 64 B: a level's rays after the FP64 clip, in walk order (k_bounce_prep)
    void*         bounce_res;   // device [band samples] x 16 B: nearest hit of every such ray (k_bounce_walk)
    int32_t*      bounce_stack; // device: the part of k_bounce_walk's per-lane stacks that does not live in LDS ([level][lane])
    size_t        bounce_stack_bytes;
    // path tracing (SR_F_PATH_TRACING; all nullptr / 0 otherwise).  The second rays are queued in hits2
    uint8_t*      pt_flags;     // device [band samples]: hit flag per scan position
    uint32_t*     pt_index;     // device [band samples]: hits before the position inside its chunk of pipeline_pt_chunk() positions
    uint32_t*     pt_totals;    // device [chunks + 1]: hits before each chunk, the band's hit count behind them
    uint32_t*     pt_carry;     // device [pt_blocks]: hits of every row block in the bands rendered so far (zeroed by launch_pipeline)
    const int32_t* pt_table;    // device: InternalSample() ints of Random(random_seed), 3 per sample of the largest row block
    int32_t       pt_block_height, pt_blocks;   // rows per row block and their number (Renderer.cs:1655-1666)
    // a part of a path-traced frame that a multi-device scene has split (0 / nullptr otherwise): the row blocks are those of the whole
    // row range [pt_range_first, pt_range_first + pt_range_rows), of which this launch renders the rows of row_map
    int32_t       pt_phase;     // 0: a whole frame.  1: primary pass + hit-index scan + the rows' hit counts -> pt_row_hits, no pixels.
                                // 2: pt_row_k0 from the merged pt_row_hits, then the second rays and the pixels
    bool          pt_reuse;     // the part's rows are one band: phase 2 starts from the queue, flags and scan phase 1 left (it repeats them otherwise)
    uint32_t*     pt_row_hits;  // device [pt_range_rows]: hits per image row of the range (phase 1 writes the part's rows, phase 2 reads all)
    uint32_t*     pt_row_k0;    // device [fc.num_rows]: hits of any part that precede the compact row inside its row block
    int32_t       pt_range_first, pt_range_rows;
    // ambient occlusion (SR_F_AMBIENT_OCCLUSION; all nullptr otherwise).  The stage runs on the band's hit queue after the shadow stage; it uses
    // pt_flags / pt_index / pt_totals / pt_carry and pt_block_height / pt_blocks for the generators' scan and hits2 for the generator list
    uint8_t*      ao_cache;     // device [128^3]: the scene's AO cache, 0 = empty cell (read and written in cached mode only)
    unsigned long long* ao_claim; // device [128^3]: smallest order key that asked for an empty cell (cached mode)
    uint32_t*     ao_escapes;   // device [band samples]: escaped probes per generator, then its byte
    // called once the number of generators is known (the stream has been waited for): the table of the seed's InternalSample() ints that
    // holds 300 draws for each of `generators` generators of one row block, or nullptr when the host refuses it
    const int32_t* (*ao_table)(void* user, unsigned long long generators);
    // colour light field (SR_F_LIGHT_FIELD; all nullptr / 0 otherwise): the frame runs k_lf_lookup / k_lf_fill / k_lf_apply per row band instead of
    // the primary walk; counters[0] is the length of the band's fill list
    uint32_t*     lf_cache;     // device [lf_entries]: the scene's light field, 0 = empty entry
    uint32_t*     lf_claim;     // device [(lf_entries + 31) / 32]: one bit per entry, set while a cell waits in a fill list; all zero between frames
    const double* lf_points;    // device [2 lf_res][lf_res][3]: the patch centres P(i, j) of the canonical rays, made on the host
    int32_t       lf_res;       // N
    uint32_t      lf_entries;   // 4 N^4
    uint32_t*     lf_cells;     // device [band samples]: cache index per sample, 0xFFFFFFFF = the sample's line misses the sphere
    uint32_t*     lf_list;      // device [band samples]: the cells the band fills
    // ... with dynamic shadows (sr_set_light_field_shadows + SR_F_SHADOWS): the canonical rays' hits go through the frame's shadow stage as a
    // compact queue in `hits` (sample = queue slot, pad[1] = the cell), their colours wait in lf_stage, k_lf_store writes the cells
    bool          lf_shadows;
    uint32_t*     lf_stage;     // device [band samples]: the staged colour of every queue slot (the shadow stage's "sample buffer")
    // sr_bake_light_field with shadows (lf_bake_count > 0: launch_pipeline renders no rows): the range, the cells per pass -- band samples,
    // what the queue, lf_stage and the shadow stage's lists hold -- and where the entries written are counted
    uint64_t      lf_bake_first, lf_bake_count, lf_bake_pass_cells;
    unsigned long long* lf_bake_filled;
    bool          lf_bake_packet;   // BakeLaunch::packet
    // quad-linear interpolation (sr_set_light_field_interpolation): k_lfi_lookup / k_lfi_apply take the places of k_lf_lookup / k_lf_apply, and
    // lf_list (with shadows also hits, lf_stage and the shadow stage's lists) has room for min(16 x band samples, lf_entries) cells
    bool          lf_interp;
    bool          lf_carry;         // the lookup hands base cell (lf_cells) and fractions (lf_fracs) to the apply kernel; false (hook 39): apply computes them again
    double*       lf_fracs;         // device [band samples][4] (lf_carry), else nullptr
    // triangle light field (sr_set_light_field_triangles): lf_cache / lf_claim are the TRIANGLE table's (0 empty, 1 nothing, t + 2 triangle t) and the
    // band runs k_lf_lookup, k_lft_fill, k_lft_hit (!lf_fused: and k_lft_trace); counters[0] = the fill list's length, counters[1] = the trace list's
    bool          lf_tris;
    const int32_t* lf_handle;       // device [ntris]: the reference tree's node index of every triangle's handle leaf (Triangle.HandleToLeafNode)
    uint32_t*     lf_trace_list;    // device [band samples]: the samples whose first two stages missed
    bool          lf_fused;         // k_lft_hit runs the full trace itself (production); false (hook 43): it lists the samples for k_lft_trace, same frame
    // sr_shadow_points (pts_n > 0: launch_pipeline renders no rows): n caller-given surface points in passes of pts_pass (band samples) go through
    // the frame's dynamic shadow stage as a compact queue in `hits`; pts_out is the stage's sample buffer (k_pts_ingest, sr_pipeline.hip)
    int64_t       pts_n, pts_pass;
    const double* pts_pos;      // device [n][3], model space
    const double* pts_nrm;      // device [n][3], as given
    const uint32_t* pts_color;  // device [n] or nullptr (every point 0xFFFFFFFF); may be pts_out
    uint32_t*     pts_out;      // device [n]
    bool          pts_sort;     // queue a pass in ray_sort's order (cell of the point, octant of the normal) instead of input order (point_order)
    bool          pts_per_lane; // the first shaft round with private per-lane walks (A/B hook)
    bool          pts_escape;   // a directional light whose samples all escape for a probe end inside [pts_escape_lo, pts_escape_hi]
    double        pts_escape_lo[3], pts_escape_hi[3];
    // sr_static_shadow_points (pts_static, with pts_n > 0): the points go through the scene's static shadow cache instead -- the first point of an
    // empty cell (input order: static_claim, reset once per call) generates its byte through the frame's stage with the static bit set, every point
    // reads its cell (k_ssp_claim / k_ssp_select / k_ssp_apply, sr_pipeline.hip).  pts_out and pts_amount are each optional
    bool          pts_static;
    uint8_t*      pts_amount;       // device [n] or nullptr: every point's cell byte
    unsigned long long* pts_generators; // device, or nullptr: the generators are added to it (the caller zeroes it)
    // sr_render_hits (hits_req: launch_pipeline runs k_hits per row band instead of the frame's kernels and writes no pixel)
    bool          hits_req;
    HitsOut       hits_out;
    // sr_trace_origin_rays (org_n > 0: launch_pipeline renders no rows): n caller-given directions from fc.start_world in passes of org_pass rays
    // through k_origin_rays on the frame's primary walk (primary_walk_kind), answers straight into hits_out (starts / dirs unused) at the
    // ray's input index.  A packet pass is ordered by dir_order (ray_sort_buf: 4 x the pass rounded up to 256 words, ray_sort_temp)
    int64_t       org_n, org_pass;
    const double* org_dirs;     // device [n][3], as given
    bool          org_coherent; // SR_RAYS_COHERENT: a pass keeps its input order (the irregular rays still go last)
    // sr_light_field_rays (lfr_n > 0: launch_pipeline renders no rows): n caller-given rays in passes of lfr_pass rays through k_lfr_lookup, the
    // frame's fill stage and k_lfr_finish (lf_interp: k_lfri_lookup / k_lfri_finish).  lf_list has room for a pass's cells (lf_interp: min(16 x
    // pass, lf_entries)); lf_cells is the pending list, 2 + 2 x pass words ([0]: its length); with shadows `hits`, lf_stage and the shadow stage's
    // lists hold one slot per listed cell
    int64_t       lfr_n, lfr_pass;
    const double* lfr_starts;   // device [n][3], model space
    const double* lfr_dirs;     // device [n][3], as given
    uint32_t*     lfr_out;      // device [n]
    uint8_t*      lfr_inside;   // device [n] or nullptr: 1 = the line pierces the sphere
    unsigned long long* lfr_filled; // device, or nullptr: the entries written are added to it (the caller zeroes it)
    void*         static_hits;  // device HitRec[min(band samples, 128^3)]: generators of a static-shadow frame
    unsigned long long* static_claim; // device [128^3]: smallest order key that asked for an empty cell
    int32_t       static_concurrency; // rayTraceConcurrency of the frame
    unsigned int* fallback;     // device [band samples]: hits that need the exact per-lane fallback
    void*         fallback_state; // device RoundState per fallback entry: which samples are still undecided
    unsigned int* fallback_rays;  // device [fallback_ray_cap]: (entry << 7 | sample) of every undecided sample
    unsigned int  fallback_ray_cap;
    unsigned int* fallback_overflow; // device [band samples]: entries the ray list had no room for
    int32_t     band_rows;      // rows per band (multiple of 16)
    int32_t     row_first, row_limit; // compact rows [row_first, row_limit) of the frame are this launch's share
    int32_t     persistent_blocks;
    bool        per_lane_shadows; // force k_shadow (one lane per hit) instead of k_shadow_packet (cross-check)
    int32_t     tile_queue_n2, tile_queue_rows; // (set by launch_pipeline) > 0: the hit queue of this band is tile-indexed
    int32_t     round2_node_budget; // later shaft rounds: a private walk gives up after this many nodes (0 = never)
    bool        per_lane_primary; // k_primary with private walks instead of the packet walk + camera-cone filter (cross-check)
    bool        bvh2_packets;     // the packet walks on the two-wide tree with a per-step vote (round 2's kernels; cross-check)
    bool        primary_stats_only;   // `stats` counts the primary rays only (SR_F_PRIMARY_STATS_ONLY): the shadow / bounce stages run their uncounted instantiations
    int32_t     shaft_wgs_per_cu; // resident workgroups per CU of the persistent shaft walk (0 = 6)
    bool        shadows_on_bvh;   // mode != BVH: the shadow rays of a dynamic frame are traced on the own BVH (shaft path) all the same
    int32_t     per_lane_shaft;   // bit 0: k_shaft (private walks) for the first round instead of k_shaft_pkt, bit 1: for the later rounds instead of k_shaft_coop (cross-checks)
    bool        exact_shadow_tests; // k_shadow_test (every pair in FP64) instead of k_shadow_cls (fp32 classification first)
    unsigned long long* stats;  // device [8] or nullptr
    // longest-first order of the persistent shaft kernel's tiles: k_shaft_pkt4 leaves every 8x8 tile's walk length in tile_cost, k_tile_order
    // turns them into per-XCD lists (longest walks first) for the NEXT frame with the same tile grid; `tile_order_tag` is host state of the
    // scratch set: the grid the lists in tile_order were made for (0: none).  All three nullptr: natural order
    unsigned int* tile_cost;
    unsigned int* tile_order;
    unsigned long long* tile_order_tag;
    // umbra hints of the same walk (sr_umbra_hint.h): one word per 8x8 tile, indexed like tile_cost, in two arrays -- a launch reads the one the
    // previous launch wrote and writes the other, so what it does is a function of the previous launch and not of which wave ran first.
    // `tile_hint_cur` is host state of the scratch set: the array the next launch writes (it flips it).  Both 0xFFFFFFFF-filled by the owner
    // whenever they are (re)allocated or the scene's records change.  nullptr: no hints
    unsigned int* tile_hint[2];
    int* tile_hint_cur;
    uint32_t* shaft_launches;   // host [2] or nullptr: += persistent launches of the shaft walk, += those that walked tile_order (sr_debug_counters [6], [7])
    hipStream_t stream;
    void (*get_events)(void* user, int kernel_id, hipEvent_t* start, hipEvent_t* stop);   // optional per-launch timing
    // optional: called when every kernel of a row band has been enqueued on `stream` -- compact rows [row_begin, row_begin + row_count)
    // of the frame are final once what is on the stream now has run (sr_render copies a band to the host while the next ones render)
    void (*band_done)(void* user, int band_index, int row_begin, int row_count, hipStream_t stream);
    void*       user;
};
hipError_t launch_pipeline(const PipelineLaunch& L);

// sr_bake_light_field: the dense fill of entries [first, first + count) of the light field (k_lf_bake, sr_pipeline.hip)
struct BakeLaunch {
    DevScene    sc;
    FrameConst  fc;
    int32_t     mode;
    const double* points;       // device [2 res][res][3]: the patch centres
    int32_t     res;            // N
    uint32_t*   cache;          // device [4 N^4]: the scene's light field
    uint64_t    first, count;   // the range, inside the table
    uint64_t    launch_cells;   // cells per launch (rounded down to whole origin patches, at least one)
    bool        tris;           // `cache` is the triangle table: k_lft_bake stores triangle index + 2 / 1 (model alone, no shading)
    bool        packet;         // SR_MODE_BVH with one packet walk per wave instead of private per-lane walks (cross-check, A/B measurement)
    bool        walk_stats;     // count what the walks do in stats[5..7] too
    unsigned long long* stats;  // device [8] or nullptr: [4] += canonical rays traced, [5..7] += the walks' counters
    unsigned long long* filled; // device: += entries written
    hipStream_t stream;
    void (*get_events)(void* user, int kernel_id, hipEvent_t* start, hipEvent_t* stop);   // optional per-launch timing
    void*       user;
};
hipError_t launch_lf_bake(const BakeLaunch& L);
// sr_light_field_coords: RayToFloat4D of n rays at resolution `res` (k_lf_coords, sr_pipeline.hip: the device function of the interpolating frame kernels)
hipError_t launch_lf_coords(long long n, const double* starts, const double* dirs, int res, double* coords, uint8_t* inside, hipStream_t stream);
// sr_ao_points (sr_pipeline.hip k_aop_ingest): n caller-given surface points through AmbientOcclusionMethod's step in passes of `pass` points
constexpr int64_t kAopMaxPass = 1ll << 17;     // 2^17 generators: a 150 MiB draw table
struct NetWindow { int32_t s[109]; };           // the first 109 InternalSample() values of a Random (sr_host.h net_random_window)
struct AoPointsLaunch {
    DevScene    sc;
    int32_t     mode;
    int64_t     n, pass;
    const double* pos;          // device [n][3], model space
    const double* nrm;          // device [n][3], as given
    const uint32_t* color;      // device [n] or nullptr (every point 0xFFFFFFFF); may be `out`
    uint32_t*   out;            // device [n] or nullptr
    uint8_t*    amount;         // device [n] or nullptr
    uint64_t    first_generator;
    uint8_t*    cache;          // device [128^3]: the scene's AO cache; nullptr: uncached, every point generates
    unsigned long long* claim;  // device [128^3] (cached)
    void*       recs;           // device HitRec[pass]: the pass's points
    void*       gen;            // device HitRec[pass]: its generators
    uint8_t*    flags;          // device [pass]
    uint32_t*   index;          // device [pass]
    uint32_t*   totals;         // device [pass / pipeline_pt_chunk() + 2]
    uint32_t*   escapes;        // device [pass]
    int32_t*    table;          // device, ao_points_table_bytes(pass): the pass's draws, 300 per generator
    NetWindow   window;         // ... of Random(random_seed) (unused with host_table)
    const uint32_t* stride_rows; // device [2][55][55]: the jump coefficients of one chunk and of 64 chunks (sr_api.cpp)
    int32_t*    base_window;    // device [55]
    unsigned long long* running; // device: generators of the call's earlier passes
    unsigned long long* generators_out; // device or nullptr: receives the call's generator count
    bool        nearest_walks;  // SR_MODE_BVH with nearest-hit walks instead of any-hit walks (hook 34)
    // not nullptr: the host makes every pass's table -- `count` generators from draw 300 * base on -- and the call waits once per pass
    hipError_t (*host_table)(void* user, uint64_t base, uint32_t count, int32_t* d_table, hipStream_t stream);
    unsigned long long* stats;  // device [8] or nullptr: [4] += probes, [5..7] += what their walks count
    int32_t     persistent_blocks;
    hipStream_t stream;
    void (*get_events)(void* user, int kernel_id, hipEvent_t* start, hipEvent_t* stop);
    void*       user;
};
hipError_t launch_ao_points(const AoPointsLaunch& L);
size_t ao_points_table_bytes(int64_t pass);
// sr_path_points (sr_pipeline.hip k_pp_ingest): n caller-given surface points through PathTracingMethod's step in passes of `pass` points
constexpr int64_t kPpMaxPass = 1ll << 22;      // 2^22 points: a 48 MiB draw table, 256 MiB of ray records
struct NetState { int32_t s[55]; };             // 55 consecutive InternalSample() values of a Random: all a jump-ahead needs to go on from
struct PathPointsLaunch {
    DevScene    sc;
    FrameConst  fc;             // shading of the second hit (SR_F_SHADING: transform and lights)
    int32_t     mode;
    int64_t     n, pass;
    const double* pos;          // device [n][3], model space
    const double* nrm;          // device [n][3], as given
    const uint32_t* color;      // device [n] or nullptr (every point 0xFFFFFFFF); may be `out`
    uint32_t*   out;            // device [n] or nullptr
    uint32_t*   incoming;       // device [n] or nullptr
    double*     dirs;           // device [n][3] or nullptr
    uint64_t    first_sample;
    void*       rays;           // device HitRec[pass]: the pass's second rays (unused when only `dirs` is asked for)
    int32_t*    table;          // device, path_points_table_bytes(pass): the pass's draws, 3 per point
    const NetState* windows;    // HOST, one per pass: the draws 3 (first_sample + pass start) .. + 54 (nullptr with host_table)
    const uint32_t* stride_rows; // device [2][55][55]: the jump coefficients of one chunk and of 64 chunks (as AoPointsLaunch)
    int32_t*    base_window;    // device [55]
    uint32_t*   pass_units;     // device: the 300-draw units of the pass's table (what k_aop_states / k_draws call generators)
    // not nullptr: the host makes every pass's table -- 3 `count` draws from draw 3 `first_point` on -- and the call waits once per pass
    hipError_t (*host_table)(void* user, uint64_t first_point, uint32_t count, int32_t* d_table, hipStream_t stream);
    // SR_MODE_BVH: the incoherent-ray route of a path-traced frame (PipelineLaunch's fields of the same names)
    unsigned int* counters;     // device [4]: [0] the pass's rays, [2] the walk's work head
    unsigned int* ray_sort_buf; // device [4 x pass]
    void*       ray_sort_temp;
    size_t      ray_sort_temp_bytes;
    void*       bounce_prep;    // device [pass] x 64 B
    void*       bounce_res;     // device [pass] x 16 B
    int32_t*    bounce_stack;
    size_t      bounce_stack_bytes;
    bool        bvh2_packets;   // SR_DBG_BVH2_PACKETS: the walk on the two-wide tree, as a frame's
    unsigned long long* stats;  // device [SR_STATS_COUNT] or nullptr: [4..7] (SR_MODE_BVH: [20..23] too) += what the second rays count
    int32_t     persistent_blocks;
    hipStream_t stream;
    void (*get_events)(void* user, int kernel_id, hipEvent_t* start, hipEvent_t* stop);
    void*       user;
};
hipError_t launch_path_points(const PathPointsLaunch& L);
size_t path_points_table_bytes(int64_t pass);
// per-frame pre-pass: a copy of the four-wide nodes with every node's children sorted by the distance of their box centres from
// `point` (model space), nearest first (camera origin) or farthest first (light: nearest to the surface points first)
// swap_mask (bit a): exchange lo and hi on axis a in the copy (the rays of the frame travel towards smaller coordinates there)
// live_runs (nullable): int2 per (node, slot) from launch_facing_partition -- the (offset, count) of a leaf's records that rays of this
// copy can hit
hipError_t launch_order_nodes(const Bvh4Node* in, Bvh4Node* out, int num_nodes, const RootBox& root, const double point[3], bool far_first, int swap_mask,
                              const void* live_runs, hipStream_t stream);
// per (camera origin, light) pre-pass, before launch_order_nodes (sr_lbvh.hip, sr_tight_boxes.h): d_out = the base tree's nodes with the live
// runs applied and the boxes fitted to the live records below them; launch_order_nodes then runs with in == out == d_out and no live runs.
// level_first: collapse_bvh4_device's level ranges; cut: only the lowest `cut` levels are fitted (< 0: all)
hipError_t tight_boxes_device(const Bvh4Node* d_base, Bvh4Node* d_out, int num_wide, const std::vector<int>& level_first, const void* d_live_runs,
                              const Rec128* d_btris, const double* d_v9, int ntris, const RootBox& root, int cut, hipStream_t stream);
// per (camera origin, light) pre-pass: re-orders the records of every leaf in place so that the records a camera ray / a shadow sample ray
// can hit (the triangle faces the origin / the light) are contiguous, and writes their (offset, count) per (node, slot) (int2 each)
hipError_t launch_facing_partition(const Bvh4Node* base, int num_nodes, Rec128* btris, TriSlab* bslab, const double origin[3], bool use_cam,
                                   const double light[3], double light_radius, bool use_light, void* cam_rng, void* light_rng, hipStream_t stream);
// per-frame pre-pass: camera-cone records of every BVH triangle for the ray origin `origin` (model space)
hipError_t launch_cam_cones(const DevScene& sc, int ntris, const double origin[3], CamCone* out, hipStream_t stream);
// k_light_cones: the LightCone record of every BVH triangle record for the light ball (light, light_radius); re-run when the light, the
// tree or the records' order changed
hipError_t launch_light_cones(const DevScene& sc, int ntris, const double light[3], double light_radius, LightCone* out, hipStream_t stream);
// per-tree pre-pass (re-made when the records move): the interior byte of every BVH triangle record, DevScene::binter
hipError_t launch_interior_flags(const DevScene& sc, int ntris, uint8_t* out, hipStream_t stream);
size_t pipeline_hit_record_bytes();
size_t pipeline_static_cells();
int pipeline_round_cap(int round);
int pipeline_round_cap_max(int round);
int pipeline_bounce_lds_levels();      // stack levels per lane k_bounce_walk keeps in LDS (deeper ones live in PipelineLaunch::bounce_stack)
int pipeline_pt_chunk();               // scan positions per workgroup of the path tracer's hit-index scan
size_t pipeline_round_state_bytes();
size_t pipeline_counter_bytes();
size_t pipeline_tile_items(int width, int rows, int n2);

// Own BVH built on the device (sr_lbvh.hip).  Inputs in TriangleIndex order, outputs caller-allocated (n entries each).
hipError_t gather_records_device(int n, const unsigned int* d_order, const Rec128* d_tris, Rec128* d_btris, const TriSlab* d_slab_in,
                                 TriSlab* d_bslab, hipStream_t stream);
hipError_t build_bvh_device(const double* d_v9, int n, const RootBox& root, const Rec128* d_tris, const TriSlab* d_slab_in,
                            BvhNode* d_nodes, Rec128* d_btris, TriSlab* d_bslab, int* num_nodes, int* depth, hipStream_t stream, int leaf_max = 0);

// order of a bounce level's ray queue by (origin cell, direction octant) (sr_raysort.hip): order_out = permutation of [0, cap)
size_t ray_sort_temp_bytes(unsigned int cap);
hipError_t ray_sort(const void* queue, const unsigned int* d_count, unsigned int cap, const RootBox& root, unsigned int* keys, unsigned int* keys2,
                    unsigned int* idx, unsigned int* order_out, void* temp, size_t temp_bytes, hipStream_t stream);

// sr_shadow_points: the order of a pass's queue.  recs: n records where their points lie (sample word 0xffffffff = not queued); order_out:
// the queued points first -- sorted: by ray_sort's key of (position, normal), ties in input order; !sorted: in input order.  A stable
// sort, so the queue does not depend on which wave ran first
// (keys2 returns the sorted keys: point_order_skip_mask(sorted) is their bit that marks a point that is not queued)
size_t point_order_temp_bytes(unsigned int cap);
unsigned int point_order_skip_mask(bool sorted);
hipError_t point_order(const void* recs, unsigned int n, bool sorted, const RootBox& root, unsigned int* keys, unsigned int* keys2, unsigned int* idx,
                       unsigned int* order_out, void* temp, size_t temp_bytes, hipStream_t stream);

// sr_trace_origin_rays: the order of a pass of n rays with a common origin (dirs: [n][3]).  order_out: the regular rays first -- sorted: by the
// cell of the unit direction in an octahedral map of 2^12 x 2^12 cells, Morton-interleaved (24 bits), ties in input order; !sorted: in input
// order -- then the irregular ones (a component not finite, or max |d_k| outside [2^-40, 2^40]) in input order.  A stable sort; keys2
// returns the sorted keys: point_order_skip_mask(sorted) is their bit that marks an irregular ray.  Scratch as point_order's
hipError_t dir_order(const double* dirs, unsigned int n, bool sorted, unsigned int* keys, unsigned int* keys2, unsigned int* idx, unsigned int* order_out,
                     void* temp, size_t temp_bytes, hipStream_t stream);

// sr_occluded_rays: the order of a pass of n arbitrary rays (starts, dirs: [n][3]; limits: [n] or nullptr = 1.0; endpoints: the direction is
// dirs - starts).  A ray is REGULAR when its start is finite (max |s_k| <= 2^100), its limit is neither NaN nor -inf and its direction is
// regular by dir_order's definition.  order_out: the regular rays first -- sorted: by ray_sort's key of (start, direction), ties in input
// order; !sorted: in input order -- then the others in input order.  A stable sort; keys2 returns the sorted keys:
// point_order_skip_mask(sorted) is their bit that marks an irregular ray.  Scratch as point_order's
hipError_t occl_order(const double* starts, const double* dirs, const double* limits, unsigned int n, bool endpoints, bool sorted, const RootBox& root,
                      unsigned int* keys, unsigned int* keys2, unsigned int* idx, unsigned int* order_out, void* temp, size_t temp_bytes, hipStream_t stream);

// What the launches of the six batch calls below share (sr_batch.h holds the pass driver that reads it).  A call runs its n items in passes
// of `pass`; on the own BVH a pass is ordered first, the regular items in front and the irregular tail last
constexpr int64_t kBatchMaxPass = 1ll << 22;
struct BatchLaunch {
    int64_t     n, pass;
    const double* limits;       // device [n] or nullptr (what that means is the call's own)
    bool        input_order;    // SR_RAYS_COHERENT / SR_POINTS_COHERENT / the call's hook: a pass keeps its input order (the irregular items still go last)
    unsigned int* sort_buf;     // device: 4 x the pass rounded up to 256 words, and one more for a persistent walk's work head (ordered passes)
    void*       sort_temp;
    size_t      sort_temp_bytes; // point_order_temp_bytes
    unsigned long long* stats;  // device [SR_STATS_COUNT] or nullptr: [0] += items, [1..3] += what their walks count
    hipStream_t stream;
    void (*get_events)(void* user, int kernel_id, hipEvent_t* start, hipEvent_t* stop);
    void*       user;
};

// sr_occluded_rays (sr_occluded.hip): occluded[i] = sr_trace_rays' hit && ray_frac <= limit for n caller-given rays (no limits: every ray 1.0)
struct OccludedLaunch : BatchLaunch {
    DevScene    sc;
    int32_t     mode;           // SR_MODE_*
    bool        with_extra;     // root geometry of the chain (extra + model)
    const double* starts;       // device [n][3]
    const double* dirs;         // device [n][3]: directions, or end points (endpoints)
    uint8_t*    occluded;       // device [n]
    bool        endpoints;      // SR_RAYS_ENDPOINTS
    bool        nearest_walks;  // SR_MODE_BVH with nearest-hit walks plus the comparison for every ray (hook 47)
    int         refill_at;      // >= 0 (hook 100 + T): the any-hit launch with persistent lanes that fetch new rays at T busy lanes; < 0: one lane per ray
    int32_t     persistent_blocks;
};
hipError_t launch_occluded(const OccludedLaunch& L);

// sr_nearest_rays (sr_nearest.hip): sr_trace_rays' answer where it is a hit with ray_frac <= limit (no limits: no comparison), its miss
// otherwise, for n caller-given rays.  SR_MODE_BVH: occl_order's order, then k_nr_prep / k_nr_walk / k_nr_finish for the regular rays
constexpr int kNearestRefillAt = 24;    // k_nr_walk fetches new rays when at most this many lanes of a wave are still walking (k_bounce_walk's)
struct NearestLaunch : BatchLaunch {
    DevScene    sc;
    int32_t     mode;           // SR_MODE_*
    bool        with_extra;     // root geometry of the chain (extra + model)
    const double* starts;       // device [n][3]
    const double* dirs;         // device [n][3]: directions, or end points (endpoints)
    uint8_t* hit; double* ray_frac; double* pos; double* normal; uint32_t* color; int32_t* tri;    // device [n] each, or nullptr
    bool        endpoints;      // SR_RAYS_ENDPOINTS
    bool        lane_walks;     // SR_MODE_BVH with one private walk per lane for every ray, in input order (hook 49)
    bool        bvh2;           // SR_DBG_BVH2_PACKETS: the walk on the two-wide tree
    int         refill_at;      // k_nr_walk's refill threshold (hook 100 + T)
    int         lds_levels;     // stack levels per lane k_nr_walk keeps in LDS (hook 200 + K)
    int32_t     persistent_blocks;
    void*       prep;           // device [pass] x 64 B
    void*       res;            // device [pass] x 16 B
    int32_t*    deep;           // device: the stack levels beyond lds_levels, [level][lane of the grid]
    size_t      deep_bytes;
};
hipError_t launch_nearest(const NearestLaunch& L);

// sr_all_hits_rays (sr_allhits.hip): every qualifying hit of n caller-given rays (no limits: no comparison) -- count, and the first max_hits
// of them by (ray_frac, extra elements before triangles, element / TriangleIndex).  SR_MODE_BVH: occl_order's order, k_ah_walk for the
// regular rays, k_ah_loop (the per-record loop) for the others; SR_MODE_BRUTE: k_ah_loop in input order
constexpr int kAllHitsMax = 64;         // SR_HITS_MAX
struct AllHitsLaunch : BatchLaunch {
    DevScene    sc;
    int32_t     mode;           // SR_MODE_BVH or SR_MODE_BRUTE
    bool        with_extra;     // root geometry of the chain (extra + model)
    const double* starts;       // device [n][3]
    const double* dirs;         // device [n][3]: directions, or end points (endpoints)
    int32_t     max_hits;       // K, 0 .. kAllHitsMax
    uint32_t*   count;          // device [n] or nullptr (nullptr and K > 0: the walk culls at the K-th kept hit)
    int32_t*    index;          // device [n][K] or nullptr
    double*     ray_frac;       // device [n][K] or nullptr
    int32_t*    scratch_index;  // device [pass][K]: a lane's row where index is nullptr (K > 0)
    double*     scratch_frac;   // device [pass][K]: ... where ray_frac is nullptr
    bool        endpoints;      // SR_RAYS_ENDPOINTS
    bool        loop_all;       // SR_MODE_BVH with the per-record loop for every ray (hook 51)
};
hipError_t launch_all_hits(const AllHitsLaunch& L);

// sr_closest_points (sr_closest.hip): for n caller-given points the triangle that minimises (squared distance, TriangleIndex), its distance,
// the closest point and its weights, where the distance is within the limit (no limits: no comparison).  SR_MODE_BVH: k_cp_keys + the
// radix sort, k_cp_walk for the regular points (closest_regular, sr_closest.h), k_cp_loop (the per-record loop) for the others;
// SR_MODE_BRUTE: k_cp_loop in input order
struct ClosestLaunch : BatchLaunch {
    DevScene    sc;
    int32_t     mode;           // SR_MODE_BVH or SR_MODE_BRUTE
    const double* points;       // device [n][3]
    int32_t* tri; double* dist; double* pos; double* uv;      // device [n], [n], [n][3], [n][2]; each may be nullptr
    bool        loop_all;       // SR_MODE_BVH with the per-record loop for every point (hook 53)
};
hipError_t launch_closest(const ClosestLaunch& L);

// sr_near_triangles (sr_near.hip): for n caller-given points every triangle whose distance is a number within the limit (no limits: no
// comparison) -- count, and the first max_hits of them by (squared distance, TriangleIndex) with their distances, closest points and
// weights.  SR_MODE_BVH: sr_closest_points' order of a pass, k_nt_walk for the regular points, k_nt_loop (the per-record loop) for the
// others; SR_MODE_BRUTE: k_nt_loop in input order
struct NearLaunch : BatchLaunch {
    DevScene    sc;
    int32_t     mode;           // SR_MODE_BVH or SR_MODE_BRUTE
    const double* points;       // device [n][3]
    int32_t     max_hits;       // K, 0 .. kAllHitsMax
    uint32_t*   count;          // device [n] or nullptr (nullptr and K > 0: the walk also culls at the K-th kept entry)
    int32_t*    index;          // device [n][K] or nullptr
    double*     dist;           // device [n][K] or nullptr
    double*     pos;            // device [n][K][3] or nullptr
    double*     uv;             // device [n][K][2] or nullptr
    int32_t*    scratch_index;  // device [pass][K]: a lane's row where index is nullptr (K > 0)
    double*     scratch_dist;   // device [pass][K]: ... where dist is nullptr
    bool        loop_all;       // SR_MODE_BVH with the per-record loop for every point (hook 55)
};
hipError_t launch_near(const NearLaunch& L);

// sr_overlap_triangles (sr_overlap.hip): for n caller-given triangles every triangle of the model that the pair predicate of
// sr_tri_overlap.h reports -- count, and the first max_hits of them by TriangleIndex with the masks of their pairs.  SR_MODE_BVH: a pass
// ordered by the Morton cell of the centre of the query's box (k_ot_keys), k_ot_walk for the regular queries, k_ot_loop (the per-record
// loop) for the others; SR_MODE_BRUTE: k_ot_loop in input order
struct OverlapLaunch : BatchLaunch {
    DevScene    sc;
    int32_t     mode;           // SR_MODE_BVH or SR_MODE_BRUTE
    const double* tris;         // device [n][3][3]
    int32_t     max_hits;       // K, 0 .. kAllHitsMax
    bool        any;            // SR_OVERLAP_ANY: count is 0 or 1 and a query stops at its first reported triangle (max_hits == 0)
    uint32_t*   count;          // device [n] or nullptr
    int32_t*    index;          // device [n][K] or nullptr
    uint8_t*    mask;           // device [n][K] or nullptr
    int32_t*    scratch_index;  // device [pass][K]: a lane's row where index is nullptr and mask is not (K > 0)
    bool        loop_all;       // SR_MODE_BVH with the per-record loop for every query (hook 57)
};
hipError_t launch_overlap(const OverlapLaunch& L);

// the four-wide tree collapsed from a device-resident binary tree (same rule as the host's collapse_bvh4); d_wide: >= num_nodes entries
// level_first (nullable): the wide nodes are numbered level by level -- level L is [level_first[L], level_first[L + 1]), the last entry
// is *num_wide (what the refit's per-level launches need)
hipError_t collapse_bvh4_device(const BvhNode* d_nodes, int num_nodes, Bvh4Node* d_wide, int* num_wide, int* depth, hipStream_t stream,
                                std::vector<int>* level_first = nullptr);

// fp32 TriSlab records of n triangles (TriangleIndex order) computed on the device from the FP64 vertices (sr_lbvh.hip)
hipError_t make_slabs_device(const double* d_v9, int n, const RootBox& root, TriSlab* d_out, hipStream_t stream);

// sr_set_triangles_device (sr_lbvh.hip): the scene's vertex and record arrays (TriangleIndex order, n entries each) from the caller's
// device arrays -- d_src_argb == nullptr keeps the colour of the record that is in d_tris -- and the bounds of the vertices folded
// with the caller's box: six doubles {vmin, vmax} at the start of d_scratch (tri_bounds_scratch_bytes() bytes)
hipError_t tri_records_device(const double* d_src_v9, const uint32_t* d_src_argb, int n, double* d_v9, Rec128* d_tris, hipStream_t stream);
size_t tri_bounds_scratch_bytes();
hipError_t tri_bounds_device(const double* d_v9, int n, const double box_min[3], const double box_max[3], double* d_scratch, hipStream_t stream);

// sr_refit_triangles_device (sr_lbvh.hip): a device-built own BVH keeps its topology, leaf order and node numbering, and everything in it
// that describes geometry is re-made from d_v9 / d_tris (TriangleIndex order, already rewritten) and the new root: the leaf-order records
// and TriSlabs (position -> triangle = the record's aux), then the fp32 boxes bottom-up, one launch per level, deepest first -- of the
// binary nodes (d_depth: a byte per node, made on the tree's first call: *depths_made; tree_depth: the build's) and of the four-wide
// nodes (level_first).  d_tbox: n x refit_box_bytes() of scratch.  phase of get_events: 0 = k_refit_leaves, 1 = the node kernels.
size_t refit_box_bytes();
hipError_t refit_bvh_device(const double* d_v9, const Rec128* d_tris, int n, const RootBox& root, Rec128* d_btris, TriSlab* d_bslab, BvhNode* d_nodes,
                            int num_nodes, int tree_depth, Bvh4Node* d_wide, int num_wide, const std::vector<int>& level_first, void* d_tbox,
                            uint8_t* d_depth, bool* depths_made, hipStream_t stream,
                            void (*get_events)(void* user, int phase, hipEvent_t* start, hipEvent_t* stop), void* user);

// Surface passes (sr_post.hip): PostProcessImage colour functions and AntiAliasImage, Renderer.cs:819-978.
hipError_t launch_post_process(uint32_t* d_pixels, long long count, int style, uint32_t background, int num_cus, hipStream_t stream);
hipError_t launch_anti_alias(const uint32_t* d_src, uint32_t* d_dst, int dst_w, int dst_h, int res, hipStream_t stream);

struct TraceLaunch {
    DevScene sc;
    int32_t  mode;              // SR_MODE_*
    bool     with_extra;        // root geometry of the chain (extra + model)
    int64_t  n;
    const double* starts; const double* dirs;      // device [n][3]
    uint8_t* hit; double* ray_frac; double* pos; double* normal; uint32_t* color; int32_t* tri; int32_t* counters;
    hipStream_t stream;
};
hipError_t launch_trace(const TraceLaunch& L);
// k_resolve for the compact rows [row_begin, row_begin + row_count) of a band-local sample buffer (sr_pipeline.hip)
hipError_t launch_resolve_rows(const FrameConst& fc, const int32_t* row_map, int row_begin, int row_count, const uint32_t* samples, uint32_t* pixels, hipStream_t stream);

// ---- rayTraceVoxels (SR_F_VOXELS; sr_voxels.hip): the model as an N^3 grid of coloured cells, [x][y][z] order, N = sr_set_voxel_res ----
constexpr int kVoxelGrid = 64;                    // the default N, Renderer.cs:1570
constexpr int kVoxelGridMax = 256;                // three 8-bit coordinates: a 24-bit sort key
struct VoxelGridDev {
    uint32_t* colors;       // device [N^3]: 0 = empty cell
    double*   normals;      // device [N^3][3]
    uint32_t* mask;         // device [voxel_mask_words(N)]: bit (cell & 31) of word (cell >> 5) = the cell's colour is not 0; the tail is 0
    // N > 64 only (nullptr otherwise): bricks of 4x4x4 cells, brick index ((x>>2) * nb + (y>>2)) * nb + (z>>2), nb = (N + 3) / 4
    unsigned long long* bricks;   // device [nb^3]: bit (x&3)*16 + (y&3)*4 + (z&3) = the cell is filled; cells beyond N are 0
    uint32_t* coarse;       // device [voxel_mask_words(nb)]: bit (brick & 31) of word (brick >> 5) = the brick's word is not 0
    int32_t   n;            // N
    int32_t   nb;           // bricks per axis
};
// words of a bit mask over g^3 items: whole waves' ballots (64 bits) and whole uint4 for the staging loop
constexpr size_t voxel_mask_words(int g) { return (((size_t)g * g * g + 127) / 128) * 4; }
// The voxeliser in three steps, because the number of (cell, triangle) pairs decides what the second one needs:
// (1) cells per triangle and their exclusive scan (d_temp == nullptr: only the scan's scratch size -> *temp_bytes);
// (2) the caller reads offsets[n - 1] + counts[n - 1] back and provides d_pairs (4 x npairs words) and the sort's scratch;
// (3) pairs -> stable sort by cell -> per-cell sums in ascending triangle order -> colours, normals, occupancy bits.
// d_first_last: 2 x N^3 words of scratch.  The sort key has voxel_key_bits(N) = ceil(log2(N^3)) bits (18 at N = 64).
int voxel_key_bits(int n);
hipError_t voxel_count_cells(const double* d_v9, int ntris, int n, unsigned long long* d_counts, unsigned long long* d_offsets, void* d_temp, size_t* temp_bytes, hipStream_t stream);
size_t voxel_sort_temp_bytes(unsigned int npairs, int key_bits);
hipError_t voxel_fill_grid(const double* d_v9, const Rec128* d_tris, int ntris, const unsigned long long* d_offsets, unsigned int npairs, unsigned int* d_pairs,
                           void* d_temp, size_t temp_bytes, unsigned int* d_first_last, const VoxelGridDev& grid, hipStream_t stream);
struct VoxelLaunch {
    FrameConst  fc;
    RootBox     box;            // AxisAlignedBox((-1,-1,-1), (1,1,1)), VoxelGrid.cs:38
    VoxelGridDev grid;
    const int32_t* row_map;     // device [fc.num_rows]
    uint32_t*   pixels;         // device output frame (full surface or compact strips)
    uint32_t*   samples;        // device [band_rows * width * n^2] (sub_pixel_res > 1 only)
    int32_t     band_rows;
    int32_t     persistent_blocks;
    bool        global_table;   // a step reads the colour table instead of the occupancy bits in LDS (A/B measurement, same pixels)
    bool        flat_mask;      // N > 64: a step reads the row-major occupancy bits in global memory instead of the two-level walk (A/B, same pixels)
    unsigned long long* stats;  // device [4..] or nullptr
    hipStream_t stream;
    void (*get_events)(void* user, int kernel_id, hipEvent_t* start, hipEvent_t* stop);
    void*       user;
};
hipError_t launch_voxel_frame(const VoxelLaunch& L);
hipError_t launch_voxel_trace(const TraceLaunch& L, const RootBox& box, const VoxelGridDev& grid, int max_blocks, bool flat_mask);
hipError_t launch_shade_points(const FrameConst& fc, long long n, const double* pos, const double* nrm, const uint32_t* color, uint32_t* out, hipStream_t stream);

// `enqueue()` between the two timing events of kernel_id, where the caller wants them: for every launch struct above (get_events, user,
// stream).  The stop event is recorded on every exit from the body -- a pair that was opened stays a pair -- and the body's error wins
template <class Launch, class Enqueue>
hipError_t timed(const Launch& L, int kernel_id, Enqueue enqueue) {
    hipError_t e;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (L.get_events) L.get_events(L.user, kernel_id, &e0, &e1);
    if (e0 && (e = hipEventRecord(e0, L.stream)) != hipSuccess) return e;
    e = enqueue();
    const hipError_t stop = e1 ? hipEventRecord(e1, L.stream) : hipSuccess;
    return e != hipSuccess ? e : stop;
}

// --------------------------------------------------------------------------------------------------
// Wave votes of the packet walks.  THE RULE: a vote is a test of an INTEGER, and __ballot only ever sees ONE comparison.
// A lane predicate that is only voted on or used to gate per-lane work lives as a 64-bit mask in a scalar register pair:
//   vote(a < b)                one v_cmp that writes the SGPR pair itself -- nothing else
//   m0 & m1 & ~done_m          s_and_b64 / s_andn2_b64; `m == 0` is s_cmp_eq_u64 (or the SCC of the last s_and) + s_cbranch
//   lane_of(m)                 the mask as this lane's predicate again: the selector of a v_cndmask / the exec mask of a branch, no instruction
// __ballot(a && b && !done) instead is lowered as s_and_b64 (the conjunction IS a mask already) -> v_cndmask_b32 v, 0, 1 -> v_cmp_ne_u32 0, v:
// two vector instructions per vote in kernels that are bound by vector issue, and a loop-carried `bool` takes the same round trip through a
// VGPR at every use.  NaN: ballot the comparison AS WRITTEN and complement the mask -- !(a < b) is `lanes & ~vote(a < b)`, never vote(a >= b).
// Every vote sits where all 64 lanes execute (the walks' control flow is wave-uniform); lane_of needs a wave-uniform mask, which the
// result of votes and scalar algebra is.  Do not move a comparison into the body of an `if (lane_of(..))`: its vote would miss lanes.
// --------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
typedef unsigned long long lanemask;
__device__ __forceinline__ lanemask vote(bool one_comparison) { return __builtin_amdgcn_ballot_w64(one_comparison); }
__device__ __forceinline__ lanemask lanes_if(bool wave_uniform) { return wave_uniform ? ~0ull : 0ull; }      // a scalar condition as a mask (s_cselect_b64)
__device__ __forceinline__ bool lane_of(lanemask m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
#endif

}  // namespace sr
