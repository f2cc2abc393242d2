// sr_api.cpp -- the C ABI of libsoftray_hip.so (include/softray.h): scene ownership, H2D staging,
// per-frame constant preparation and kernel dispatch.  There is no CPU compute path in here: a scene
// without a HIP device refuses every compute call with SR_ERR_NO_DEVICE.
// Compile with -ffp-contract=off (the per-frame constants must round like the reference's C#).
#include "../../include/softray.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sr_device.h"
#include "sr_host.h"
#include "sr_rccl.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return SR_ERR_HIP;
}
#define SR_HIP(call)                                         \
    do {                                                     \
        hipError_t e__ = (call);                             \
        if (e__ != hipSuccess) return hip_fail(e__, #call);  \
    } while (0)

int rccl_fail(const sr::RcclApi* api, int rc, const char* what) {
    g_err = std::string(what) + ": " + (api && api->GetErrorString ? api->GetErrorString(rc) : "RCCL error") + " (" + std::to_string(rc) + ")";
    return SR_ERR_HIP;
}
#define SR_RCCL(api, call)                                        \
    do {                                                          \
        int r__ = (call);                                         \
        if (r__ != 0) return rccl_fail(api, r__, #call);          \
    } while (0)

// growable device buffer
struct DBuf {
    void*  p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap && p) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = std::max<size_t>(bytes, 256);
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    template <class T> hipError_t upload(const std::vector<T>& v) {
        hipError_t e = reserve(v.size() * sizeof(T));
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

}  // namespace

// the ordered copies' boxes are fitted to their live records (tight_boxes_device) on the lowest kTightCut levels of the wide tree
// (< 0: all of them); SR_DBG_KERNEL_SWITCH 72: neither copy, 73: the camera copy only, 74: the light copy only, 75 .. 79: both on the lowest 1 .. 5 levels
constexpr int kTightNone = -2, kTightCut = -1;

struct sr_scene {
    int device = -1;
    // sr_create_multi: this scene only dispatches to one complete scene per device (the model is replicated, a frame is split
    // into interleaved 16-row strips); empty for an ordinary scene
    std::vector<sr_scene*> parts;
    // host copies (what Renderer keeps between frames)
    std::vector<double>   v9;
    std::vector<uint32_t> argb;
    double bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};
    double vmin[3] = {0, 0, 0}, vmax[3] = {0, 0, 0};   // bounds of the vertices themselves (the caller's box need not be tight, nor, in brute-force mode, contain them)
    bool have_model = false;
    size_t ntris = 0;                      // triangles of the model (a part of a multi-device scene keeps the count, not the arrays)
    // (part of a multi-device scene) the scene whose HOST arrays -- vertices, records, reference tree, SAH nodes and order -- this
    // part uploads from: the model lives once on the host however many devices render it
    const sr_scene* host_src = nullptr;
    // sr_set_triangles_device: the model is on the device only -- v9, argb and tri_recs are empty (and tris_dirty is false: sync_geometry
    // must not upload them) until a consumer of the host arrays asks for them (ensure_host_model)
    bool host_model_stale = false;
    std::vector<sr::Rec128> tri_recs;      // geometry_simple, Renderer.cs:1452-1469
    std::vector<sr::Rec128> extra_recs;    // ExtraGeometryToRaytrace
    sr::RootBox root{};
    sr::RefTree ref;
    sr::Bvh     bvh;
    bool        bvh_on_device = false;   // built by sr_lbvh.hip: no host copy of the nodes
    size_t      bvh_num_nodes = 0;
    // device state
    DBuf d_tris, d_extra, d_rnodes, d_rboxes, d_rleaf, d_bnodes, d_btris, d_bslab, d_v9, d_bcam;
    DBuf d_bounds;                       // sr_set_triangles_device: the bounds kernels' partials, the six doubles of the result in front
    // sr_refit_triangles_device (a device-built own BVH only): the wide tree's level ranges (collapse_bvh4_device), the binary nodes'
    // depths (a byte each, made at the tree's first refit) and the triangles' fp32 boxes in leaf order; all belong to one tree
    std::vector<int> b4_level_first;
    DBuf d_bdepth, d_tbox;
    bool bdepth_valid = false;
    double cam_origin[3] = {0, 0, 0};    // ray origin the camera-cone records in d_bcam (and the node order of d_b4cam) were made for
    bool   cam_valid = false;
    // penumbra-plane records of the packet shaft walk (k_light_cones): made for one (tree, record order, light ball); like d_bcam they follow
    // the records' positions, so they are invalidated wherever cam_valid and b4light_valid are
    DBuf   d_blight;
    bool   blight_valid = false;
    double blight_pos[3] = {0, 0, 0}, blight_radius = 0;
    DBuf   d_binter;                     // interior byte of every BVH record (k_interior_flags); follows the records' positions like d_bcam
    bool   interior_valid = false;
    // four-wide tree of the packet walks: build-order nodes + the two per-frame ordered copies (camera origin / point light)
    DBuf d_b4, d_b4cam, d_b4light;
    size_t b4_num = 0;
    int    b4_depth = 0;
    bool   b4cam_valid = false, b4light_valid = false;
    int    b4cam_known = 0, b4light_known = 0;   // axes on which the ordered copy holds (near, far) planes (sr_device.h)
    int    b4cam_tight = kTightNone, b4light_tight = kTightNone;   // depth cut-off the copy's boxes were fitted with (sr_tight_boxes.h), kTightNone: the base boxes
    // k_facing_partition: the leaves' records grouped by which of {camera rays, shadow sample rays} can hit them, for one (origin, light)
    DBuf   d_rng_cam, d_rng_light;
    bool   part_valid = false, part_cam = false, part_light = false;
    double part_origin[3] = {0, 0, 0}, part_lightpos[3] = {0, 0, 0}, part_radius = 0;
    double b4_light[3] = {0, 0, 0};      // light position the order of d_b4light was made for
    double b4_light_radius = 0;          // ... and the light radius (which axes the light's ball lies outside of depends on it)
    // sr_debug_counters [5..7] of the last frame, host bookkeeping: {b4light_known | b4cam_known << 4 of the ordered copies the frame walked,
    // persistent shaft walks launched, those of them that walked a tile order made by an earlier frame}
    uint32_t dbg_frame[3] = {0, 0, 0};
    // the per-origin / per-light records above are written on whatever stream the frame that needs them runs on: `pre_ready` is
    // recorded after every rewrite and waited for by every frame (another stream may use them next), `pre_used` is recorded at the
    // end of every frame that read them and waited for before the next rewrite
    hipEvent_t pre_ready = nullptr, pre_used = nullptr;
    bool pre_ready_set = false, pre_used_set = false;
    DBuf d_shadow_cache, d_static_claim, d_static_hits;
    // rayTraceAmbientOcclusion (SR_F_AMBIENT_OCCLUSION): the 128^3 cache a Renderer keeps for its life and the claim words of one frame.  A host-only
    // scene keeps the bytes sr_set_ao_cache gave it on the host (empty vector: all zeros)
    DBuf d_ao_cache, d_ao_claim;
    // sr_ao_points: a pass's draw table, the jump coefficients of its chunk strides (uploaded once) and the call's words of device state
    DBuf d_aop_table, d_aop_rows, d_aop_state;
    DBuf d_pp_state;                     // sr_path_points: a pass's window, table size and ray counters
    bool aop_rows_ready = false;
    std::unique_ptr<sr::NetRandom> aop_host_random;   // (host tables) the Random of the call being enqueued, at ...
    uint64_t aop_host_drawn = 0;                      // ... this many units (generators / points) of ...
    uint32_t aop_host_ints = 0;                       // ... this many draws each
    bool ao_cache_empty = true;          // the device cache must be zeroed before its next use (a new Renderer / a new model)
    std::vector<uint8_t> ao_cache_host;
    std::vector<uint8_t> shadow_cache_host;   // sr_set_shadow_cache on a host-only scene (sr_get_shadow_cache reads it back)
    int32_t ao_table_seed = 0;           // random_seed of the frame being enqueued (read by PipelineLaunch::ao_table)
    int  ao_table_rc = SR_OK;            // why the frame's draw table was refused (PipelineLaunch::ao_table)
    // rayTraceLightField (SR_F_LIGHT_FIELD): the 4 N^4 uint32 entries a Renderer's LightFieldColorMethod keeps for its life (allocated on first use),
    // one claim bit per entry (all zero between frames) and the 2N x N patch centres of the canonical rays.  A host-only scene keeps the
    // entries sr_set_light_field gave it on the host (empty vector: all zeros)
    DBuf d_lf_cache, d_lf_claim, d_lf_points;
    int32_t lf_res = 64;                 // lightFieldRes, Renderer.cs:93
    bool lf_shadows = false;             // sr_set_light_field_shadows: SR_F_LIGHT_FIELD | SR_F_SHADOWS (dynamic) is accepted; a setting, like lf_res
    bool lf_interp = false;              // sr_set_light_field_interpolation: SR_F_LIGHT_FIELD frames blend the 16 entries around a sample (a setting, like lf_shadows)
    int32_t lf_points_res = 0;           // the resolution d_lf_points was made for (0: none)
    bool lf_cache_empty = true;          // the device cache (and the claim bits) must be zeroed before their next use
    std::vector<uint32_t> lf_cache_host;
    // LightFieldStoresTriangles = true (sr_set_light_field_triangles): SR_F_LIGHT_FIELD frames and sr_bake_light_field run LightFieldTriMethod on a SECOND
    // table of 4 N^4 uint32 (0 empty, 1 the canonical ray hit nothing, t + 2 triangle t) with claim bits of its own; neither table touches the other.
    // d_rhandle: Triangle.HandleToLeafNode per triangle (RefTree::handle_leaf), uploaded with the reference tree
    bool lf_tris = false;
    DBuf d_lft_cache, d_lft_claim, d_rhandle;
    bool lft_cache_empty = true;
    std::vector<uint32_t> lft_cache_host;
    // path tracing (SR_F_PATH_TRACING) and ambient occlusion: the InternalSample() ints of Random(pt_table_seed), 3 per sample of the largest row
    // block (300 per generator of the fullest one) a frame has asked for so far; made once per (seed, length) and kept for later frames
    DBuf d_pt_table;
    int32_t pt_table_seed = 0;
    size_t  pt_table_samples = 0;
    // (part of a multi-device scene, path tracing) hits per image row of the frame's row range: the part's own rows after the first phase,
    // every part's after the exchange (multi_render); the hits that precede each of the part's compact rows inside its row block
    DBuf d_pt_row_hits, d_pt_row_k0;
    hipEvent_t pt_counted = nullptr;     // ... the part's counts of the current frame have reached pt_counts_host of the multi scene
    // (multi-device scene) where the parts' row counts meet: portable pinned host memory, one word per row of the range
    void* pt_counts_host = nullptr; size_t pt_counts_cap = 0;
    int32_t last_parts = 1;              // sr_last_frame_parts
    // rayTraceVoxels (SR_F_VOXELS): the N^3 grid (N = vox_res) of the current model, made by sr_build_voxels / the first voxel frame and dropped by
    // sr_set_triangles.  A scene with a device keeps it there (colours, normals, occupancy bits); a host-only scene on the host
    DBuf d_vox_colors, d_vox_normals, d_vox_mask;
    DBuf d_vox_bricks, d_vox_coarse;     // N > 64: one 64-bit word per brick of 4x4x4 cells, one bit per brick (sr_voxels.hip k_vox_bricks)
    int32_t vox_res = sr::kVoxelGrid;    // sr_set_voxel_res; 64 = Renderer.cs:1570
    std::vector<uint32_t> vox_colors_host;
    std::vector<double>   vox_normals_host;
    bool vox_valid = false;
    sr::RootBox vox_box{};               // AxisAlignedBox((-1,-1,-1), (1,1,1)), VoxelGrid.cs:38
    bool shadow_cache_empty = true;      // the device cache must be zeroed before its next use
    DBuf d_pixels, d_aa, d_stats, d_io[9];
    // per-frame tables (area-light offsets + row map): pinned host staging and device copies, double-buffered; a slot is
    // rewritten only after the frame that last used it has finished (event), and not at all when the tables are unchanged
    struct FrameTables {
        void* host = nullptr; size_t host_cap = 0;
        DBuf  dev;
        hipEvent_t used = nullptr; bool in_flight = false;
        hipEvent_t ready = nullptr; bool ready_set = false;       // recorded after the upload: a frame on ANOTHER stream that reuses the slot waits for it
        size_t off_bytes = 0, map_bytes = 0;
    } tables[2];
    int tables_cur = 0;
    bool tables_valid = false;
    // per-band scratch of the pipeline.  Two sets + two internal streams: the two halves of a frame run concurrently, so that
    // the short, latency-bound tail kernels of one half (second shaft round, fallback walks) overlap the other half's work
    static constexpr int kMaxSplit = 4;
    struct BandScratch {
        DBuf hits, hits2, bounce_levels, bounce_nlev, bounce_prep, bounce_res, bounce_stack, samples, counters, fallback, fallback_state, fallback_rays, fallback_ovf, ray_sort, ray_sort_temp;
        DBuf pt_flags, pt_index, pt_totals, pt_carry;   // path tracing: hit flags, hit-index scan, row-block carries (sr_pipeline.hip k_pt_*)
        DBuf ao_escapes;                   // ambient occlusion: escaped probes, then the byte, per generator (sr_pipeline.hip k_ao_*)
        DBuf lf_cells, lf_list;            // light field: cache index per sample, the cells the band fills (sr_pipeline.hip k_lf_*)
        DBuf lf_fracs;                     // ... interpolating: the four fractions of every sample, from k_lfi_lookup to k_lfi_apply
        DBuf lf_stage;                     // ... with shadows: the staged colour of every slot of the fill's / a bake pass's hit queue (triangle table: the samples that need the full trace)
        DBuf accum;                        // escape counts per sample index of a chunked (> 128 samples) shadow stage; zero between frames
        DBuf tile_cost, tile_order;        // walk length per 8x8 tile of the last shaft launch / the next one's longest-first lists
        unsigned long long tile_order_tag = 0;   // the tile grid tile_order was made for (0: none)
        DBuf tile_hint[2];                 // umbra hint per 8x8 tile: what the last shaft launch left / what the next one writes (sr_umbra_hint.h)
        int tile_hint_cur = 0;             // the one the next launch writes
        uint64_t tile_hint_epoch = 0;      // sr_scene::records_epoch the words were made under (another: both arrays are refilled with "absent")
        DBuf rlist[sr::kShaftRounds], rstate[sr::kShaftRounds], rcount[sr::kShaftRounds], rcand[sr::kShaftRounds];
        hipStream_t stream = nullptr;
        hipEvent_t  done = nullptr;
        bool used_last_frame = false;
        void release() {
            tile_cost.release(); tile_order.release(); tile_order_tag = 0;
            tile_hint[0].release(); tile_hint[1].release(); tile_hint_cur = 0; tile_hint_epoch = 0;
            DBuf* b[] = {&hits, &hits2, &bounce_levels, &bounce_nlev, &bounce_prep, &bounce_res, &bounce_stack, &samples, &counters, &fallback, &fallback_state, &fallback_rays, &fallback_ovf, &ray_sort, &ray_sort_temp, &accum, &ao_escapes, &lf_cells, &lf_list, &lf_fracs, &lf_stage, &pt_flags, &pt_index, &pt_totals, &pt_carry};
            for (DBuf* x : b) x->release();
            for (int r = 0; r < sr::kShaftRounds; ++r) { rlist[r].release(); rstate[r].release(); rcount[r].release(); rcand[r].release(); }
            if (stream) (void)hipStreamDestroy(stream);
            if (done) (void)hipEventDestroy(done);
            stream = nullptr; done = nullptr;
        }
    } scratch[kMaxSplit];
    hipEvent_t fork = nullptr;
    hipEvent_t multi_done = nullptr;     // (part of a multi-device scene) this part's strips of the current frame are rendered
    // RCCL strip gather: one communicator per process-per-GPU scene (sr_rccl_init), or one per part of a multi-device
    // scene (sr_set_gather(SR_GATHER_RCCL): ncclCommInitAll); rank 0 / the first part receives into d_gather (compact, rank after rank)
    sr::RcclComm comm = nullptr;
    int rccl_world = 0, rccl_rank = -1;
    std::vector<sr::RcclComm> comms;
    int gather_kind = 0;
    DBuf d_gather;
    // the blocking calls (sr_render) never use the null stream: frames are enqueued on io_stream, their way back to the host runs on
    // copy_stream band by band (an event per row band: a band is copied while the next ones render)
    hipStream_t io_stream = nullptr, copy_stream = nullptr;
    struct BandRec { hipEvent_t ev; int band, row_begin, row_count; };
    std::vector<hipEvent_t> band_ev_pool;
    size_t band_ev_used = 0;
    std::vector<BandRec> band_recs;
    bool collect_bands = false;
    bool can_peer = true;                // (part of a multi-device scene) the first part's device can read this part's memory
    void* stage_host = nullptr; size_t stage_cap = 0;   // (part without peer access) pinned staging of its strips
    hipEvent_t staged = nullptr;
    int num_cus = 0;
    bool tris_dirty = true, extra_dirty = true, ref_dirty = true, bvh_dirty = true;
    // counts the changes of the own BVH's triangle records (a new model, a new tree, a refit): whatever names records by index across frames
    // -- the shaft walk's umbra hints -- is dropped when it changes.  Starts at 1: a fresh scratch set's 0 never matches
    uint64_t records_epoch = 1;
    std::vector<double>  offsets_host;
    std::vector<int32_t> rowmap_host;
    // kernel timing: one HIP event pair per launch, accumulated until sr_reset_kernel_times()
    std::vector<hipEvent_t> ev[sr::K_COUNT];       // [2*i] start, [2*i+1] stop
    int  ev_used[sr::K_COUNT] = {};
    uint64_t last_stats[SR_STATS_COUNT] = {};
    int64_t dbg[SR_DBG_COUNT];             // sr_debug_set hooks, -1 = default (never read from the environment)
    sr_scene() { for (auto& d : dbg) d = -1; }
};

namespace {

const int kMaxShaftSamples = 1024;       // area-light samples the shaft path takes (in chunks of 128); more: one lane per hit point (k_shadow)
const long long kMaxPathTable = 256ll << 20;   // bytes of the path tracer's random table (include/softray.h SR_F_PATH_TRACING)
const int kAoRes = 128;                  // staticShadowRes, the resolution Renderer hands AmbientOcclusionMethod (Renderer.cs:1635)
const size_t kAoCells = (size_t)kAoRes * kAoRes * kAoRes;
// cells per pass of sr_bake_light_field with shadows: what the pass's hit queue (64 B per cell), staging buffer and the shadow stage's
// candidate lists (about 0.6 KB per cell) are sized for -- 2.6 GB of scratch at 2^22, whatever the size of the table
const long long kBakeShadowPassCells = 1ll << 22;
const int kMaxLightFieldRes = 128;       // 4 N^4 entries: 4 GiB at 128 (and the reference's coordinates are bytes: 2 N - 1 <= 255)
size_t lf_entries(int n) { return (size_t)4 * n * n * n * n; }
const int kMaxTreeDepth = 62;            // (depth + 2) stack levels x 256 lanes x 4 B = 64 KB of LDS per workgroup

int use_device(sr_scene* s) {
    if (s->device < 0) return fail(SR_ERR_NO_DEVICE, "host-only scene: no HIP device bound (compute is never emulated on the CPU)");
    SR_HIP(hipSetDevice(s->device));
    return SR_OK;
}

// axes on which the ball of `radius` about `p` lies outside the root box's slab (by more than the shadow probe offset and the boxes'
// padding): known = those axes, beyond = those of them on which p lies ABOVE the box.  The camera is a point (radius 0); a light's ball
// is its area-light samples: a sample that reaches back into the slab makes the shafts' direction along that axis depend on the hit
// point (extra geometry can lie beyond the light), so that axis is not known
void point_outside_axes(const sr::RootBox& root, const double p[3], double radius, int& known, int& beyond) {
    known = beyond = 0;
    for (int a = 0; a < 3; ++a) {
        const double margin = 0.01 + 1e-3 * (root.max[a] - root.min[a]) + radius;
        if (p[a] > root.max[a] + margin) { known |= 1 << a; beyond |= 1 << a; }
        else if (p[a] < root.min[a] - margin) known |= 1 << a;
    }
}

// the four-wide tree of the packet walks = the binary tree collapsed on the host (sr_host.cpp collapse_bvh4)
int upload_wide_tree(sr_scene* s, const sr::BvhNode* nodes, size_t num_nodes) {
    std::vector<sr::Bvh4Node> wide;
    s->b4_depth = sr::collapse_bvh4(nodes, num_nodes, wide);
    s->b4_num = wide.size();
    s->b4cam_valid = s->b4light_valid = false;
    s->blight_valid = false;
    s->part_valid = false;
    s->records_epoch++;
    if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));       // a frame in flight may still be walking the old tree's copies
    SR_HIP(s->d_b4.upload(wide));
    SR_HIP(s->d_b4cam.reserve(wide.size() * sizeof(sr::Bvh4Node)));
    SR_HIP(s->d_b4light.reserve(wide.size() * sizeof(sr::Bvh4Node)));
    return SR_OK;
}

int sync_geometry(sr_scene* s, uint32_t need_mode) {
    const sr_scene* h = s->host_src ? s->host_src : s;              // where the host arrays are
    if (s->tris_dirty) { SR_HIP(s->d_tris.upload(h->tri_recs)); SR_HIP(s->d_v9.upload(h->v9)); s->tris_dirty = false; s->cam_valid = false; s->blight_valid = false; s->interior_valid = false; s->records_epoch++; }
    if (s->extra_dirty) { SR_HIP(s->d_extra.upload(s->extra_recs)); s->extra_dirty = false; }
    if (need_mode == SR_MODE_REF_TREE && s->ref_dirty) {
        SR_HIP(s->d_rnodes.upload(h->ref.nodes));
        SR_HIP(s->d_rboxes.upload(h->ref.leaf_boxes));
        SR_HIP(s->d_rleaf.upload(h->ref.leaf_tris));
        SR_HIP(s->d_rhandle.upload(h->ref.handle_leaf));
        s->ref_dirty = false;
    }
    if (need_mode == SR_MODE_BVH && s->bvh_dirty && !s->bvh_on_device) {
        SR_HIP(s->d_bnodes.upload(h->bvh.nodes));
        // the leaf-order copies of the FP64 records and the fp32 shaft records are made on the device from the TriangleIndex-order
        // arrays that are there already: only the order (4 B per triangle) travels
        const size_t n = h->bvh.order.size();
        DBuf d_order, d_slab;
        SR_HIP(d_order.upload(h->bvh.order));
        SR_HIP(d_slab.reserve(n * sizeof(sr::TriSlab)));
        SR_HIP(sr::make_slabs_device((const double*)s->d_v9.p, (int)n, s->root, (sr::TriSlab*)d_slab.p, nullptr));
        SR_HIP(s->d_btris.reserve(n * sizeof(sr::Rec128)));
        SR_HIP(s->d_bslab.reserve(n * sizeof(sr::TriSlab)));
        SR_HIP(sr::gather_records_device((int)n, (const unsigned int*)d_order.p, (const sr::Rec128*)s->d_tris.p, (sr::Rec128*)s->d_btris.p,
                                         (const sr::TriSlab*)d_slab.p, (sr::TriSlab*)s->d_bslab.p, nullptr));
        SR_HIP(hipDeviceSynchronize());
        d_order.release();
        d_slab.release();
        s->bvh_num_nodes = h->bvh.nodes.size();
        s->bvh_dirty = false;
        s->cam_valid = false; s->blight_valid = false; s->interior_valid = false;
        s->records_epoch++;
        int rc = upload_wide_tree(s, h->bvh.nodes.data(), h->bvh.nodes.size());
        if (rc) return rc;
    }
    return SR_OK;
}

sr::DevScene dev_scene(const sr_scene* s) {
    sr::DevScene d{};
    d.tris = (const sr::Rec128*)s->d_tris.p; d.ntris = (int32_t)s->ntris;
    d.extra = (const sr::Rec128*)s->d_extra.p; d.nextra = (int32_t)s->extra_recs.size();
    d.rnodes = (const sr::RefNode*)s->d_rnodes.p; d.rboxes = (const sr::LeafBox*)s->d_rboxes.p; d.rleaf = (const int32_t*)s->d_rleaf.p;
    d.rdepth = s->ref.tree_depth;
    d.bnodes = (const sr::BvhNode*)s->d_bnodes.p; d.btris = (const sr::Rec128*)s->d_btris.p; d.bdepth = s->bvh.depth;
    d.bslab = (const sr::TriSlab*)s->d_bslab.p;
    d.binter = (const uint8_t*)s->d_binter.p;
    d.bcam = s->cam_valid ? (const sr::CamCone*)s->d_bcam.p : nullptr;
    d.blight = s->blight_valid ? (const sr::LightCone*)s->d_blight.p : nullptr;
    d.v9 = (const double*)s->d_v9.p;
    // the four-wide walks stack up to three entries per level: a private walk needs (3 depth + 2) x 1 KB of LDS per workgroup, a packet
    // walk (3 depth + 2) x 528 B; a tree too deep for that is walked in its binary form (a pathological scene, not a large one:
    // 10 M triangles give depth 14).  Seen so far: private walks off the wide tree (b4depth >= 21) from a chain of shrinking triangles
    // at one per leaf and from the device build's deepest accepted tree; packet walks off it (b4depth >= 41) from the cluster staircase
    // of the tests (wide_deep: depth 60, wide depth 48 on the MI355X), where the partition, the cone records and both ordered copies are
    // still made and k_primary / k_hits / k_origin_rays and the first shaft round take the binary packet walks
    const size_t lv4 = (size_t)(3 * s->b4_depth + 2);
    const bool wide_private = s->b4_num > 0 && lv4 * 1024 <= 65536, wide_packets = s->b4_num > 0 && lv4 * 528 <= 65536;
    d.b4 = wide_private ? (const sr::Bvh4Node*)s->d_b4.p : nullptr;
    d.b4cam = (wide_packets && s->b4cam_valid && s->cam_valid) ? (const sr::Bvh4Node*)s->d_b4cam.p : nullptr;
    d.b4light = (wide_packets && s->b4light_valid) ? (const sr::Bvh4Node*)s->d_b4light.p : nullptr;
    d.b4depth = s->b4_depth;
    d.b4cam_known = s->b4cam_known; d.b4light_known = s->b4light_known;
    d.bnode_bits = 1;
    while ((1ull << d.bnode_bits) < s->bvh_num_nodes + 1 && d.bnode_bits < 26) d.bnode_bits++;
    d.root = s->root;
    d.shadow_cache = (uint8_t*)s->d_shadow_cache.p;
    return d;
}

int check_mode(const sr_scene* s, int mode) {
    if (!s->have_model || s->ntris == 0) return fail(SR_ERR_NO_MODEL, "no model: Render() returns without drawing (Renderer.cs:736-739)");
    if (mode == SR_MODE_REF_TREE && !s->ref.built) return fail(SR_ERR_NOT_BUILT, "SR_MODE_REF_TREE needs sr_build(1 << SR_MODE_REF_TREE)");
    // one stack word per level and lane in LDS: (depth + 2) x 256 x 4 bytes must fit the 64 KB a workgroup may ask for
    if (mode == SR_MODE_REF_TREE && s->ref.tree_depth > kMaxTreeDepth) return fail(SR_ERR_UNSUPPORTED, "reference tree deeper than 62 levels does not fit the LDS traversal stacks");
    if (mode == SR_MODE_BVH && !s->bvh.built) return fail(SR_ERR_NOT_BUILT, "SR_MODE_BVH needs sr_build(1 << SR_MODE_BVH)");
    if (mode != SR_MODE_REF_TREE && mode != SR_MODE_BRUTE && mode != SR_MODE_BVH) return fail(SR_ERR_INVALID_ARG, "unknown trace mode");
    return SR_OK;
}

bool row_owned(const sr_frame* f, int r) {
    if (f->strip_count <= 0) return true;
    return ((r / f->strip_rows) % f->strip_count) == f->strip_index;
}

// SR_F_PATH_TRACING: the combinations the reference would allow and the library does not build (include/softray.h)
int check_path_tracing(const sr_frame* f) {
    if (!(f->flags & SR_F_PATH_TRACING)) return SR_OK;
    if (f->flags & SR_F_SHADOWS) return fail(SR_ERR_UNSUPPORTED, "path tracing together with shadows (dynamic or static) is not supported");
    if (f->max_bounces > 0) return fail(SR_ERR_UNSUPPORTED, "path tracing together with mirror bounces (max_bounces > 0) is not supported");
    if (f->flags & SR_F_SINGLE_KERNEL) return fail(SR_ERR_UNSUPPORTED, "path tracing is not built into the one-kernel renderer (SR_F_SINGLE_KERNEL)");
    return SR_OK;
}

// SR_F_AMBIENT_OCCLUSION: what draws from the same Random, fills another cache with the probes' hit points, or has no surface point
// (include/softray.h); the one-band rule is checked where the bands are laid out (render_common)
int check_ambient_occlusion(const sr_frame* f) {
    if (!(f->flags & SR_F_AMBIENT_OCCLUSION)) return SR_OK;
    if (f->flags & SR_F_PATH_TRACING) return fail(SR_ERR_UNSUPPORTED, "ambient occlusion together with path tracing is not supported (both draw from the row block's Random)");
    if (f->flags & SR_F_VOXELS) return fail(SR_ERR_UNSUPPORTED, "ambient occlusion together with voxel rendering is not supported (a voxel hit has no position)");
    if ((f->flags & SR_F_STATIC_SHADOWS) && (f->flags & SR_F_SHADOWS))
        return fail(SR_ERR_UNSUPPORTED, "ambient occlusion together with static shadows is not supported (the probes' hit points would fill the shadow cache)");
    if (f->max_bounces > 0) return fail(SR_ERR_UNSUPPORTED, "ambient occlusion together with mirror bounces (max_bounces > 0) is not supported");
    if (f->flags & SR_F_SINGLE_KERNEL) return fail(SR_ERR_UNSUPPORTED, "ambient occlusion is not built into the one-kernel renderer (SR_F_SINGLE_KERNEL)");
    if (f->strip_count > 0) return fail(SR_ERR_UNSUPPORTED, "ambient occlusion with row strips: the cache is filled in one order over the whole frame");
    return SR_OK;
}

// SR_F_LIGHT_FIELD: the colour light field replaces the camera rays' walk; the decorators that need a surface point per camera sample (or
// whose caches the canonical rays would fill) are not composable with it in one sitting (include/softray.h)
// (sr_set_light_field_shadows lets DYNAMIC shadows through: the canonical rays' hits take the frame's shadow stage, the table stores
// shadowed colours)
int check_light_field(const sr_frame* f, bool dynamic_shadows_allowed) {
    if (!(f->flags & SR_F_LIGHT_FIELD)) return SR_OK;
    if ((f->flags & SR_F_SHADOWS) && !(dynamic_shadows_allowed && !(f->flags & SR_F_STATIC_SHADOWS))) return fail(SR_ERR_UNSUPPORTED, "light field together with shadows (dynamic or static) is not supported (a cell stores a colour, not a surface point)");
    if (f->flags & SR_F_AMBIENT_OCCLUSION) return fail(SR_ERR_UNSUPPORTED, "light field together with ambient occlusion is not supported (a cell stores a colour, not a surface point)");
    if (f->flags & SR_F_PATH_TRACING) return fail(SR_ERR_UNSUPPORTED, "light field together with path tracing is not supported (a cell stores a colour, not a surface point)");
    if (f->flags & SR_F_VOXELS) return fail(SR_ERR_UNSUPPORTED, "light field together with voxel rendering is not supported");
    if (f->max_bounces > 0) return fail(SR_ERR_UNSUPPORTED, "light field together with mirror bounces (max_bounces > 0) is not supported");
    if (f->flags & SR_F_SINGLE_KERNEL) return fail(SR_ERR_UNSUPPORTED, "light field is not built into the one-kernel renderer (SR_F_SINGLE_KERNEL)");
    if (f->strip_count > 0) return fail(SR_ERR_UNSUPPORTED, "light field with row strips: the cache lives on one device and is filled by the whole frame");
    return SR_OK;
}

// SR_F_VOXELS: the decorators whose result on a voxel hit is the reference's rayFrac = 0 artefact (unpinned) and the one-kernel renderer
int check_voxels(const sr_frame* f) {
    if (!(f->flags & SR_F_VOXELS)) return SR_OK;
    if (f->flags & SR_F_SHADOWS) return fail(SR_ERR_UNSUPPORTED, "voxel rendering together with shadows (dynamic or static) is not supported");
    if (f->flags & SR_F_PATH_TRACING) return fail(SR_ERR_UNSUPPORTED, "voxel rendering together with path tracing is not supported");
    if (f->max_bounces > 0) return fail(SR_ERR_UNSUPPORTED, "voxel rendering together with mirror bounces (max_bounces > 0) is not supported");
    if (f->flags & SR_F_SINGLE_KERNEL) return fail(SR_ERR_UNSUPPORTED, "voxel rendering is not built into the one-kernel renderer (SR_F_SINGLE_KERNEL)");
    return SR_OK;
}

// what the frame's geometry needs: a voxel frame only triangles (it ignores trace_mode), any other frame its trace mode's structure
int check_frame_mode(const sr_scene* s, const sr_frame* f) {
    if (f->flags & SR_F_VOXELS) {
        if (!s->have_model || s->ntris == 0) return fail(SR_ERR_NO_MODEL, "no model: Render() returns without drawing (Renderer.cs:736-739)");
        return SR_OK;
    }
    int rc = check_mode(s, f->trace_mode);
    // LightFieldTriMethod's second stage walks Triangle.HandleToLeafNode: the reference tree, whatever traces the full rays
    if (!rc && s->lf_tris && (f->flags & SR_F_LIGHT_FIELD)) rc = check_mode(s, SR_MODE_REF_TREE);
    return rc;
}

// `s`: the scene whose settings decide what a frame may combine (nullptr: the defaults)
int validate_frame(const sr_frame* f, const sr_scene* s = nullptr) {
    if (!f) return fail(SR_ERR_INVALID_ARG, "frame is NULL");
    if (f->width <= 0 || f->height <= 0) return fail(SR_ERR_INVALID_ARG, "surface size must be positive");
    if (f->sub_pixel_res < 1 || f->sub_pixel_res > 64) return fail(SR_ERR_INVALID_ARG, "sub_pixel_res out of range");
    if (f->strip_count < 0 || (f->strip_count > 0 && (f->strip_rows <= 0 || f->strip_index < 0 || f->strip_index >= f->strip_count)))
        return fail(SR_ERR_INVALID_ARG, "bad strip parameters");
    if (f->shadow_samples < 0 || f->shadow_samples > 4096) return fail(SR_ERR_INVALID_ARG, "shadow_samples out of range");
    if ((long long)f->width * f->sub_pixel_res > (1ll << 24) || (long long)f->height > (1ll << 24)) return fail(SR_ERR_INVALID_ARG, "surface too large");
    if (f->max_bounces < 0 || f->max_bounces > 16 || !(f->reflectivity >= 0.0 && f->reflectivity <= 1.0))
        return fail(SR_ERR_INVALID_ARG, "max_bounces must be 0..16 and reflectivity 0..1");
    // LightFieldTriMethod (sr_set_light_field_triangles): every refusal of a colour light-field frame, shadows in both forms whatever
    // sr_set_light_field_shadows says (the reference's shadow rays go through the decorator too: not built), and no brute-force mode -- the
    // method never traces the triangle list
    const bool lft = s && s->lf_tris && (f->flags & SR_F_LIGHT_FIELD);
    int rc = check_light_field(f, s && s->lf_shadows && !lft);
    if (!rc && lft && f->trace_mode == SR_MODE_BRUTE)
        rc = fail(SR_ERR_UNSUPPORTED, "triangle light field (sr_set_light_field_triangles) with SR_MODE_BRUTE is not supported: LightFieldTriMethod reads the spatial subdivision");
    if (!rc) rc = check_ambient_occlusion(f);
    if (!rc) rc = check_voxels(f);
    return rc ? rc : check_path_tracing(f);
}

void clamp_rows(const sr_frame* f, int& a, int& b) {                  // Renderer.cs:1652-1653
    a = std::min(std::max(0, f->start_row), f->height - 1);
    b = std::min(std::max(0, f->end_row), f->height - 1);                 // b < a: the row loop does not run (Renderer.cs:1666)
}

// everything RaytraceGeometry derives per frame (Renderer.cs:1510-1528, 1717)
int prepare_frame(sr_scene* s, const sr_frame* f, sr::FrameConst& fc) {
    std::memset(&fc, 0, sizeof(fc));
    fc.width = f->width; fc.height = f->height;
    fc.sub_pixel_res = f->sub_pixel_res;
    fc.background = f->background_argb | 0xFF000000u;               // BackgroundColorWithAlpha, :325-331
    fc.flags = f->flags;
    fc.shadow_samples = f->shadow_samples > 0 ? f->shadow_samples : 100;   // ShadowMethod.cs:9
    fc.strip_rows = f->strip_rows; fc.strip_count = f->strip_count; fc.strip_index = f->strip_index;
    int a, b;
    clamp_rows(f, a, b);
    fc.start_row = a;
    s->rowmap_host.clear();
    for (int r = a; r <= b; ++r) if (row_owned(f, r)) s->rowmap_host.push_back(r);
    fc.num_rows = (int32_t)s->rowmap_host.size();
    fc.first_row = fc.num_rows ? s->rowmap_host[0] : 0;
    for (int i = 0; i < 12; ++i) { fc.t[i] = f->transform[i]; fc.it[i] = f->inv_transform[i]; }
    fc.position_z = f->position_z; fc.fov_depth = f->fov_depth;
    fc.focal_depth = f->focal_depth; fc.focal_blur_strength = f->focal_blur_strength;
    fc.ambient = f->ambient; fc.shininess = f->shininess;
    const double* it = fc.it;
    for (int i = 0; i < 3; ++i) { fc.light_dir_view[i] = f->light_dir_view[i]; fc.light_pos_view[i] = f->light_pos_view[i]; }
    const double* ld = f->light_dir_view; const double* lp = f->light_pos_view;
    for (int r = 0; r < 3; ++r) {
        // Instance.TransformDirectionReverse (Instance.cs:229-235) and TransformPosFromView (:192-209, which
        // IGNORES its un-projection and returns inverseTransform(3x4) * pos -- kept)
        fc.light_dir_model[r] = ld[0] * it[4 * r] + ld[1] * it[4 * r + 1] + ld[2] * it[4 * r + 2];
        fc.light_pos_model[r] = lp[0] * it[4 * r] + lp[1] * it[4 * r + 1] + lp[2] * it[4 * r + 2] + it[4 * r + 3];
        const double vx = 0.0, vy = 0.0, vz = -f->position_z;         // new Vector(0, 0, -instance.Position.z), :1717
        fc.start_world[r] = vx * it[4 * r] + vy * it[4 * r + 1] + vz * it[4 * r + 2];
    }
    fc.aspect = (double)f->height / (double)f->width;               // Renderer.cs:621
    fc.max_bounces = f->max_bounces;
    fc.reflectivity = f->reflectivity;

    // area-light offsets (ShadowMethod.cs:63-73)
    s->offsets_host.resize((size_t)fc.shadow_samples * 3);
    if (f->area_light_offsets) std::memcpy(s->offsets_host.data(), f->area_light_offsets, s->offsets_host.size() * sizeof(double));
    else sr::area_light_offsets(f->random_seed, fc.shadow_samples, s->offsets_host.data());
    double r2max = 0;
    for (int i = 0; i < fc.shadow_samples; ++i) {
        const double* o = &s->offsets_host[3 * i];
        r2max = std::max(r2max, o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
    }
    fc.light_radius = std::sqrt(r2max);
    fc.debug = s->dbg[SR_DBG_KERNEL_SWITCH] > 0 ? (int32_t)s->dbg[SR_DBG_KERNEL_SWITCH] : 0;
    return SR_OK;
}

int ensure_io_streams(sr_scene* s) {
    if (!s->io_stream) SR_HIP(hipStreamCreateWithFlags(&s->io_stream, hipStreamNonBlocking));
    if (!s->copy_stream) SR_HIP(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
    return SR_OK;
}

// pins the caller's (pageable) surface for the duration of one blocking call, so that the band copies are real asynchronous DMA
// straight into it; the library does not keep the pointer.  Small frames and refusals (already registered, odd mappings) simply
// take the runtime's pageable path.
struct HostPin {
    void* p = nullptr;
    HostPin(void* ptr, size_t bytes) {
        if (bytes < ((size_t)4 << 20)) return;
        if (hipHostRegister(ptr, bytes, hipHostRegisterPortable) == hipSuccess) p = ptr;
        else (void)hipGetLastError();
    }
    ~HostPin() { if (p) (void)hipHostUnregister(p); }
};

const int kMaxTimedLaunches = 4096;

// hands out the event pair for the next launch of kernel k (nullptr once the pool is exhausted)
int next_events(sr_scene* s, int k, hipEvent_t& a, hipEvent_t& b) {
    a = b = nullptr;
    if (s->dbg[SR_DBG_KERNEL_TIMING] <= 0) return SR_OK;          // opt-in: no events inside an ordinary frame
    if (s->ev_used[k] >= kMaxTimedLaunches) return SR_OK;
    if ((size_t)(2 * s->ev_used[k] + 2) > s->ev[k].size()) {
        hipEvent_t e0, e1;
        SR_HIP(hipEventCreate(&e0));
        SR_HIP(hipEventCreate(&e1));
        s->ev[k].push_back(e0);
        s->ev[k].push_back(e1);
    }
    a = s->ev[k][2 * s->ev_used[k]];
    b = s->ev[k][2 * s->ev_used[k] + 1];
    s->ev_used[k]++;
    return SR_OK;
}

// the `get_events` of every launch struct (sr_device.h): `user` is the scene, no pair is no timing
void timing_events(void* user, int kid, hipEvent_t* a, hipEvent_t* b) {
    hipEvent_t x = nullptr, y = nullptr;
    if (next_events((sr_scene*)user, kid, x, y) != SR_OK) { x = y = nullptr; }
    *a = x; *b = y;
}

int ensure_num_cus(sr_scene* s) {
    if (s->num_cus) return SR_OK;
    hipDeviceProp_t prop;
    SR_HIP(hipGetDeviceProperties(&prop, s->device));
    s->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    return SR_OK;
}

// frames of one scene run in submission order whatever streams they are given: the scene's scratch (hit queues, candidate lists,
// counters) and its per-origin / per-light records belong to one frame -- or one batch call -- at a time.  Entering makes `stream` wait
// for `pre_used` (a no-op on the same stream; `entered` is the refusal of that wait); leaving, by whatever return, records it again: when
// everything the frame enqueues is on its stream
struct StreamOrder {
    sr_scene* s; hipStream_t st; int entered;
    StreamOrder(sr_scene* scene, hipStream_t stream) : s(scene), st(stream), entered(wait()) {}
    StreamOrder(const StreamOrder&) = delete;
    ~StreamOrder() {
        if (entered != SR_OK) return;
        if (!s->pre_used && hipEventCreateWithFlags(&s->pre_used, hipEventDisableTiming) != hipSuccess) return;
        if (hipEventRecord(s->pre_used, st) == hipSuccess) s->pre_used_set = true;
    }
private:
    int wait() {
        if (s->pre_used_set) SR_HIP(hipStreamWaitEvent(st, s->pre_used, 0));
        return SR_OK;
    }
};

// a draw table made on the host (sr_ao_points, sr_path_points): System.Random(seed) itself, one draw after the other, from unit `first`
// on, `ints` draws per unit (300 per generator, 3 per point).  fill_host_table is the launch structs' callback (`user`: the scene): the passes
// ask in ascending order, and the call waits once per pass
void start_host_table(sr_scene* s, int32_t seed, uint64_t first, uint32_t ints) {
    s->aop_host_random.reset(new sr::NetRandom(seed));
    for (uint64_t i = 0; i < first * ints; ++i) (void)s->aop_host_random->next();
    s->aop_host_drawn = first;
    s->aop_host_ints = ints;
}
hipError_t fill_host_table(void* user, uint64_t base, uint32_t count, int32_t* d_table, hipStream_t st) {
    sr_scene* sc = (sr_scene*)user;
    if (base != sc->aop_host_drawn) return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;                             // (a pass of sr_ao_points without a generator; sr_path_points has none)
    std::vector<int32_t> ints((size_t)count * sc->aop_host_ints);
    for (int32_t& v : ints) v = sc->aop_host_random->next();
    sc->aop_host_drawn += count;
    hipError_t e = hipMemcpyAsync(d_table, ints.data(), ints.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(st);                               // (`ints` leaves scope)
}

// TriMeshToVoxelGrid.Convert for the scene's model, once per model.  A scene with a device runs sr_voxels.hip's voxeliser from the device triangle
// records (on `stream`; the call waits for it: the number of (cell, triangle) pairs sizes the sort's buffers); a host-only scene runs the plain
// host loop (sr_host.cpp voxelise_host)
const long long kMaxVoxelPairs = 1ll << 30;
sr::VoxelGridDev voxel_grid_dev(const sr_scene* s) {
    const bool two = s->vox_res > sr::kVoxelGrid;
    return sr::VoxelGridDev{(uint32_t*)s->d_vox_colors.p, (double*)s->d_vox_normals.p, (uint32_t*)s->d_vox_mask.p,
                            two ? (unsigned long long*)s->d_vox_bricks.p : nullptr, two ? (uint32_t*)s->d_vox_coarse.p : nullptr, s->vox_res,
                            (s->vox_res + 3) / 4};
}
int ensure_voxels(sr_scene* s, hipStream_t stream) {
    if (s->vox_valid) return SR_OK;
    const int N = s->vox_res;
    const size_t cells = (size_t)N * N * N;
    const double lo[3] = {-1, -1, -1}, hi[3] = {1, 1, 1};
    s->vox_box = sr::make_root_box(lo, hi);
    if (s->device < 0) {
        s->vox_colors_host.assign(cells, 0u);
        s->vox_normals_host.assign(cells * 3, 0.0);
        sr::voxelise_host(s->v9.data(), s->tri_recs.data(), s->ntris, N, s->vox_colors_host.data(), s->vox_normals_host.data());
        s->vox_valid = true;
        return SR_OK;
    }
    if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));       // a frame in flight may still walk the old grid
    SR_HIP(s->d_vox_colors.reserve(cells * 4));
    SR_HIP(s->d_vox_normals.reserve(cells * 3 * sizeof(double)));
    SR_HIP(s->d_vox_mask.reserve(sr::voxel_mask_words(N) * 4));
    if (N > sr::kVoxelGrid) {
        const int nb = (N + 3) / 4;
        SR_HIP(s->d_vox_bricks.reserve((size_t)nb * nb * nb * 8));
        SR_HIP(s->d_vox_coarse.reserve(sr::voxel_mask_words(nb) * 4));
    }
    const int n = (int)s->ntris;
    DBuf counts, offsets, temp, pairs, first_last;
    struct Free { DBuf* b[5]; ~Free() { for (DBuf* x : b) x->release(); } } free_all{{&counts, &offsets, &temp, &pairs, &first_last}};
    size_t scan_bytes = 0;
    SR_HIP(sr::voxel_count_cells(nullptr, n, N, nullptr, nullptr, nullptr, &scan_bytes, stream));
    SR_HIP(counts.reserve((size_t)n * 8));
    SR_HIP(offsets.reserve((size_t)n * 8));
    SR_HIP(temp.reserve(scan_bytes));
    SR_HIP(first_last.reserve(cells * 2 * 4));
    hipEvent_t e0, e1;
    int rc = next_events(s, sr::K_VOXELISE, e0, e1);
    if (rc) return rc;
    if (e0) SR_HIP(hipEventRecord(e0, stream));
    SR_HIP(sr::voxel_count_cells((const double*)s->d_v9.p, n, N, (unsigned long long*)counts.p, (unsigned long long*)offsets.p, temp.p, &scan_bytes, stream));
    unsigned long long tail[2] = {0, 0};
    SR_HIP(hipMemcpyAsync(&tail[0], (const unsigned long long*)offsets.p + (n - 1), 8, hipMemcpyDeviceToHost, stream));
    SR_HIP(hipMemcpyAsync(&tail[1], (const unsigned long long*)counts.p + (n - 1), 8, hipMemcpyDeviceToHost, stream));
    SR_HIP(hipStreamSynchronize(stream));
    const unsigned long long npairs = tail[0] + tail[1];
    if (npairs > (unsigned long long)kMaxVoxelPairs)
        return fail(SR_ERR_UNSUPPORTED, "voxel grid: the triangles' boxes of cells hold more than 2^30 (cell, triangle) pairs");
    const size_t sort_bytes = npairs ? sr::voxel_sort_temp_bytes((unsigned int)npairs, sr::voxel_key_bits(N)) : 0;
    if (npairs) {
        SR_HIP(pairs.reserve((size_t)npairs * 4 * 4));
        if (sort_bytes > temp.cap) SR_HIP(temp.reserve(sort_bytes));
    }
    const sr::VoxelGridDev grid = voxel_grid_dev(s);
    SR_HIP(sr::voxel_fill_grid((const double*)s->d_v9.p, (const sr::Rec128*)s->d_tris.p, n, (const unsigned long long*)offsets.p, (unsigned int)npairs,
                               (unsigned int*)pairs.p, temp.p, sort_bytes, (unsigned int*)first_last.p, grid, stream));
    if (e1) SR_HIP(hipEventRecord(e1, stream));
    SR_HIP(hipStreamSynchronize(stream));                                 // the scratch is freed on return
    s->vox_valid = true;
    return SR_OK;
}

// the table of Random(seed)'s InternalSample() ints, at least 3 * triples of them (path tracing: 3 per sample, ambient occlusion: 300 per
// generator -- the same sequence); kept per (seed, length)
int ensure_draw_table(sr_scene* s, int32_t seed, size_t triples) {
    if (s->d_pt_table.p && s->pt_table_seed == seed && s->pt_table_samples >= triples) return SR_OK;
    if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));      // a frame in flight may still read the old table
    std::vector<int32_t> ints(triples * 3);
    sr::NetRandom random(seed);
    for (int32_t& v : ints) v = random.next();
    s->pt_table_samples = 0;
    SR_HIP(s->d_pt_table.upload(ints));
    s->pt_table_seed = seed;
    s->pt_table_samples = triples;
    return SR_OK;
}

// the scene's light field on the device: the table and its claim bits (allocated on first use, zeroed on `stream` when the scene starts
// as a new Renderer) and the patch centres of the current resolution.  What a light-field frame and sr_bake_light_field begin with
int ensure_light_field_points(sr_scene* s);
int ensure_light_field(sr_scene* s, hipStream_t stream) {
    const int N = s->lf_res;
    const size_t entries = lf_entries(N), claim_bytes = (entries + 31) / 32 * 4;
    if (!s->d_lf_cache.p || !s->d_lf_claim.p) s->lf_cache_empty = true;
    SR_HIP(s->d_lf_cache.reserve(entries * 4));
    SR_HIP(s->d_lf_claim.reserve(claim_bytes));
    if (s->lf_cache_empty) {
        SR_HIP(hipMemsetAsync(s->d_lf_cache.p, 0, entries * 4, stream));
        SR_HIP(hipMemsetAsync(s->d_lf_claim.p, 0, claim_bytes, stream));
        s->lf_cache_empty = false;
    }
    return ensure_light_field_points(s);
}

// the 2N x N patch centres of the current resolution (both tables' canonical rays)
int ensure_light_field_points(sr_scene* s) {
    const int N = s->lf_res;
    if (s->lf_points_res != N) {
        // Coord4DToRay + Sphere.ConvertLine (LightField4D.cs:253-273, Sphere.cs:122-142) with the host's sin / cos: the device calls neither
        std::vector<double> pts((size_t)2 * N * N * 3);
        const double max_h = (double)(N * 2 - 1), max_w = (double)(N - 1), radius = 0.866, pi = 3.14159265358979323846;
        for (int i = 0; i < 2 * N; ++i) {
            const double h = (((double)i + 0.5) / max_h - 0.5) * pi * 2;
            for (int j = 0; j < N; ++j) {
                const double w = (((double)j + 0.5) / max_w - 0.5) * pi;
                const double horiz = std::cos(w) * radius;
                double* p = &pts[((size_t)i * N + j) * 3];
                p[0] = std::sin(h) * horiz; p[1] = std::sin(w) * radius; p[2] = std::cos(h) * horiz;
            }
        }
        if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));      // a frame in flight may still read the old table
        s->lf_points_res = 0;
        SR_HIP(s->d_lf_points.upload(pts));
        s->lf_points_res = N;
    }
    return SR_OK;
}

// the same for the triangle table (sr_set_light_field_triangles): its own entries and claim bits, the patch centres are shared (read-only)
int ensure_light_field_tris(sr_scene* s, hipStream_t stream) {
    const size_t entries = lf_entries(s->lf_res), claim_bytes = (entries + 31) / 32 * 4;
    if (!s->d_lft_cache.p || !s->d_lft_claim.p) s->lft_cache_empty = true;
    SR_HIP(s->d_lft_cache.reserve(entries * 4));
    SR_HIP(s->d_lft_claim.reserve(claim_bytes));
    if (s->lft_cache_empty) {
        SR_HIP(hipMemsetAsync(s->d_lft_cache.p, 0, entries * 4, stream));
        SR_HIP(hipMemsetAsync(s->d_lft_claim.p, 0, claim_bytes, stream));
        s->lft_cache_empty = false;
    }
    return ensure_light_field_points(s);
}

// pt_phase: 0, or the phase (1, 2) of a part of a path-traced frame that multi_render has split (sr_device.h PipelineLaunch::pt_phase)
// sr_bake_light_field with shadows: the bake needs everything a shadowed frame sets up (the light's records and node order, the offset
// table, the shadow stage's scratch), so it runs through render_common with no rows to render
struct LfBakeReq { uint64_t first, count; unsigned long long* filled; };
// sr_shadow_points: the same set-up for the same reason, then passes of the caller's points through the shadow stage (device arrays)
struct PtsReq {
    int64_t n; const double* pos; const double* nrm; const uint32_t* color; uint32_t* out; bool coherent;
    // sr_static_shadow_points: the points go through the static cache (the frame carries SR_F_STATIC_SHADOWS); out / amount each optional
    bool through_cache = false; uint8_t* amount = nullptr; unsigned long long* generators = nullptr;
};
// sr_render_hits: the frame's own set-up of the primary stage (camera cones, ordered node copy, facing partition, row bands), then k_hits
// per band into the caller's device arrays instead of the frame's kernels.  The caller has cleared the decorator switches of `f`
struct HitsReq { sr::HitsOut out; };
// sr_trace_origin_rays: the same set-up for `origin` in the camera's place (the frame `f` is a stand-in: one pixel, no decorator), then passes of
// the caller's directions through k_origin_rays into the caller's device arrays.  with_extra: the root geometry (SR_TARGET_ROOT)
struct OriginReq { double origin[3]; int64_t n; const double* dirs; sr::HitsOut out; bool coherent; bool with_extra; };
// sr_light_field_rays: a light-field frame's set-up (the table, the patch centres, with shadows the shadow stage's records and scratch), then
// passes of the caller's rays through the fused lookup, the frame's fill stage and the finish kernel (device arrays)
struct LfRaysReq { int64_t n; const double* starts; const double* dirs; uint32_t* out; uint8_t* inside; unsigned long long* filled; };

// points per pass of sr_shadow_points: the bake's rule (SR_DBG_BAND_SAMPLES shrinks the pass)
const long long kPtsPassPoints = 1ll << 22;

// what render_common is asked for besides a whole frame: nothing, a phase of a split path-traced frame, or one of the requests above (a
// call site passes `&req`: the request's type says which)
struct RenderAsk {
    int pt_phase = 0;
    const LfBakeReq* bake = nullptr;
    const PtsReq* pts = nullptr;
    const HitsReq* hreq = nullptr;
    const OriginReq* org = nullptr;
    const LfRaysReq* lfr = nullptr;
    RenderAsk() {}
    RenderAsk(const LfBakeReq* r) : bake(r) {}
    RenderAsk(const PtsReq* r) : pts(r) {}
    RenderAsk(const HitsReq* r) : hreq(r) {}
    RenderAsk(const OriginReq* r) : org(r) {}
    RenderAsk(const LfRaysReq* r) : lfr(r) {}
    static RenderAsk phase(int p) { RenderAsk a; a.pt_phase = p; return a; }
};

int render_common(sr_scene* s, const sr_frame* f, uint32_t* d_pixels, hipStream_t stream, unsigned long long* d_stats, const RenderAsk& ask = RenderAsk()) {
    const int pt_phase = ask.pt_phase;
    const LfBakeReq* const bake = ask.bake;
    const PtsReq* const pts = ask.pts;
    const HitsReq* const hreq = ask.hreq;
    const OriginReq* const org = ask.org;
    const LfRaysReq* const lfr = ask.lfr;
    for (uint32_t& c : s->dbg_frame) c = 0;
    sr::FrameConst fc;
    int rc = check_path_tracing(f);                                 // (sr_rccl_render makes strips of its own after validate_frame)
    if (rc) return rc;
    const bool voxels = (f->flags & SR_F_VOXELS) != 0;                // (the voxel grid replaces the model's tree AND the extra geometry, Renderer.cs:1568-1588)
    // strips that the caller (or sr_rccl_render) made: this one call on this one scene cannot know how many samples hit in the rows the other
    // ranks render.  The strips of a multi-device scene are the library's own: multi_render exchanges the counts between the two phases
    if ((f->flags & SR_F_PATH_TRACING) && f->strip_count > 1 && !pt_phase)
        return fail(SR_ERR_UNSUPPORTED, "path tracing with row strips: a rank would need the hit counts of rows it does not render");
    if ((rc = prepare_frame(s, f, fc))) return rc;
    if (org) for (int a = 0; a < 3; ++a) fc.start_world[a] = org->origin[a];   // everything per-origin below is keyed to fc.start_world
    if ((rc = sync_geometry(s, voxels ? ~0u : (uint32_t)f->trace_mode))) return rc;
    // LightFieldTriMethod: stage 2 reads the reference tree's leaves whatever trace_mode walks the full rays
    const bool lft = s->lf_tris && (f->flags & SR_F_LIGHT_FIELD) && !bake && !pts;
    if (lft && (rc = sync_geometry(s, SR_MODE_REF_TREE))) return rc;
    if (voxels && (rc = ensure_voxels(s, stream))) return rc;
    if (fc.num_rows == 0 && !bake && !pts && !org && !lfr) return SR_OK;
    // ---- frames of one scene run in submission order whatever streams they are given ----
    StreamOrder order(s, stream);
    if (order.entered) return order.entered;
    // ---- frame tables -> device ----
    const size_t off_bytes = (s->offsets_host.size() * sizeof(double) + 255) / 256 * 256, map_bytes = s->rowmap_host.size() * sizeof(int32_t);
    {
        sr_scene::FrameTables* T = &s->tables[s->tables_cur];
        const bool same = s->tables_valid && T->off_bytes == off_bytes && T->map_bytes == map_bytes && T->host &&
                          std::memcmp(T->host, s->offsets_host.data(), s->offsets_host.size() * sizeof(double)) == 0 &&
                          std::memcmp((const char*)T->host + off_bytes, s->rowmap_host.data(), map_bytes) == 0;
        if (!same) {
            s->tables_cur ^= 1;
            T = &s->tables[s->tables_cur];
            if (T->in_flight) { SR_HIP(hipEventSynchronize(T->used)); T->in_flight = false; }
            const size_t need = off_bytes + map_bytes;
            if (need > T->host_cap) {
                if (T->host) SR_HIP(hipHostFree(T->host));
                T->host = nullptr; T->host_cap = 0;
                SR_HIP(hipHostMalloc(&T->host, need + 4096, hipHostMallocDefault));
                T->host_cap = need + 4096;
            }
            SR_HIP(T->dev.reserve(need));
            std::memcpy(T->host, s->offsets_host.data(), s->offsets_host.size() * sizeof(double));
            std::memcpy((char*)T->host + off_bytes, s->rowmap_host.data(), map_bytes);
            T->off_bytes = off_bytes; T->map_bytes = map_bytes;
            SR_HIP(hipMemcpyAsync(T->dev.p, T->host, need, hipMemcpyHostToDevice, stream));
            if (!T->ready) SR_HIP(hipEventCreateWithFlags(&T->ready, hipEventDisableTiming));
            SR_HIP(hipEventRecord(T->ready, stream));
            T->ready_set = true;
            s->tables_valid = true;
        } else if (T->ready_set) {
            SR_HIP(hipStreamWaitEvent(stream, T->ready, 0));        // uploaded on another stream, perhaps
        }
    }
    sr_scene::FrameTables& FT = s->tables[s->tables_cur];
    const double* d_offsets = (const double*)FT.dev.p;
    const int32_t* d_rowmap = (const int32_t*)((const char*)FT.dev.p + off_bytes);
    struct MarkUsed {                                               // the slot is busy until everything enqueued below has run
        sr_scene::FrameTables& t; hipStream_t st;
        ~MarkUsed() {
            if (!t.used && hipEventCreateWithFlags(&t.used, hipEventDisableTiming) != hipSuccess) return;
            if (hipEventRecord(t.used, st) == hipSuccess) t.in_flight = true;
        }
    } mark_used{FT, stream};
    if (voxels) {
        // ---- one walk kernel per row band (+ k_resolve with sub-pixel samples); the rows are independent: strips and parts need no exchange ----
        const long long n2v = (long long)fc.sub_pixel_res * fc.sub_pixel_res;
        const long long budget = s->dbg[SR_DBG_BAND_SAMPLES] > 0 ? s->dbg[SR_DBG_BAND_SAMPLES] : (32ll << 20);
        long long rows = std::max<long long>(16, (budget / ((long long)fc.width * n2v)) / 16 * 16);
        rows = std::min<long long>(rows, ((long long)fc.num_rows + 15) / 16 * 16);
        sr_scene::BandScratch& B = s->scratch[0];
        if (n2v > 1) SR_HIP(B.samples.reserve((size_t)(rows * fc.width * n2v) * 4));
        if ((rc = ensure_num_cus(s))) return rc;
        sr::VoxelLaunch V{};
        V.fc = fc;
        V.box = s->vox_box;
        V.grid = voxel_grid_dev(s);
        V.row_map = d_rowmap;
        V.pixels = d_pixels;
        V.samples = (uint32_t*)B.samples.p;
        V.band_rows = (int32_t)rows;
        V.persistent_blocks = s->num_cus * 3;                         // 3 workgroups x 32 KB of occupancy bits per CU (137 VGPRs: 3 waves per SIMD)
        V.global_table = s->dbg[SR_DBG_KERNEL_SWITCH] == 41;          // (hook: no LDS mask, a step reads the colour table)
        V.flat_mask = s->dbg[SR_DBG_KERNEL_SWITCH] == 42;             // (hook, N > 64: one level, a step reads the occupancy bits in global memory)
        V.stats = d_stats;
        V.stream = stream;
        V.user = s;
        V.get_events = timing_events;
        SR_HIP(sr::launch_voxel_frame(V));
        return SR_OK;
    }
    const bool static_shadows = (f->flags & SR_F_STATIC_SHADOWS) && (f->flags & SR_F_SHADOWS);
    if (static_shadows) {
        if ((f->flags & SR_F_SINGLE_KERNEL) || f->max_bounces > 0 || f->strip_count > 1)
            return fail(SR_ERR_UNSUPPORTED, "static shadows need the whole frame in one pipeline call (no strips, mirror bounces or SR_F_SINGLE_KERNEL)");
        SR_HIP(s->d_shadow_cache.reserve(sr::pipeline_static_cells()));
        SR_HIP(s->d_static_claim.reserve(sr::pipeline_static_cells() * 8));
        if (s->shadow_cache_empty) {
            SR_HIP(hipMemsetAsync(s->d_shadow_cache.p, 0, sr::pipeline_static_cells(), stream));
            s->shadow_cache_empty = false;
        }
    } else {
        fc.flags &= ~(uint32_t)SR_F_STATIC_SHADOWS;          // meaningless without SR_F_SHADOWS (RendererTests.cs:420)
    }
    // mirror bounces: wavefront pipeline (k_primary -> k_bounce per level -> k_fold) on the own BVH without shadows; every other
    // combination is traced inline by the one-kernel renderer
    const bool bounce_pipe = f->max_bounces > 0 && f->trace_mode == SR_MODE_BVH && !(f->flags & SR_F_SHADOWS) && !(f->flags & SR_F_SINGLE_KERNEL);
    if ((f->flags & SR_F_SINGLE_KERNEL) || (f->max_bounces > 0 && !bounce_pipe)) {
        sr::RenderLaunch L{};
        L.sc = dev_scene(s);
        L.fc = fc;
        L.mode = f->trace_mode;
        L.offsets = d_offsets;
        L.row_map = d_rowmap;
        L.pixels = d_pixels;
        L.stats = d_stats;
        L.stream = stream;
        hipEvent_t e0, e1;
        if ((rc = next_events(s, sr::K_RENDER, e0, e1))) return rc;
        if (e0) SR_HIP(hipEventRecord(e0, stream));
        SR_HIP(sr::launch_render(L));
        if (e1) SR_HIP(hipEventRecord(e1, stream));
        return SR_OK;
    }
    // ---- camera-cone records of the packet primary walk: one pre-pass per (tree, ray origin) ----
    // ---- two proofs that let a frame skip literal shadow rays without changing a byte ----
    // (1) directional light (ShadowMethod.cs:160-166): a sample ray starts at E' + dir * 1000 + offset and runs along +dir, AWAY from
    //     the surface point; whatever it could hit lies at least 1000 |dir| - R from E'.  When that exceeds the diagonal of everything
    //     a hit point or a triangle can be in, no sample of no hit point is occluded: rayEscapeCount = softShadowQuality, the factor
    //     is the constant (byte)(1.0 * 255) (applied by k_primary).  Extra geometry (unbounded planes) and the static cache (its
    //     cells are renderer state) keep the literal path.
    // (a light-field frame keeps the literal rays: the constant factor is k_primary's)
    bool pts_escape = false;
    if ((fc.flags & SR_F_SHADOWS) && !(fc.flags & SR_F_POINT_LIGHT) && (!static_shadows || pts) && s->extra_recs.empty() && !(f->flags & SR_F_LIGHT_FIELD) &&
        !(f->flags & (SR_F_SINGLE_KERNEL | SR_F_PER_LANE_SHADOWS)) && f->max_bounces == 0 && s->dbg[SR_DBG_LITERAL_SHADOWS] <= 0) {
        double diag2 = 0, len2 = 0;
        for (int a = 0; a < 3; ++a) {
            const double e = std::max(s->vmax[a], s->root.max[a]) - std::min(s->vmin[a], s->root.min[a]) + 0.004;   // + the probe offset, both ends
            diag2 += e * e;
            len2 += fc.light_dir_model[a] * fc.light_dir_model[a];
        }
        if (1000.0 * std::sqrt(len2) - fc.light_radius > std::sqrt(diag2) * 1.001 + 0.01) {
            // (sr_shadow_points: a caller's point need not lie where a hit point does.  The proof holds for a probe end inside the box
            // the diagonal was taken of; k_pts_ingest finishes those points and queues the others for the literal rays.  sr_static_shadow_points:
            // the same for the generators, k_ssp_select stores their byte -- a static FRAME keeps the literal rays)
            if (pts) pts_escape = true;
            else fc.flags = (fc.flags & ~(uint32_t)SR_F_SHADOWS) | sr::kFlagAllSamplesEscape;
        }
    }
    // (2) a REF_TREE frame: the shadow rays only answer "is there a hit with rayFrac <= 1.0", which the own BVH answers identically
    //     (include/softray.h SR_MODE_BVH) -- they take the shaft path.  The four statistics of sr_render count the PRIMARY rays, which
    //     keep the literal traversal, so a caller that reads them loses nothing; SR_F_LITERAL_SECONDARY asks for the literal traversal
    //     of the shadow rays too (their counters in sr_last_ray_stats are then the reference tree's)
    const bool shadows_on_bvh = (fc.flags & SR_F_SHADOWS) && f->trace_mode == SR_MODE_REF_TREE && !(f->flags & SR_F_LITERAL_SECONDARY) && s->bvh.built && !static_shadows &&
                                (fc.flags & SR_F_POINT_LIGHT) && fc.shadow_samples <= kMaxShaftSamples && f->max_bounces == 0 &&
                                !(f->flags & (SR_F_SINGLE_KERNEL | SR_F_PER_LANE_SHADOWS)) && s->dbg[SR_DBG_LITERAL_SHADOWS] <= 0;
    if (shadows_on_bvh && (rc = sync_geometry(s, SR_MODE_BVH))) return rc;
    const bool bvh_walks = f->trace_mode == SR_MODE_BVH || shadows_on_bvh;
    const bool wide = bvh_walks && s->b4_num > 0 && s->dbg[SR_DBG_BVH2_PACKETS] <= 0;
    bool rewrote = false;                                             // (frames enqueued earlier have been waited for: see pre_used above)
    // ---- which records can the frame's camera rays / shadow sample rays hit at all?  (k_facing_partition, sr_pipeline.hip) ----
    const bool lf = (f->flags & SR_F_LIGHT_FIELD) != 0;              // (no camera ray is walked: none of the packet walk's per-origin records is needed)
    // sr_trace_origin_rays from an origin no frame's camera stands at (include/softray.h): further from the root box's centre than 2^20 box diagonals
    // on some axis (the FP64 rounding of k_cam_cones' vertex - origin comes within reach of the fp32 margin of cone_rejects), or so far that a
    // cone-plane product with a direction of 2^40 can overflow fp32 (|w| |d| 3 < 2^127 needs the furthest vertex within 2^42.5).  Private walks
    bool org_far = false;
    if (org) {
        double diag2 = 0, away = 0;
        for (int a = 0; a < 3; ++a) {
            const double e = s->root.max[a] - s->root.min[a];
            diag2 += e * e;
            away = std::max(away, std::fabs(org->origin[a] - s->root.centre[a]));
        }
        const double diag = std::sqrt(diag2);
        org_far = !(away <= 0x1p20 * diag) || !(away * 1.7320508075688772 + 0.5 * diag <= 0x1p42);
    }
    const bool pkt_primary = f->trace_mode == SR_MODE_BVH && s->dbg[SR_DBG_PER_LANE_PRIMARY] <= 0 && !((f->flags & SR_F_FOCAL_BLUR) && f->sub_pixel_res > 1) && !lf && !pts && !org_far;
    const bool want_cam = wide && pkt_primary, want_light = wide && (fc.flags & SR_F_SHADOWS) && (fc.flags & SR_F_POINT_LIGHT);
    if ((want_cam || want_light) && s->dbg[SR_DBG_KERNEL_SWITCH] != 71) {
        const auto same3 = [](const double* a, const double* b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; };
        const bool cam_ok = !want_cam || (s->part_cam && same3(s->part_origin, fc.start_world));
        const bool light_ok = !want_light || (s->part_light && same3(s->part_lightpos, fc.light_pos_model) && s->part_radius == fc.light_radius);
        if (!s->part_valid || !cam_ok || !light_ok) {
            SR_HIP(s->d_rng_cam.reserve(s->b4_num * 4 * 8));
            SR_HIP(s->d_rng_light.reserve(s->b4_num * 4 * 8));
            rewrote = true;
            s->part_valid = false;
            s->cam_valid = false; s->b4cam_valid = false; s->b4light_valid = false;      // the records move: cone records and both copies are re-made
            s->blight_valid = false;
            s->interior_valid = false;                                                   // ... and the interior bytes
            SR_HIP(sr::launch_facing_partition((const sr::Bvh4Node*)s->d_b4.p, (int)s->b4_num, (sr::Rec128*)s->d_btris.p, (sr::TriSlab*)s->d_bslab.p,
                                               fc.start_world, want_cam, fc.light_pos_model, fc.light_radius, want_light, s->d_rng_cam.p, s->d_rng_light.p, stream));
            s->part_cam = want_cam; s->part_light = want_light;
            for (int i = 0; i < 3; ++i) { s->part_origin[i] = fc.start_world[i]; s->part_lightpos[i] = fc.light_pos_model[i]; }
            s->part_radius = fc.light_radius;
            s->part_valid = true;
        }
    } else if (s->part_valid && s->dbg[SR_DBG_KERNEL_SWITCH] == 71) {
        s->part_valid = false; s->b4cam_valid = false; s->b4light_valid = false;        // (hook: no live runs -- the copies are re-made without them)
        s->blight_valid = false;
    }
    // ---- the ordered copies' boxes, fitted to the live runs the partition left (sr_tight_boxes.h): part of making a copy, so it
    //      re-runs exactly when b4cam_valid / b4light_valid fall.  A tree without level ranges (host build) and a copy without live runs
    //      (SR_DBG_KERNEL_SWITCH 71) keep the base boxes ----
    const auto tight_wanted = [&](const void* runs, bool light_copy) {
        const int64_t sw = s->dbg[SR_DBG_KERNEL_SWITCH];
        if (!runs || sw == 72 || sw == (light_copy ? 73 : 74) || s->b4_level_first.size() < 2 || s->b4_level_first.back() != (int)s->b4_num || !s->d_v9.p) return kTightNone;
        return sw >= 75 && sw <= 79 ? (int)(sw - 74) : kTightCut;
    };
    const auto tighten = [&](void* copy, const void* runs, int cut) -> int {
        int rc2;
        hipEvent_t e0, e1;
        if ((rc2 = next_events(s, sr::K_TIGHT_BOXES, e0, e1))) return rc2;
        if (e0) SR_HIP(hipEventRecord(e0, stream));
        SR_HIP(sr::tight_boxes_device((const sr::Bvh4Node*)s->d_b4.p, (sr::Bvh4Node*)copy, (int)s->b4_num, s->b4_level_first, runs, (const sr::Rec128*)s->d_btris.p,
                                      (const double*)s->d_v9.p, (int)s->ntris, s->root, cut, stream));
        if (e1) SR_HIP(hipEventRecord(e1, stream));
        return SR_OK;
    };
    // ---- interior bytes of the records in their final order (the shadow classification's umax shortcut) ----
    if (bvh_walks && (fc.flags & SR_F_SHADOWS) && (fc.flags & SR_F_POINT_LIGHT) && s->d_bslab.p && !s->interior_valid) {
        SR_HIP(s->d_binter.reserve(s->ntris));
        rewrote = true;
        SR_HIP(sr::launch_interior_flags(dev_scene(s), (int)s->ntris, (uint8_t*)s->d_binter.p, stream));
        s->interior_valid = true;
    }
    if (pkt_primary) {
        const size_t nt = s->ntris;
        const bool same_origin = s->cam_origin[0] == fc.start_world[0] && s->cam_origin[1] == fc.start_world[1] && s->cam_origin[2] == fc.start_world[2];
        if (!s->cam_valid || !same_origin) {
            SR_HIP(s->d_bcam.reserve(nt * sizeof(sr::CamCone)));
            rewrote = true;
            s->cam_valid = false;
            s->b4cam_valid = false;
            SR_HIP(sr::launch_cam_cones(dev_scene(s), (int)nt, fc.start_world, (sr::CamCone*)s->d_bcam.p, stream));
            for (int i = 0; i < 3; ++i) s->cam_origin[i] = fc.start_world[i];
            s->cam_valid = true;
        }
        if (wide && s->b4cam_valid && s->b4cam_tight != tight_wanted((s->part_valid && s->part_cam) ? s->d_rng_cam.p : nullptr, false)) s->b4cam_valid = false;
        if (wide && !s->b4cam_valid) {                                // the four-wide nodes, children front to back for this origin
            rewrote = true;
            int known, swap;                                      // (a camera ABOVE the box on an axis looks towards smaller coordinates: hi first)
            point_outside_axes(s->root, fc.start_world, 0.0, known, swap);
            // the camera-ordered copy holds (near, far) planes only when that is true on ALL axes (one extra instantiation of k_primary, not seven)
            if (known != 7 || s->dbg[SR_DBG_KERNEL_SWITCH] == 61) known = swap = 0;
            const void* runs = (s->part_valid && s->part_cam) ? s->d_rng_cam.p : nullptr;
            const int cut = tight_wanted(runs, false);
            if (cut != kTightNone) {                                  // boxes of the camera-live records only, then sorted where they lie
                if ((rc = tighten(s->d_b4cam.p, runs, cut))) return rc;
                SR_HIP(sr::launch_order_nodes((const sr::Bvh4Node*)s->d_b4cam.p, (sr::Bvh4Node*)s->d_b4cam.p, (int)s->b4_num, s->root, fc.start_world, false, swap, nullptr, stream));
            } else {
                SR_HIP(sr::launch_order_nodes((const sr::Bvh4Node*)s->d_b4.p, (sr::Bvh4Node*)s->d_b4cam.p, (int)s->b4_num, s->root, fc.start_world, false, swap, runs, stream));
            }
            s->b4cam_tight = cut;
            s->b4cam_known = known;
            s->b4cam_valid = true;
        }
        if (wide && dev_scene(s).b4cam) s->dbg_frame[0] |= (uint32_t)s->b4cam_known << 4;      // (a copy the tree is too deep to walk is no copy walked)
    }
    if (wide && (fc.flags & SR_F_SHADOWS) && (fc.flags & SR_F_POINT_LIGHT)) {
        const bool same_light = s->b4_light[0] == fc.light_pos_model[0] && s->b4_light[1] == fc.light_pos_model[1] && s->b4_light[2] == fc.light_pos_model[2] &&
                                s->b4_light_radius == fc.light_radius;
        const void* lruns = (s->part_valid && s->part_light) ? s->d_rng_light.p : nullptr;
        if (!s->b4light_valid || !same_light || s->b4light_tight != tight_wanted(lruns, true)) {   // ... and nearest-to-the-surface first for this light
            rewrote = true;
            s->b4light_valid = false;
            int known, beyond;                                    // (a light BELOW the box on an axis: every shaft travels towards smaller coordinates there, hi first)
            point_outside_axes(s->root, fc.light_pos_model, fc.light_radius, known, beyond);
            if (s->dbg[SR_DBG_KERNEL_SWITCH] == 62) known = 0;                    // (hook: (lo, hi) planes on every axis)
            const int cut = tight_wanted(lruns, true);
            if (cut != kTightNone) {                                  // boxes of the light-live records only
                if ((rc = tighten(s->d_b4light.p, lruns, cut))) return rc;
                SR_HIP(sr::launch_order_nodes((const sr::Bvh4Node*)s->d_b4light.p, (sr::Bvh4Node*)s->d_b4light.p, (int)s->b4_num, s->root, fc.light_pos_model, true,
                                              known & ~beyond, nullptr, stream));
            } else {
                SR_HIP(sr::launch_order_nodes((const sr::Bvh4Node*)s->d_b4.p, (sr::Bvh4Node*)s->d_b4light.p, (int)s->b4_num, s->root, fc.light_pos_model, true, known & ~beyond,
                                              lruns, stream));
            }
            s->b4light_tight = cut;
            s->b4light_known = known;
            for (int i = 0; i < 3; ++i) s->b4_light[i] = fc.light_pos_model[i];
            s->b4_light_radius = fc.light_radius;
            s->b4light_valid = true;
        }
        if (dev_scene(s).b4light) s->dbg_frame[0] |= (uint32_t)s->b4light_known;
    }
    // ---- penumbra-plane records of the packet shaft walk's triangle filter: one pre-pass per (tree, record order, light ball) ----
    const bool shadows = (fc.flags & SR_F_SHADOWS) != 0;
    // (more than 128 samples: the shaft path runs in chunks of 128, escape counts summed per hit point; not for the static cache)
    const bool shaft = shadows && bvh_walks && (fc.flags & SR_F_POINT_LIGHT) && !(f->flags & SR_F_PER_LANE_SHADOWS) &&
                       (fc.shadow_samples <= 128 || (fc.shadow_samples <= kMaxShaftSamples && !static_shadows));
    if (shaft && wide && s->b4light_valid && dev_scene(s).b4light && !(s->dbg[SR_DBG_PER_LANE_SHAFT] > 0 && (s->dbg[SR_DBG_PER_LANE_SHAFT] & 1)) &&
        s->dbg[SR_DBG_KERNEL_SWITCH] != 96) {
        const bool same_ball = s->blight_pos[0] == fc.light_pos_model[0] && s->blight_pos[1] == fc.light_pos_model[1] && s->blight_pos[2] == fc.light_pos_model[2] &&
                               s->blight_radius == fc.light_radius;
        if (!s->blight_valid || !same_ball) {
            s->blight_valid = false;
            // (a refused reservation is no error: the frame filters with the TriSlab records, like SR_DBG_KERNEL_SWITCH 96)
            if (s->d_blight.reserve(s->ntris * sizeof(sr::LightCone)) == hipSuccess) {
                rewrote = true;
                SR_HIP(sr::launch_light_cones(dev_scene(s), (int)s->ntris, fc.light_pos_model, fc.light_radius, (sr::LightCone*)s->d_blight.p, stream));
                for (int i = 0; i < 3; ++i) s->blight_pos[i] = fc.light_pos_model[i];
                s->blight_radius = fc.light_radius;
                s->blight_valid = true;
            } else {
                (void)hipGetLastError();
            }
        }
    } else if (s->dbg[SR_DBG_KERNEL_SWITCH] == 96) {
        s->blight_valid = false;                                      // (hook: this frame's dev_scene carries no records)
    }
    if (rewrote) {
        if (!s->pre_ready) SR_HIP(hipEventCreateWithFlags(&s->pre_ready, hipEventDisableTiming));
        SR_HIP(hipEventRecord(s->pre_ready, stream));
        s->pre_ready_set = true;
    } else if (s->pre_ready_set) {
        SR_HIP(hipStreamWaitEvent(stream, s->pre_ready, 0));          // written on another stream, perhaps: order this frame after it
    }
    // ---- default: the primary / shadow / resolve pipeline, in row bands ----
    const long long n2 = (long long)fc.sub_pixel_res * fc.sub_pixel_res;
    const bool chunked_shadows = shaft && fc.shadow_samples > 128;
    // samples per band: bounds the hit queue (64 B/sample) and, on the shaft path, the candidate lists (256 B/sample for
    // round 0 + 1/4 of the hits x 1 KB for round 1): 16 Mi samples = one 4096^2 frame = 10 GB of scratch in HBM
    long long kMaxBandSamples = shaft ? (16ll << 20) : (32ll << 20);
    int round_cap[sr::kShaftRounds];
    for (int r = 0; r < sr::kShaftRounds; ++r) round_cap[r] = sr::pipeline_round_cap(r);
    {   // test hooks (sr_debug_set): shrink the bands / candidate lists so that small frames exercise banding, round 2 and the fallback
        if (s->dbg[SR_DBG_BAND_SAMPLES] > 0) kMaxBandSamples = s->dbg[SR_DBG_BAND_SAMPLES];
        if (s->dbg[SR_DBG_ROUND_CAP0] > 0) round_cap[0] = (int)std::min<int64_t>(s->dbg[SR_DBG_ROUND_CAP0], sr::pipeline_round_cap_max(0));
        if (s->dbg[SR_DBG_ROUND_CAP1] > 0) round_cap[1] = (int)std::min<int64_t>(s->dbg[SR_DBG_ROUND_CAP1], sr::pipeline_round_cap_max(1));
        if (s->dbg[SR_DBG_EXACT_SHADOW_TESTS] > 0) round_cap[1] = std::min(round_cap[1], 64);   // k_shadow_test keeps a list in one wave's registers
    }
    // Two halves of the frame (16-row granularity) run as two pipelines on two internal streams, each with its own scratch
    // set; a half that exceeds its share of the band budget is processed in sequential bands on its stream.  A static
    // frame (one global fill order) and shadow-less frames (one kernel) stay whole on the first set.
    int want_split = 2;
    if (s->dbg[SR_DBG_SPLIT] > 0) want_split = (int)std::min<int64_t>(s->dbg[SR_DBG_SPLIT], (int)sr_scene::kMaxSplit);   // experiment hook
    const bool ao = (f->flags & SR_F_AMBIENT_OCCLUSION) != 0, ao_uncached = ao && (f->flags & SR_F_AO_UNCACHED);
    // (a light-field frame stays whole: a band's apply reads the cells the same band's fill stored)
    const bool split = (shadows || bounce_pipe) && !static_shadows && !ao && !lf && !pts && want_split > 1 && fc.num_rows >= 32 * want_split && !(f->flags & SR_F_NO_SPLIT);
    const int halves = split ? want_split : 1;
    const int rows_half = split ? (int)((((long long)fc.num_rows + halves - 1) / halves + 15) / 16 * 16) : fc.num_rows;
    // an interpolating light-field band lists up to 16 cells per sample (never more than the table has).  Without shadows only the fill list
    // grows; with shadows every listed cell may become a hit of the shadow stage, whose scratch is 100+ bytes per hit: the band shrinks to
    // 1/16 of the budget instead, so that the stage's scratch stays what a nearest-lookup frame reserves
    const bool lf_interp = lf && !bake && s->lf_interp && !lft;          // (Interpolate belongs to the colour method)
    const long long budget = kMaxBandSamples / halves / ((lf_interp && shadows) ? 16 : 1);
    // queue capacity counts whole 16x16-pixel tiles: the tile-aligned hit queue of the shaft path gives every wave (8x8 pixels
    // x one sub-sample) 64 entries, also at the right / bottom edge of the frame
    const long long wpad = ((long long)fc.width + 15) / 16 * 16;
    long long band_rows = std::max<long long>(16, (budget / (wpad * n2)) / 16 * 16);
    band_rows = std::min<long long>(band_rows, ((long long)rows_half + 15) / 16 * 16);
    long long band_samples = band_rows * wpad * n2;
    long long lfr_pass = 0;
    if (lfr) {
        // a pass of rays in a band's place: at most kPtsPassPoints (SR_DBG_BAND_SAMPLES: fewer), 1/16 of that where a band shrinks, no more than the call has
        const long long want = (s->dbg[SR_DBG_BAND_SAMPLES] > 0 ? std::min<long long>(s->dbg[SR_DBG_BAND_SAMPLES], kPtsPassPoints) : kPtsPassPoints) / ((lf_interp && shadows) ? 16 : 1);
        lfr_pass = std::max<long long>(1, std::min<long long>(want, lfr->n));
        band_samples = (lfr_pass + 255) / 256 * 256;                    // (the scratch in whole workgroups)
    }
    const long long lf_band_samples = band_samples;                     // per-sample scratch of a light-field band
    const long long lf_list_cells = lf_interp ? std::min<long long>(16 * band_samples, (long long)lf_entries(s->lf_res)) : band_samples;
    if (lf_interp && shadows) band_samples = std::max(band_samples, lf_list_cells);      // the queue, the staging buffer and the stage's lists: one slot per listed cell
    // (sr_light_field_rays: its finish kernel computes them again from the ray)
    const bool lf_carry = lf_interp && !lfr && s->dbg[SR_DBG_KERNEL_SWITCH] != 39;               // (hook 39: the apply kernel computes base cell and fractions again; same frame)
    if (bake) {
        // a bake pass: whole origin patches (2 N^2 cells each), at most kBakeShadowPassCells cells (SR_DBG_BAND_SAMPLES shrinks the pass), at least one patch
        const long long per_origin = 2ll * s->lf_res * s->lf_res;
        const long long want = s->dbg[SR_DBG_BAND_SAMPLES] > 0 ? (long long)s->dbg[SR_DBG_BAND_SAMPLES] : kBakeShadowPassCells;
        band_samples = std::max<long long>(1, want / per_origin) * per_origin;
    }
    long long pts_pass = 0;
    if (pts) {
        // a pass of points: at most kPtsPassPoints (SR_DBG_BAND_SAMPLES shrinks the pass), no more than the call has
        const long long want = s->dbg[SR_DBG_BAND_SAMPLES] > 0 ? (long long)s->dbg[SR_DBG_BAND_SAMPLES] : kPtsPassPoints;
        pts_pass = std::max<long long>(1, std::min<long long>(want, pts->n));
        band_samples = (pts_pass + 255) / 256 * 256;                    // (the scratch in whole workgroups of queue entries)
    }
    long long org_pass = 0;
    if (org) {
        // a pass of rays: at most kPtsPassPoints (SR_DBG_BAND_SAMPLES: fewer), no more than the call has
        const long long want = s->dbg[SR_DBG_BAND_SAMPLES] > 0 ? std::min<long long>(s->dbg[SR_DBG_BAND_SAMPLES], kPtsPassPoints) : kPtsPassPoints;
        org_pass = std::max<long long>(1, std::min<long long>(want, org->n));
        band_samples = (org_pass + 255) / 256 * 256;                    // (the order's scratch in whole workgroups)
    }
    // (hook 37: a pass is queued in input order whatever the caller promised)
    const bool pts_sort = pts && !pts->coherent && s->dbg[SR_DBG_KERNEL_SWITCH] != 37;
    if (shaft && band_samples >= (1ll << 25)) return fail(SR_ERR_UNSUPPORTED, "row band too large for the 25-bit fallback entry ids (surface too wide for this sub-pixel resolution)");
    if (static_shadows && !pts) {
        if (band_rows < fc.num_rows) return fail(SR_ERR_UNSUPPORTED, "static shadows: the frame does not fit one row band");
        SR_HIP(s->d_static_hits.reserve((size_t)std::min<long long>(band_samples, (long long)sr::pipeline_static_cells()) * sr::pipeline_hit_record_bytes()));
    }
    // fallback ray list: one 32-bit id (entry << 7 | sample; bands have < 2^25 entries) per undecided sample.  6 per band
    // sample = 0.4 GB for a 4096^2 frame; whatever it has no room for is taken by the one-wave-per-hit kernel.  Test hook
    // SR_FB_RAY_CAP shrinks it
    long long fallback_ray_cap = std::min<long long>(6 * band_samples, 0xfffffff0ll);
    if (s->dbg[SR_DBG_FB_RAY_CAP] > 0) fallback_ray_cap = s->dbg[SR_DBG_FB_RAY_CAP];
    unsigned round_items[sr::kShaftRounds] = {};
    for (int r = 0; r < sr::kShaftRounds; ++r)      // round 0 sees every hit; each later round is provisioned for 1/4 of the previous one
        round_items[r] = r == 0 ? (unsigned)band_samples : (unsigned)std::max<long long>(1024, (long long)round_items[r - 1] / 4);
    if ((rc = ensure_num_cus(s))) return rc;
    if (split) {
        if (!s->fork) SR_HIP(hipEventCreateWithFlags(&s->fork, hipEventDisableTiming));
        SR_HIP(hipEventRecord(s->fork, stream));                    // the halves start after the caller's earlier work
    }
    // ---- path tracing: the row blocks that each restart Random(random_seed) (Renderer.cs:1655-1666) and the table of its draws ----
    const bool path = (f->flags & SR_F_PATH_TRACING) != 0;
    int pt_block_height = 0, pt_blocks = 0;
    int pt_range_first = 0, pt_range_rows = 0;
    if (path) {
        const long long conc = f->concurrency > 0 ? f->concurrency : 4;
        // (a part of a split frame: the blocks are those of the whole row range, not of the rows the part owns)
        int ra, rb;
        clamp_rows(f, ra, rb);
        pt_range_first = ra; pt_range_rows = rb - ra + 1;
        const int block_rows = pt_phase ? pt_range_rows : fc.num_rows;
        pt_block_height = (int)(((long long)block_rows - 1 + conc) / conc);
        pt_blocks = (block_rows + pt_block_height - 1) / pt_block_height;
        const long long block_samples = (long long)pt_block_height * fc.width * n2;
        if (block_samples * 12 > kMaxPathTable)
            return fail(SR_ERR_UNSUPPORTED, "path tracing: the random table of the largest row block (12 bytes per sample) exceeds 256 MiB; raise concurrency or render row ranges");
        if ((rc = ensure_draw_table(s, f->random_seed, (size_t)block_samples))) return rc;
    }
    // ---- ambient occlusion: the same row blocks; the stage sees every hit record of the frame, so the frame is one pipeline and one band ----
    if (ao) {
        if (band_rows < fc.num_rows) return fail(SR_ERR_UNSUPPORTED, "ambient occlusion: the row range does not fit one row band");
        const long long conc = f->concurrency > 0 ? f->concurrency : 4;
        pt_block_height = (int)(((long long)fc.num_rows - 1 + conc) / conc);
        pt_blocks = (fc.num_rows + pt_block_height - 1) / pt_block_height;
        if (!ao_uncached) {
            SR_HIP(s->d_ao_cache.reserve(kAoCells));
            SR_HIP(s->d_ao_claim.reserve(kAoCells * 8));
            if (s->ao_cache_empty) {
                SR_HIP(hipMemsetAsync(s->d_ao_cache.p, 0, kAoCells, stream));
                s->ao_cache_empty = false;
            }
        }
    }
    // ---- light field: the scene's cache (allocated on first use), its claim bits and the patch centres of this resolution ----
    if (lf && (rc = lft ? ensure_light_field_tris(s, stream) : ensure_light_field(s, stream))) return rc;
    const bool path_walk = path && f->trace_mode == SR_MODE_BVH;
    // (path tracing never runs as two halves: the part's rows are one band when they fit the budget)
    const bool pt_reuse = pt_phase && band_rows >= fc.num_rows;
    if (pt_phase) {
        SR_HIP(s->d_pt_row_hits.reserve((size_t)pt_range_rows * 4));
        SR_HIP(s->d_pt_row_k0.reserve((size_t)fc.num_rows * 4));
        if (pt_phase == 1) SR_HIP(hipMemsetAsync(s->d_pt_row_hits.p, 0, (size_t)pt_range_rows * 4, stream));
    }
    for (auto& sc : s->scratch) sc.used_last_frame = false;
    for (int h = 0; h < halves; ++h) {
        sr_scene::BandScratch& B = s->scratch[h];
        B.used_last_frame = true;
        if (shadows || bounce_pipe || path || ao) SR_HIP(B.hits.reserve((size_t)band_samples * sr::pipeline_hit_record_bytes()));
        if (ao) SR_HIP(B.ao_escapes.reserve((size_t)band_samples * 4));
        if (lfr) {
            // the pending list: its length, then (ray, cell) per ray that met an empty entry (interpolating: the ray alone)
            SR_HIP(B.lf_cells.reserve(((size_t)lf_band_samples * 2 + 2) * 4));
            SR_HIP(B.lf_list.reserve((size_t)lf_list_cells * 4));
        } else if (lf && !bake) {
            if (!lf_interp || lf_carry) SR_HIP(B.lf_cells.reserve((size_t)lf_band_samples * 4));
            if (lf_carry) SR_HIP(B.lf_fracs.reserve((size_t)lf_band_samples * 32));
            SR_HIP(B.lf_list.reserve((size_t)lf_list_cells * 4));
        }
        if (lf && shadows) SR_HIP(B.lf_stage.reserve((size_t)band_samples * 4));
        if (lft) SR_HIP(B.lf_stage.reserve((size_t)lf_band_samples * 4));      // the samples of the band that need the full trace (k_lft_hit -> k_lft_trace)
        if (path || ao) {
            SR_HIP(B.hits2.reserve((size_t)band_samples * sr::pipeline_hit_record_bytes()));
            SR_HIP(B.pt_flags.reserve((size_t)band_samples));
            SR_HIP(B.pt_index.reserve((size_t)band_samples * 4));
            SR_HIP(B.pt_totals.reserve(((size_t)band_samples / (size_t)sr::pipeline_pt_chunk() + 2) * 4));
            SR_HIP(B.pt_carry.reserve((size_t)pt_blocks * 4));
        }
        if (path_walk) {
            // the second rays of a SR_MODE_BVH frame take the incoherent-ray route of the mirror extension: the same scratch
            SR_HIP(B.bounce_prep.reserve((size_t)band_samples * 64));
            SR_HIP(B.bounce_res.reserve((size_t)band_samples * 16));
            const long long deep = std::max(3 * (long long)s->b4_depth + 2, (long long)s->bvh.depth + 2) - sr::pipeline_bounce_lds_levels();
            if (deep > 0) SR_HIP(B.bounce_stack.reserve((size_t)deep * (size_t)s->num_cus * 8 * 256 * 4));
            SR_HIP(B.ray_sort.reserve((size_t)band_samples * 4 * 4));
            SR_HIP(B.ray_sort_temp.reserve(sr::ray_sort_temp_bytes((unsigned)band_samples)));
        }
        if (pts) {
            // the pass as k_pts_ingest leaves it, and its order: by (cell of the point, octant of the normal), or the input's
            SR_HIP(B.hits2.reserve((size_t)band_samples * sr::pipeline_hit_record_bytes()));
            SR_HIP(B.ray_sort.reserve((size_t)band_samples * 4 * 4));
            SR_HIP(B.ray_sort_temp.reserve(sr::point_order_temp_bytes((unsigned)band_samples)));
        }
        if (org) {
            // the order of a pass (dir_order): keys, sorted keys, indices, order + the device sort's own scratch
            SR_HIP(B.ray_sort.reserve((size_t)band_samples * 4 * 4));
            SR_HIP(B.ray_sort_temp.reserve(sr::point_order_temp_bytes((unsigned)band_samples)));
        }
        if (bounce_pipe) {
            // level colours are indexed like the sample buffer: the frame (or compact strip buffer) for one sample per pixel, band-local otherwise
            const size_t idx_space = n2 == 1 ? (size_t)(f->strip_count > 0 ? fc.num_rows : fc.height) * fc.width : (size_t)band_samples;
            SR_HIP(B.hits2.reserve((size_t)band_samples * sr::pipeline_hit_record_bytes()));
            SR_HIP(B.bounce_levels.reserve(idx_space * (size_t)(f->max_bounces + 1) * 4));
            SR_HIP(B.bounce_nlev.reserve(idx_space));
            SR_HIP(B.bounce_prep.reserve((size_t)band_samples * 64));
            SR_HIP(B.bounce_res.reserve((size_t)band_samples * 16));
            // (k_bounce_walk keeps sr::pipeline_bounce_lds_levels() stack levels per lane in LDS, the rest of the worst case here)
            const long long deep = std::max(3 * (long long)s->b4_depth + 2, (long long)s->bvh.depth + 2) - sr::pipeline_bounce_lds_levels();
            if (deep > 0) SR_HIP(B.bounce_stack.reserve((size_t)deep * (size_t)s->num_cus * 8 * 256 * 4));
            // per-level ray order (keys, sorted keys, indices, order) + the device sort's own scratch
            SR_HIP(B.ray_sort.reserve((size_t)band_samples * 4 * 4));
            SR_HIP(B.ray_sort_temp.reserve(sr::ray_sort_temp_bytes((unsigned)band_samples)));
        }
        // (one band per part-frame pipeline: a second band would walk other tiles with the first one's lists)
        // (a light-field frame's queue is compact: no tile grid whose walk lengths the next frame could use)
        const bool order_tiles = shaft && band_rows >= rows_half && !lf && !pts;
        bool hints_fresh = false;                                  // the hint arrays are new, or name another scene's records: "absent" everywhere, on the half's own stream below
        if (order_tiles) {
            const size_t bytes = sr::pipeline_tile_items(fc.width, (int)band_rows, (int)n2) * 4;
            if (bytes > B.tile_cost.cap) B.tile_order_tag = 0;
            SR_HIP(B.tile_cost.reserve(bytes));
            SR_HIP(B.tile_order.reserve(bytes));
            hints_fresh = bytes > B.tile_hint[0].cap || bytes > B.tile_hint[1].cap || !B.tile_hint[0].p || !B.tile_hint[1].p || B.tile_hint_epoch != s->records_epoch;
            SR_HIP(B.tile_hint[0].reserve(bytes));
            SR_HIP(B.tile_hint[1].reserve(bytes));
            B.tile_hint_epoch = s->records_epoch;
        }
        if (shaft) {
            SR_HIP(B.fallback.reserve((size_t)band_samples * 4));
            SR_HIP(B.fallback_state.reserve((size_t)band_samples * sr::pipeline_round_state_bytes()));
            SR_HIP(B.fallback_rays.reserve((size_t)fallback_ray_cap * 4));
            SR_HIP(B.fallback_ovf.reserve((size_t)band_samples * 4));
            for (int r = 0; r < sr::kShaftRounds; ++r) {
                SR_HIP(B.rcount[r].reserve((size_t)round_items[r] * 4));
                SR_HIP(B.rcand[r].reserve((size_t)round_items[r] * round_cap[r] * 4));
                SR_HIP(B.rlist[r].reserve((size_t)round_items[r] * 4));     // round 0: the hits k_shaft left undecided
                if (r > 0) SR_HIP(B.rstate[r].reserve((size_t)round_items[r] * sr::pipeline_round_state_bytes()));
            }
        }
        if (n2 > 1 && !bake && !hreq && !lfr) SR_HIP(B.samples.reserve((size_t)(lf ? lf_band_samples : band_samples) * 4));
        bool accum_fresh = false;
        if (chunked_shadows) {
            // indexed like the sample buffer: the frame (or the compact strips) for one sample per pixel, band-local otherwise (a light field's
            // shadow stage: the staging buffer, one word per queue slot)
            // (sr_shadow_points: a pass's part of `out`, one word per point of the pass)
            const size_t idx_space = (n2 == 1 && !lf && !pts) ? (size_t)(f->strip_count > 0 ? fc.num_rows : fc.height) * fc.width : (size_t)band_samples;
            if (idx_space * 4 > B.accum.cap || !B.accum.p) {
                SR_HIP(B.accum.reserve(idx_space * 4));
                accum_fresh = true;                                // zeroed on the half's own stream below
            }
        }
        SR_HIP(B.counters.reserve(sr::pipeline_counter_bytes()));
        hipStream_t bs = stream;
        // the blocking call runs its part-frame pipelines one after the other on the caller's stream: a finished part travels to the host while
        // the next one renders (side by side both end together and all 64 MiB travel after the last kernel: 9.96 against 9.74 ms; the
        // persistent shaft walk of one part fills the chip anyway).  Hook 85: side by side, as the pipelined frames run
        const bool sequential_parts = s->collect_bands && s->dbg[SR_DBG_KERNEL_SWITCH] != 85;
        if (split && !sequential_parts) {
            if (!B.stream) SR_HIP(hipStreamCreateWithFlags(&B.stream, hipStreamNonBlocking));
            if (!B.done) SR_HIP(hipEventCreateWithFlags(&B.done, hipEventDisableTiming));
            bs = B.stream;
            SR_HIP(hipStreamWaitEvent(bs, s->fork, 0));
        }
        sr::PipelineLaunch P{};
        P.sc = dev_scene(s);
        P.fc = fc;
        P.fc.accum = chunked_shadows ? (uint32_t*)B.accum.p : nullptr;
        P.mode = f->trace_mode;
        P.offsets = d_offsets;
        P.row_map = d_rowmap;
        P.pixels = d_pixels;
        P.samples = (uint32_t*)B.samples.p;
        P.hits = B.hits.p;
        P.hits2 = (bounce_pipe || path || ao || pts) ? B.hits2.p : nullptr;
        P.pt_flags = (path || ao) ? (uint8_t*)B.pt_flags.p : nullptr;
        P.pt_index = (path || ao) ? (uint32_t*)B.pt_index.p : nullptr;
        P.pt_totals = (path || ao) ? (uint32_t*)B.pt_totals.p : nullptr;
        P.pt_carry = (path || ao) ? (uint32_t*)B.pt_carry.p : nullptr;
        P.ao_cache = (ao && !ao_uncached) ? (uint8_t*)s->d_ao_cache.p : nullptr;
        P.ao_claim = (ao && !ao_uncached) ? (unsigned long long*)s->d_ao_claim.p : nullptr;
        P.ao_escapes = ao ? (uint32_t*)B.ao_escapes.p : nullptr;
        P.lf_cache = lf ? (uint32_t*)(lft ? s->d_lft_cache.p : s->d_lf_cache.p) : nullptr;
        P.lf_claim = lf ? (uint32_t*)(lft ? s->d_lft_claim.p : s->d_lf_claim.p) : nullptr;
        P.lf_tris = lft;
        P.lf_handle = lft ? (const int32_t*)s->d_rhandle.p : nullptr;
        P.lf_trace_list = lft ? (uint32_t*)B.lf_stage.p : nullptr;
        P.lf_fused = lft && s->dbg[SR_DBG_KERNEL_SWITCH] != 43;       // (hook 43: the full traces as a compact list for k_lft_trace; same frame, measured slower)
        P.lf_points = lf ? (const double*)s->d_lf_points.p : nullptr;
        P.lf_res = lf ? s->lf_res : 0;
        P.lf_entries = lf ? (uint32_t)lf_entries(s->lf_res) : 0u;
        P.lf_cells = lf ? (uint32_t*)B.lf_cells.p : nullptr;
        P.lf_list = lf ? (uint32_t*)B.lf_list.p : nullptr;
        P.lf_shadows = lf && shadows;
        P.lf_stage = (lf && shadows) ? (uint32_t*)B.lf_stage.p : nullptr;
        P.lf_interp = lf_interp;
        P.lf_carry = lf_carry;
        P.lf_fracs = lf_carry ? (double*)B.lf_fracs.p : nullptr;
        if (bake) {
            P.lf_bake_first = bake->first; P.lf_bake_count = bake->count;
            P.lf_bake_pass_cells = (uint64_t)band_samples;
            P.lf_bake_filled = bake->filled;
            P.lf_bake_packet = s->dbg[SR_DBG_KERNEL_SWITCH] == 35;
        }
        if (pts) {
            P.pts_n = pts->n; P.pts_pass = pts_pass;
            P.pts_pos = pts->pos; P.pts_nrm = pts->nrm; P.pts_color = pts->color; P.pts_out = pts->out;
            P.pts_sort = pts_sort;
            P.pts_per_lane = s->dbg[SR_DBG_KERNEL_SWITCH] == 38;
            P.pts_escape = pts_escape;
            P.pts_static = pts->through_cache;
            P.pts_amount = pts->amount;
            P.pts_generators = pts->generators;
            for (int a = 0; a < 3; ++a) {                                 // (the box of the shortcut's diagonal: model and root box, + the probe offset, both ends)
                P.pts_escape_lo[a] = std::min(s->vmin[a], s->root.min[a]) - 0.002;
                P.pts_escape_hi[a] = std::max(s->vmax[a], s->root.max[a]) + 0.002;
            }
        }
        if (hreq) { P.hits_req = true; P.hits_out = hreq->out; }
        if (lfr) {
            P.lfr_n = lfr->n; P.lfr_pass = lfr_pass;
            P.lfr_starts = lfr->starts; P.lfr_dirs = lfr->dirs; P.lfr_out = lfr->out; P.lfr_inside = lfr->inside;
            P.lfr_filled = lfr->filled;
        }
        if (org) {
            P.org_n = org->n; P.org_pass = org_pass;
            P.org_dirs = org->dirs; P.hits_out = org->out;
            P.org_coherent = org->coherent;
            if (!org->with_extra) { P.sc.extra = nullptr; P.sc.nextra = 0; }    // the model alone, whatever the scene's extra geometry
        }
        s->ao_table_seed = f->random_seed;
        s->ao_table_rc = SR_OK;
        P.ao_table = !ao ? nullptr : [](void* user, unsigned long long generators) -> const int32_t* {
            sr_scene* sc = (sr_scene*)user;
            const unsigned long long limit = sc->dbg[SR_DBG_AO_TABLE_BYTES] > 0 ? (unsigned long long)sc->dbg[SR_DBG_AO_TABLE_BYTES] : (unsigned long long)kMaxPathTable;
            if (generators * 1200ull > limit) {
                sc->ao_table_rc = fail(SR_ERR_UNSUPPORTED, "ambient occlusion: the random table of the row block with the most generators (1200 bytes each) exceeds 256 MiB; raise concurrency or render row ranges");
                return nullptr;
            }
            if ((sc->ao_table_rc = ensure_draw_table(sc, sc->ao_table_seed, (size_t)generators * 100))) return nullptr;
            return (const int32_t*)sc->d_pt_table.p;
        };
        P.pt_table = path ? (const int32_t*)s->d_pt_table.p : nullptr;
        P.pt_block_height = pt_block_height;
        P.pt_blocks = pt_blocks;
        P.pt_phase = path ? pt_phase : 0;
        P.pt_reuse = pt_reuse;
        P.pt_row_hits = pt_phase ? (uint32_t*)s->d_pt_row_hits.p : nullptr;
        P.pt_row_k0 = pt_phase ? (uint32_t*)s->d_pt_row_k0.p : nullptr;
        P.pt_range_first = pt_range_first;
        P.pt_range_rows = pt_range_rows;
        P.ray_sort_buf = (bounce_pipe || path_walk || pts || org) ? (unsigned int*)B.ray_sort.p : nullptr;
        P.ray_sort_temp = (bounce_pipe || path_walk || pts || org) ? B.ray_sort_temp.p : nullptr;
        P.ray_sort_temp_bytes = (pts || org) ? sr::point_order_temp_bytes((unsigned)band_samples) : (bounce_pipe || path_walk) ? sr::ray_sort_temp_bytes((unsigned)band_samples) : 0;
        P.bounce_levels = bounce_pipe ? (uint32_t*)B.bounce_levels.p : nullptr;
        P.bounce_nlev = bounce_pipe ? (uint8_t*)B.bounce_nlev.p : nullptr;
        P.bounce_prep = (bounce_pipe || path_walk) ? B.bounce_prep.p : nullptr;
        P.bounce_res = (bounce_pipe || path_walk) ? B.bounce_res.p : nullptr;
        P.bounce_stack = (bounce_pipe || path_walk) ? (int32_t*)B.bounce_stack.p : nullptr;
        P.bounce_stack_bytes = (bounce_pipe || path_walk) ? B.bounce_stack.cap : 0;
        P.counters = (unsigned int*)B.counters.p;
        P.tile_cost = order_tiles ? (unsigned int*)B.tile_cost.p : nullptr;
        P.tile_order = order_tiles ? (unsigned int*)B.tile_order.p : nullptr;
        P.tile_order_tag = order_tiles ? &B.tile_order_tag : nullptr;
        for (int k = 0; k < 2; ++k) P.tile_hint[k] = order_tiles ? (unsigned int*)B.tile_hint[k].p : nullptr;
        P.tile_hint_cur = order_tiles ? &B.tile_hint_cur : nullptr;
        P.shaft_launches = &s->dbg_frame[1];
        P.static_hits = static_shadows ? s->d_static_hits.p : nullptr;
        P.static_claim = static_shadows ? (unsigned long long*)s->d_static_claim.p : nullptr;
        P.static_concurrency = f->concurrency;
        P.fallback = shaft ? (unsigned int*)B.fallback.p : nullptr;
        P.fallback_state = shaft ? B.fallback_state.p : nullptr;
        P.fallback_rays = shaft ? (unsigned int*)B.fallback_rays.p : nullptr;
        P.fallback_ray_cap = (unsigned int)fallback_ray_cap;
        P.fallback_overflow = shaft ? (unsigned int*)B.fallback_ovf.p : nullptr;
        for (int r = 0; r < sr::kShaftRounds; ++r) {
            P.round_items[r] = round_items[r];
            P.round_cap[r] = round_cap[r];
            P.round_list[r] = shaft ? (unsigned int*)B.rlist[r].p : nullptr;
            P.round_state[r] = (shaft && r > 0) ? B.rstate[r].p : nullptr;
            P.round_cand_count[r] = shaft ? (unsigned int*)B.rcount[r].p : nullptr;
            P.round_cand[r] = shaft ? (int32_t*)B.rcand[r].p : nullptr;
        }
        P.band_rows = (int32_t)band_rows;
        P.row_first = h * rows_half;
        P.row_limit = std::min(fc.num_rows, (h + 1) * rows_half);
        // workgroups per CU of the persistent shaft walk: two pipelines side by side leave each other room (a rank of an 8-way split: 1.41 -> 1.32 ms,
        // whole frame unchanged); a pipeline that has the chip to itself fills it (3.9 against 5.5 ms for the walk alone)
        P.shaft_wgs_per_cu = (split && !sequential_parts) ? 3 : 6;
        P.persistent_blocks = s->num_cus * 8;
        P.per_lane_shadows = (f->flags & SR_F_PER_LANE_SHADOWS) != 0;
        P.exact_shadow_tests = s->dbg[SR_DBG_EXACT_SHADOW_TESTS] > 0;
        P.per_lane_shaft = s->dbg[SR_DBG_PER_LANE_SHAFT] > 0 ? (int32_t)(s->dbg[SR_DBG_PER_LANE_SHAFT] & 3) : 0;
        P.per_lane_primary = s->dbg[SR_DBG_PER_LANE_PRIMARY] > 0 || org_far;
        P.bvh2_packets = s->dbg[SR_DBG_BVH2_PACKETS] > 0;
        P.shadows_on_bvh = shadows_on_bvh;
        P.primary_stats_only = (f->flags & SR_F_PRIMARY_STATS_ONLY) != 0;
        P.round2_node_budget = s->dbg[SR_DBG_ROUND2_NODES] >= 0 ? (int32_t)std::min<int64_t>(s->dbg[SR_DBG_ROUND2_NODES], 1 << 30) : 0;
        P.stats = (pt_phase == 1 && !pt_reuse) ? nullptr : d_stats;      // (a counting pass that phase 2 repeats: its rays are counted there)
        P.stream = bs;
        P.user = s;
        P.get_events = timing_events;
        P.band_done = nullptr;
        if (s->collect_bands) P.band_done = [](void* user, int band, int row_begin, int row_count, hipStream_t st) {
            sr_scene* sc = (sr_scene*)user;
            if (sc->band_ev_used == sc->band_ev_pool.size()) {
                hipEvent_t e = nullptr;
                if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { sc->collect_bands = false; return; }   // sr_render falls back to one copy
                sc->band_ev_pool.push_back(e);
            }
            hipEvent_t e = sc->band_ev_pool[sc->band_ev_used++];
            if (hipEventRecord(e, st) != hipSuccess) { sc->collect_bands = false; return; }
            sc->band_recs.push_back({e, band, row_begin, row_count});
        };
        if (accum_fresh) SR_HIP(hipMemsetAsync(B.accum.p, 0, B.accum.cap, bs));
        if (hints_fresh) for (DBuf& hb : B.tile_hint) SR_HIP(hipMemsetAsync(hb.p, 0xFF, hb.cap, bs));
        if (P.row_first < P.row_limit || bake || pts || org || lfr) {
            const hipError_t pe = sr::launch_pipeline(P);
            if (pe == hipErrorNotSupported && s->ao_table_rc) return s->ao_table_rc;      // (the message is the callback's)
            SR_HIP(pe);
        }
        if (split && !sequential_parts) {
            SR_HIP(hipEventRecord(B.done, bs));
            SR_HIP(hipStreamWaitEvent(stream, B.done, 0));          // the caller's stream continues after both halves
        }
    }
    return SR_OK;
}


// ------------------------------------------------------------------------------------------------------------------
// One scene over several devices of this process (sr_create_multi).  Rows are independent (the reference itself fans out row
// blocks, Renderer.cs:1659-1670): part g renders the 16-row strips s with s % n == g of the frame's row range into its own
// compact device buffer (sr_frame.strip_*), concurrently with the others (every part has its own device, streams and
// scratch; the calls below only ENQUEUE), and the strips travel straight to where the caller wants them: sr_render copies
// every part's strips device -> host into the caller's surface (each over its own PCIe link), sr_render_device copies them
// peer-to-peer (xGMI) into the caller's device surface.  No reduction, no RNG: the frame does not depend on the split.
// ------------------------------------------------------------------------------------------------------------------
const int kMultiStripRows = 16;

struct StripRun { int64_t compact_row, image_row, rows; };          // rows [image_row, image_row + rows) sit at compact_row of the part's buffer

// the runs of part g for the clamped row range [a, b]
std::vector<StripRun> strip_runs(int a, int b, int n, int g) {
    std::vector<StripRun> runs;
    int64_t compact = 0;
    for (int s0 = a / kMultiStripRows; s0 * kMultiStripRows <= b; ++s0) {
        if (s0 % n != g) continue;
        const int r0 = std::max(a, s0 * kMultiStripRows), r1 = std::min(b, s0 * kMultiStripRows + kMultiStripRows - 1);
        if (r1 < r0) continue;
        runs.push_back({compact, r0, r1 - r0 + 1});
        compact += r1 - r0 + 1;
    }
    return runs;
}

// copy the runs of one part to the full surface `dst` (host or device memory): the full strips between the (possibly
// partial) first and last one form an arithmetic progression -> ONE strided 2-D copy; the edges are copied on their own
// (src_strided: the source is laid out like the destination -- compact_row == image_row -- so its full strips are n strips apart too)
hipError_t copy_runs(const std::vector<StripRun>& runs, int n, int width, const uint32_t* src, uint32_t* dst, hipMemcpyKind kind, hipStream_t st, bool src_strided = false) {
    const size_t row_bytes = (size_t)width * 4;
    size_t i = 0;
    while (i < runs.size()) {
        size_t j = i;
        while (j + 1 < runs.size() && runs[j].rows == kMultiStripRows && runs[j + 1].rows == kMultiStripRows &&
               runs[j + 1].image_row - runs[j].image_row == (int64_t)n * kMultiStripRows) ++j;
        if (j > i) {
            const size_t strip_bytes = row_bytes * kMultiStripRows;
            hipError_t e = hipMemcpy2DAsync(dst + runs[i].image_row * width, strip_bytes * n, src + runs[i].compact_row * width, src_strided ? strip_bytes * n : strip_bytes,
                                            strip_bytes, j - i + 1, kind, st);
            if (e != hipSuccess) return e;
            i = j + 1;
        } else {
            hipError_t e = hipMemcpyAsync(dst + runs[i].image_row * width, src + runs[i].compact_row * width, row_bytes * runs[i].rows, kind, st);
            if (e != hipSuccess) return e;
            ++i;
        }
    }
    return hipSuccess;
}

// frames that cannot be split (one global fill order) are rendered whole by the first part
bool multi_splittable(const sr_frame* f) {
    return !((f->flags & SR_F_STATIC_SHADOWS) && (f->flags & SR_F_SHADOWS)) && !(f->flags & (SR_F_AMBIENT_OCCLUSION | SR_F_LIGHT_FIELD)) && f->strip_count <= 0;
}

// a part of a multi-device scene takes the first part's model by reference: counts, box and flags here, the arrays stay with `src`
// (sync_geometry uploads from them); nothing of the size of the model is copied on the host
void share_host_model(sr_scene* d, const sr_scene* src) {
    d->host_src = src;
    d->v9.clear(); d->argb.clear(); d->tri_recs.clear();
    d->host_model_stale = false;
    d->ntris = src->ntris;
    for (int a = 0; a < 3; ++a) { d->bmin[a] = src->bmin[a]; d->bmax[a] = src->bmax[a]; d->vmin[a] = src->vmin[a]; d->vmax[a] = src->vmax[a]; }
    d->have_model = src->have_model;
    d->root = src->root;
    d->shadow_cache_empty = true; d->shadow_cache_host.clear();
    d->ao_cache_empty = true; d->ao_cache_host.clear();
    d->lf_cache_empty = true; d->lf_cache_host.clear();
    d->lft_cache_empty = true; d->lft_cache_host.clear();
    d->vox_valid = false;
    d->ref = sr::RefTree(); d->bvh = sr::Bvh(); d->bvh_on_device = false;
    d->tris_dirty = d->ref_dirty = d->bvh_dirty = true;
    d->cam_valid = false; d->blight_valid = false; d->interior_valid = false;
    d->records_epoch++;
}
// ... and its host-built structures: the numbers a part needs (built / depth / counts), not the node arrays
void share_ref_tree(sr_scene* d, const sr_scene* src) {
    d->ref = sr::RefTree();
    d->ref.built = src->ref.built; d->ref.tree_depth = src->ref.tree_depth; d->ref.num_nodes = src->ref.num_nodes;
    d->ref.num_leaf_nodes = src->ref.num_leaf_nodes; d->ref.max_stack = src->ref.max_stack;
    d->ref_dirty = true;
}
void share_host_bvh(sr_scene* d, const sr_scene* src) {
    d->bvh = sr::Bvh();
    d->bvh.built = src->bvh.built; d->bvh.depth = src->bvh.depth;
    d->bvh_on_device = false;
    d->bvh_dirty = true;
}
// the scene has no own BVH (any more): what sr_set_triangles leaves, and what a refused sr_build leaves (include/softray.h sr_build).
// Nothing on the device describes a tree after this: no wide tree, no per-origin copies, no cone / interior / partition records
void drop_bvh(sr_scene* s) {
    s->bvh = sr::Bvh();
    s->bvh_on_device = false;
    s->bvh_num_nodes = 0;
    s->bvh_dirty = true;
    s->b4_num = 0; s->b4_depth = 0;
    s->b4_level_first.clear();
    s->bdepth_valid = false;
    s->b4cam_valid = s->b4light_valid = false;
    s->cam_valid = s->blight_valid = s->interior_valid = s->part_valid = false;
    s->records_epoch++;
}

// The host arrays of a model that sr_set_triangles_device left on the device only: vertices and records are read back (the colours
// come from the records).  Called by whatever reads s->v9 / s->argb / s->tri_recs -- the reference-tree build, the host's SAH build,
// sr_get_triangles; a scene that is only ever built on the device and rendered never gets here.  A part of a multi-device scene
// refills the part that holds the host arrays.
int ensure_host_model(sr_scene* s) {
    sr_scene* h = s->host_src ? const_cast<sr_scene*>(s->host_src) : s;
    if (!h->host_model_stale) return SR_OK;
    int rc = use_device(h);
    if (rc) return rc;
    const size_t n = h->ntris;
    h->v9.resize(9 * n);
    h->tri_recs.resize(n);
    h->argb.resize(n);
    if (n) {
        SR_HIP(hipMemcpy(h->v9.data(), h->d_v9.p, 9 * n * sizeof(double), hipMemcpyDeviceToHost));
        SR_HIP(hipMemcpy(h->tri_recs.data(), h->d_tris.p, n * sizeof(sr::Rec128), hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < n; ++i) h->argb[i] = h->tri_recs[i].color;
    h->host_model_stale = false;
    if (h != s && s->device >= 0) SR_HIP(hipSetDevice(s->device));
    return SR_OK;
}

// sr_set_triangles_device for one scene with a device.  src_*: arrays on device `src_device`; `copy_first`: they are copied to this
// scene's device before the kernels read them (a part of a multi-device scene other than the first; a peer copy also when the
// ordinals are equal).  `stream` belongs to this scene's device.
int set_triangles_from_device_enqueue(sr_scene* s, const double* src_v9, const uint32_t* src_argb, int64_t n, const double box_min[3],
                                      const double box_max[3], hipStream_t stream, int src_device, bool copy_first) {
    int rc = SR_OK;
    DBuf tmp_v9, tmp_argb;
    struct Free { DBuf* b[2]; ~Free() { for (DBuf* x : b) x->release(); } } free_tmp{{&tmp_v9, &tmp_argb}};
    if (copy_first && n > 0) {
        SR_HIP(tmp_v9.reserve((size_t)n * 9 * sizeof(double)));
        SR_HIP(hipMemcpyPeerAsync(tmp_v9.p, s->device, src_v9, src_device, (size_t)n * 9 * sizeof(double), stream));
        src_v9 = (const double*)tmp_v9.p;
        if (src_argb) {
            SR_HIP(tmp_argb.reserve((size_t)n * sizeof(uint32_t)));
            SR_HIP(hipMemcpyPeerAsync(tmp_argb.p, s->device, src_argb, src_device, (size_t)n * sizeof(uint32_t), stream));
            src_argb = (const uint32_t*)tmp_argb.p;
        }
    }
    double bounds[6];
    for (int a = 0; a < 3; ++a) { bounds[a] = box_min[a]; bounds[3 + a] = box_max[a]; }
    if (n > 0) {
        const size_t rec_bytes = (size_t)n * sizeof(sr::Rec128), v9_bytes = (size_t)n * 9 * sizeof(double);
        // a frame in flight keeps the old geometry: the kernels below run behind it (its event, waited for by the STREAM); only buffers
        // that have to grow are freed, and those the host waits for
        if (s->pre_used_set) {
            if (rec_bytes > s->d_tris.cap || v9_bytes > s->d_v9.cap) SR_HIP(hipEventSynchronize(s->pre_used));
            SR_HIP(hipStreamWaitEvent(stream, s->pre_used, 0));
        }
        SR_HIP(s->d_tris.reserve(rec_bytes));
        SR_HIP(s->d_v9.reserve(v9_bytes));
        SR_HIP(s->d_bounds.reserve(sr::tri_bounds_scratch_bytes()));
        hipEvent_t e0, e1;
        if ((rc = next_events(s, sr::K_TRI_RECORDS, e0, e1))) return rc;
        if (e0) SR_HIP(hipEventRecord(e0, stream));
        SR_HIP(sr::tri_records_device(src_v9, src_argb, (int)n, (double*)s->d_v9.p, (sr::Rec128*)s->d_tris.p, stream));
        if (e1) SR_HIP(hipEventRecord(e1, stream));
        if ((rc = next_events(s, sr::K_TRI_BOUNDS, e0, e1))) return rc;
        if (e0) SR_HIP(hipEventRecord(e0, stream));
        SR_HIP(sr::tri_bounds_device((const double*)s->d_v9.p, (int)n, box_min, box_max, (double*)s->d_bounds.p, stream));
        if (e1) SR_HIP(hipEventRecord(e1, stream));
        SR_HIP(hipMemcpyAsync(bounds, s->d_bounds.p, sizeof(bounds), hipMemcpyDeviceToHost, stream));
        SR_HIP(hipStreamSynchronize(stream));                          // the call's one host wait: the six doubles (and the temporaries are freed on return)
    }
    s->shadow_cache_empty = true; s->shadow_cache_host.clear();   // a new model: what sr_set_triangles drops
    s->ao_cache_empty = true; s->ao_cache_host.clear();
    s->lf_cache_empty = true; s->lf_cache_host.clear();
    s->lft_cache_empty = true; s->lft_cache_host.clear();
    s->vox_valid = false;
    std::vector<double>().swap(s->v9);
    std::vector<uint32_t>().swap(s->argb);
    std::vector<sr::Rec128>().swap(s->tri_recs);
    s->host_src = nullptr;
    s->host_model_stale = true;
    for (int a = 0; a < 3; ++a) { s->bmin[a] = box_min[a]; s->bmax[a] = box_max[a]; s->vmin[a] = bounds[a]; s->vmax[a] = bounds[3 + a]; }
    s->root = sr::make_root_box(box_min, box_max);
    s->ntris = (size_t)n;
    s->have_model = true;
    s->ref = sr::RefTree();
    s->ref_dirty = true;
    drop_bvh(s);
    s->tris_dirty = false;                                // the device arrays ARE the model: nothing to upload
    return SR_OK;
}

// the scene has no model (any more): what a device set that failed half way leaves -- its kernels may have overwritten or reallocated
// the device arrays while the host state still described the old model, which is gone either way
void drop_model(sr_scene* s) {
    std::vector<double>().swap(s->v9);
    std::vector<uint32_t>().swap(s->argb);
    std::vector<sr::Rec128>().swap(s->tri_recs);
    s->host_src = nullptr;
    s->host_model_stale = false;
    s->have_model = false;
    s->ntris = 0;
    s->ref = sr::RefTree();
    s->ref_dirty = true;
    drop_bvh(s);
    s->shadow_cache_empty = s->ao_cache_empty = s->lf_cache_empty = s->lft_cache_empty = true;
    s->vox_valid = false;
    s->tris_dirty = true;
}

int set_triangles_from_device(sr_scene* s, const double* src_v9, const uint32_t* src_argb, int64_t n, const double box_min[3],
                              const double box_max[3], hipStream_t stream, int src_device, bool copy_first) {
    int rc = use_device(s);                               // (a scene without a device is refused with nothing changed)
    if (rc) return rc;
    rc = set_triangles_from_device_enqueue(s, src_v9, src_argb, n, box_min, box_max, stream, src_device, copy_first);
    if (rc) {
        const std::string why = g_err;
        (void)hipStreamSynchronize(stream);               // nothing of the failed call is left running on the arrays
        (void)hipGetLastError();
        drop_model(s);
        g_err = why;
    }
    return rc;
}

// sr_refit_triangles_device for one scene with a device whose own BVH was built there (the caller has checked that).  Arguments as
// set_triangles_from_device_enqueue.  Nothing grows: the model keeps its count, so a frame in flight is only waited for by the STREAM.
int refit_from_device_enqueue(sr_scene* s, const double* src_v9, const uint32_t* src_argb, int64_t n, const double box_min[3],
                              const double box_max[3], hipStream_t stream, int src_device, bool copy_first) {
    int rc = SR_OK;
    DBuf tmp_v9, tmp_argb;
    struct Free { DBuf* b[2]; ~Free() { for (DBuf* x : b) x->release(); } } free_tmp{{&tmp_v9, &tmp_argb}};
    const size_t v9_bytes = (size_t)n * 9 * sizeof(double);
    if (copy_first) {
        SR_HIP(tmp_v9.reserve(v9_bytes));
        SR_HIP(hipMemcpyPeerAsync(tmp_v9.p, s->device, src_v9, src_device, v9_bytes, stream));
        src_v9 = (const double*)tmp_v9.p;
        if (src_argb) {
            SR_HIP(tmp_argb.reserve((size_t)n * sizeof(uint32_t)));
            SR_HIP(hipMemcpyPeerAsync(tmp_argb.p, s->device, src_argb, src_device, (size_t)n * sizeof(uint32_t), stream));
            src_argb = (const uint32_t*)tmp_argb.p;
        }
    }
    SR_HIP(s->d_bounds.reserve(sr::tri_bounds_scratch_bytes()));
    SR_HIP(s->d_tbox.reserve((size_t)n * sr::refit_box_bytes()));
    SR_HIP(s->d_bdepth.reserve(s->bvh_num_nodes));
    // a frame in flight keeps the old geometry and the old boxes: everything below runs behind it
    if (s->pre_used_set) SR_HIP(hipStreamWaitEvent(stream, s->pre_used, 0));
    double bounds[6];
    hipEvent_t e0, e1;
    if ((rc = next_events(s, sr::K_TRI_RECORDS, e0, e1))) return rc;
    if (e0) SR_HIP(hipEventRecord(e0, stream));
    SR_HIP(sr::tri_records_device(src_v9, src_argb, (int)n, (double*)s->d_v9.p, (sr::Rec128*)s->d_tris.p, stream));
    if (e1) SR_HIP(hipEventRecord(e1, stream));
    if ((rc = next_events(s, sr::K_TRI_BOUNDS, e0, e1))) return rc;
    if (e0) SR_HIP(hipEventRecord(e0, stream));
    SR_HIP(sr::tri_bounds_device((const double*)s->d_v9.p, (int)n, box_min, box_max, (double*)s->d_bounds.p, stream));
    if (e1) SR_HIP(hipEventRecord(e1, stream));
    SR_HIP(hipMemcpyAsync(bounds, s->d_bounds.p, sizeof(bounds), hipMemcpyDeviceToHost, stream));
    const sr::RootBox root = sr::make_root_box(box_min, box_max);
    struct Ev { sr_scene* s; int rc; } evu{s, SR_OK};
    SR_HIP(sr::refit_bvh_device((const double*)s->d_v9.p, (const sr::Rec128*)s->d_tris.p, (int)n, root, (sr::Rec128*)s->d_btris.p,
                                (sr::TriSlab*)s->d_bslab.p, (sr::BvhNode*)s->d_bnodes.p, (int)s->bvh_num_nodes, s->bvh.depth,
                                (sr::Bvh4Node*)s->d_b4.p, (int)s->b4_num, s->b4_level_first, s->d_tbox.p, (uint8_t*)s->d_bdepth.p,
                                &s->bdepth_valid, stream,
                                [](void* user, int phase, hipEvent_t* a, hipEvent_t* b) {
                                    hipEvent_t x = nullptr, y = nullptr;
                                    if (next_events(((Ev*)user)->s, phase == 0 ? sr::K_REFIT_LEAVES : sr::K_REFIT_NODES, x, y) != SR_OK) x = y = nullptr;
                                    *a = x; *b = y;
                                }, &evu));
    SR_HIP(hipStreamSynchronize(stream));                          // the call's one host wait: the six doubles (and the temporaries are freed on return)
    // ---- the geometry is new, the tree is the old one: everything made FROM the records or the boxes is stale ----
    s->b4cam_valid = s->b4light_valid = false;
    s->cam_valid = s->blight_valid = s->interior_valid = s->part_valid = false;
    s->records_epoch++;
    s->bvh_dirty = false;                                 // (kept: b4_num, b4_depth, bvh.built, bvh.depth, bvh_num_nodes, bvh_on_device)
    s->tris_dirty = false;
    s->shadow_cache_empty = true; s->shadow_cache_host.clear();   // a new model: what sr_set_triangles_device drops
    s->ao_cache_empty = true; s->ao_cache_host.clear();
    s->lf_cache_empty = true; s->lf_cache_host.clear();
    s->lft_cache_empty = true; s->lft_cache_host.clear();
    s->vox_valid = false;
    std::vector<double>().swap(s->v9);
    std::vector<uint32_t>().swap(s->argb);
    std::vector<sr::Rec128>().swap(s->tri_recs);
    s->host_src = nullptr;
    s->host_model_stale = true;
    for (int a = 0; a < 3; ++a) { s->bmin[a] = box_min[a]; s->bmax[a] = box_max[a]; s->vmin[a] = bounds[a]; s->vmax[a] = bounds[3 + a]; }
    s->root = root;
    s->ref = sr::RefTree();                               // SR_MODE_REF_TREE answers SR_ERR_NOT_BUILT until the next sr_build
    s->ref_dirty = true;
    return SR_OK;
}

int refit_from_device(sr_scene* s, const double* src_v9, const uint32_t* src_argb, int64_t n, const double box_min[3],
                      const double box_max[3], hipStream_t stream, int src_device, bool copy_first) {
    int rc = use_device(s);
    if (rc) return rc;
    rc = refit_from_device_enqueue(s, src_v9, src_argb, n, box_min, box_max, stream, src_device, copy_first);
    if (rc) {
        const std::string why = g_err;
        (void)hipStreamSynchronize(stream);               // nothing of the failed call is left running on the arrays
        (void)hipGetLastError();
        drop_model(s);
        g_err = why;
    }
    return rc;
}

// ------------------------------------------------------------------------------------------------------------------
// What the batch calls share: one stage of the renderer on data the caller supplies, as host arrays or as device arrays on a stream
// ------------------------------------------------------------------------------------------------------------------
// What a batch call that takes a frame refuses before the device is looked at, in the header's order: bad arguments; the switches that
// name no step of the call's stage, each with its sentence; (the point calls) mirror bounces and row strips; then whatever sr_render
// refuses of the frame the call runs, and of its trace mode
struct FlagRefusal { uint32_t flag; const char* why; };
struct BatchCall {
    const char* bad_argument;
    std::vector<FlagRefusal> flags;
    const char* bounces;          // max_bounces > 0 (nullptr: not read)
    const char* strips;           // strip_count > 0
    uint32_t implied;             // the switches the call's frame carries whatever the caller's says
    bool primary_only;            // sr_render_hits: the decorator switches and their parameters are not read
};

// `s`: in, the caller's scene; out, the scene that runs the call (the first part of a multi-device scene).  `args_ok`: the call's own test
// of its arguments.  `fs`: the frame the call runs
int batch_call_check(const BatchCall& c, sr_scene*& s, const sr_frame* f, bool args_ok, sr_frame& fs) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || !f || !args_ok) return fail(SR_ERR_INVALID_ARG, c.bad_argument);
    for (const FlagRefusal& r : c.flags)
        if (f->flags & r.flag) return fail(SR_ERR_UNSUPPORTED, r.why);
    if (c.bounces && f->max_bounces > 0) return fail(SR_ERR_UNSUPPORTED, c.bounces);
    if (f->strip_count > 0) return fail(SR_ERR_UNSUPPORTED, c.strips);
    fs = *f;
    fs.flags |= c.implied;
    if (c.primary_only) {
        fs.flags &= (uint32_t)(SR_F_FOCAL_BLUR | SR_F_NO_SPLIT | SR_F_PRIMARY_STATS_ONLY);
        fs.max_bounces = 0;
        fs.reflectivity = 0.0;
        fs.shadow_samples = 0;
        fs.area_light_offsets = nullptr;
    }
    int rc = validate_frame(&fs, s);
    if (rc) return rc;
    return check_frame_mode(s, &fs);
}

// One array of a host-array variant: `up` is copied to the device before the call, `down` is filled from there after it (both: the call
// works in place, as the device variant's `out` aliasing `color` does); the helper sets `dev`, nullptr where the caller passed neither
struct Staged { const void* up; void* down; size_t bytes; void* dev; };

// The host-array variant of a batch call around its device-array form: the arrays of `io` staged in the scene's d_io buffers, the
// statistics zeroed, `run(stream, d_stats)` -- the call's enqueue, on io_stream -- then the way back of the arrays and of last_stats (a
// multi-device parent `m` mirrors them; stats4: the caller's four primary counters, or nullptr) and one wait for the stream, which also
// follows a refusal of `run`.  upload_async: the uploads go on the stream instead of blocking the host one by one
template <class Run>
int run_staged(sr_scene* m, sr_scene* s, Staged* io, int count, bool upload_async, uint64_t* stats4, Run run) {
    int rc = ensure_io_streams(s);
    if (rc) return rc;
    hipStream_t stream = s->io_stream;
    for (int i = 0; i < count; ++i) {
        io[i].dev = nullptr;
        if (!io[i].up && !io[i].down) continue;
        SR_HIP(s->d_io[i].reserve(io[i].bytes));
        io[i].dev = s->d_io[i].p;
    }
    for (int i = 0; i < count; ++i) {
        if (!io[i].up) continue;
        if (upload_async) SR_HIP(hipMemcpyAsync(io[i].dev, io[i].up, io[i].bytes, hipMemcpyHostToDevice, stream));
        else SR_HIP(hipMemcpy(io[i].dev, io[i].up, io[i].bytes, hipMemcpyHostToDevice));
    }
    SR_HIP(s->d_stats.reserve(SR_STATS_COUNT * sizeof(uint64_t)));
    SR_HIP(hipMemsetAsync(s->d_stats.p, 0, SR_STATS_COUNT * sizeof(uint64_t), stream));
    if ((rc = run(stream, (unsigned long long*)s->d_stats.p))) { (void)hipStreamSynchronize(stream); return rc; }
    for (int i = 0; i < count; ++i)
        if (io[i].down) SR_HIP(hipMemcpyAsync(io[i].down, io[i].dev, io[i].bytes, hipMemcpyDeviceToHost, stream));
    SR_HIP(hipMemcpyAsync(s->last_stats, s->d_stats.p, SR_STATS_COUNT * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    SR_HIP(hipStreamSynchronize(stream));
    if (m != s) std::memcpy(m->last_stats, s->last_stats, sizeof(m->last_stats));
    if (stats4) std::memcpy(stats4, s->last_stats, 4 * sizeof(uint64_t));
    return SR_OK;
}

// ---- The batch calls without a frame (sr_occluded_rays, sr_nearest_rays, sr_all_hits_rays, sr_closest_points, sr_near_triangles, sr_overlap_triangles): one refusal ladder, one entry
// path for the host-array and the device-array variant, one setup of the passes
// What such a call refuses before the device is looked at, in the header's order.  Every sentence follows "<name>: "
struct ItemCall {
    const char* name;
    const char* null_args;        // a NULL array although n > 0
    bool        max_hits;         // max_hits is an argument (0 .. SR_HITS_MAX)
    uint32_t    options;          // the option bits the call knows
    const char* unknown_options;
    const char* voxels;           // SR_TARGET_VOXELS
    const char* root;             // SR_TARGET_ROOT (nullptr: the call takes the extra geometry)
    const char* ref_tree;         // SR_MODE_REF_TREE (nullptr: the call runs on the reference tree)
    uint32_t    counting;         // option bits that need max_hits == 0 (0: none)
    const char* counting_rows;    // ... one of them with max_hits > 0
};

// `s`: in, the caller's scene; out, the scene that runs the call (the first part of a multi-device scene).  `args_ok`: no array the call
// needs is NULL
int item_call_check(const ItemCall& c, sr_scene*& s, int32_t target, int64_t n, bool args_ok, int32_t max_hits, uint32_t options, int& mode,
                           bool& with_extra) {
    const auto refuse = [&](int code, const char* why) { return fail(code, std::string(c.name) + ": " + why); };
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s) return refuse(SR_ERR_INVALID_ARG, "the scene is NULL");
    if (n < 0) return refuse(SR_ERR_INVALID_ARG, "n is negative");
    if (n > 0 && !args_ok) return refuse(SR_ERR_INVALID_ARG, c.null_args);
    if (c.max_hits && (max_hits < 0 || max_hits > SR_HITS_MAX)) return refuse(SR_ERR_INVALID_ARG, "max_hits must be 0 .. SR_HITS_MAX (64)");
    if (options & ~c.options) return refuse(SR_ERR_INVALID_ARG, c.unknown_options);
    if ((options & c.counting) && max_hits > 0) return refuse(SR_ERR_INVALID_ARG, c.counting_rows);
    if (target & SR_TARGET_VOXELS) return refuse(SR_ERR_UNSUPPORTED, c.voxels);
    if (c.root && (target & SR_TARGET_ROOT)) return refuse(SR_ERR_UNSUPPORTED, c.root);
    with_extra = (target & SR_TARGET_ROOT) != 0;
    mode = target & 0xff;
    if (c.ref_tree && mode == SR_MODE_REF_TREE) return refuse(SR_ERR_UNSUPPORTED, c.ref_tree);
    if (!s->have_model) return refuse(SR_ERR_NO_MODEL, "the scene has no model (sr_set_triangles, sr_load_3ds)");
    int rc;
    if (s->ntris == 0 && mode == SR_MODE_BRUTE) { /* an empty model is fine for brute force, as in sr_trace_rays */ }
    else if ((rc = check_mode(s, mode))) return rc;
    if (s->device < 0) return refuse(SR_ERR_NO_DEVICE, "a host-only scene has no HIP device to walk on (compute is never emulated on the CPU)");
    return SR_OK;
}

// Where a call's arrays are.  The host-array variant: `io`, staged by run_staged, and the caller's four counters; the device-array variant
// (io == nullptr): the caller's stream and statistics words, which are zeroed first
struct ItemIo { Staged* io; int count; uint64_t* stats4; void* hip_stream; uint64_t* d_stats; };

// An entry point: the refusals, the empty batch, the device, then run(s, mode, with_extra, stream, d_stats) -- the call's enqueue
template <class Run>
int item_call(const ItemCall& c, sr_scene* m, int32_t target, int64_t n, bool args_ok, int32_t max_hits, uint32_t options, const ItemIo& io, Run run) {
    sr_scene* s = m;
    int mode = 0; bool with_extra = false;
    int rc = item_call_check(c, s, target, n, args_ok, max_hits, options, mode, with_extra);
    if (rc || n == 0) return rc;
    if ((rc = use_device(s))) return rc;
    if (io.io)
        return run_staged(m, s, io.io, io.count, true, io.stats4,
                          [&](hipStream_t stream, unsigned long long* d_stats) { return run(s, mode, with_extra, stream, d_stats); });
    hipStream_t stream = (hipStream_t)io.hip_stream;
    if (io.d_stats) SR_HIP(hipMemsetAsync(io.d_stats, 0, SR_STATS_COUNT * sizeof(uint64_t), stream));
    return run(s, mode, with_extra, stream, (unsigned long long*)io.d_stats);
}

// What the passes of such a call need before their launch, enqueued on `stream`: the geometry on the device; the call ordered like a frame
// (render_common: a frame's facing partition moves the records the walk reads) -- `order` must live until the launch is enqueued; the pass
// size, at most max_pass; `slots`, the pass rounded up to 256; (ordered: the call sorts its passes) the first scratch set's sort buffers; and
// the launch fields every call has.  L.limits and L.input_order are the caller's to set
int item_call_setup(sr_scene* s, int mode, int64_t n, int64_t max_pass, bool ordered, hipStream_t stream, unsigned long long* d_stats,
                           std::unique_ptr<StreamOrder>& order, sr::BatchLaunch& L, size_t& slots) {
    int rc = sync_geometry(s, (uint32_t)mode);
    if (rc) return rc;
    order.reset(new StreamOrder(s, stream));
    if (order->entered) return order->entered;
    if (s->pre_ready_set) SR_HIP(hipStreamWaitEvent(stream, s->pre_ready, 0));      // the records' order, written on another stream perhaps
    const int64_t want = s->dbg[SR_DBG_BAND_SAMPLES] > 0 ? std::min<int64_t>(s->dbg[SR_DBG_BAND_SAMPLES], max_pass) : max_pass;
    L.n = n;
    L.pass = std::max<int64_t>(1, std::min<int64_t>(want, n));
    slots = (size_t)(L.pass + 255) / 256 * 256;
    if (ordered) {
        sr_scene::BandScratch& B = s->scratch[0];
        L.sort_temp_bytes = sr::point_order_temp_bytes((unsigned)slots);
        SR_HIP(B.ray_sort.reserve((4 * slots + 64) * sizeof(unsigned int)));
        SR_HIP(B.ray_sort_temp.reserve(L.sort_temp_bytes));
        L.sort_buf = (unsigned int*)B.ray_sort.p;
        L.sort_temp = B.ray_sort_temp.p;
    }
    L.stats = d_stats;
    L.stream = stream;
    L.user = s;
    L.get_events = timing_events;
    return SR_OK;
}

// An empty batch of a device variant that reports generators: the count is zeroed on the caller's stream, and no device is asked for
int zero_generators_device(const sr_scene* s, uint64_t* d_generators, hipStream_t stream) {
    if (d_generators && s->device >= 0) {
        SR_HIP(hipSetDevice(s->device));
        SR_HIP(hipMemsetAsync(d_generators, 0, sizeof(uint64_t), stream));
    }
    return SR_OK;
}

}  // namespace

extern "C" {

int32_t sr_abi_version(void) { return SR_ABI_VERSION; }
const char* sr_last_error(void) { return g_err.c_str(); }

int sr_create(int32_t device, sr_scene** out) {
    if (!out) return fail(SR_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (device >= 0) {
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess || count <= 0) return fail(SR_ERR_NO_DEVICE, "no HIP device available (libsoftray_hip has no CPU fallback)");
        if (device >= count) return fail(SR_ERR_INVALID_ARG, "device ordinal out of range");
        SR_HIP(hipSetDevice(device));
    } else if (device != -1) {
        return fail(SR_ERR_INVALID_ARG, "device must be >= 0, or -1 for a host-only scene");
    }
    sr_scene* s = new sr_scene();
    s->device = device;
    *out = s;
    return SR_OK;
}

int sr_create_multi(const int32_t* devices, int32_t n, sr_scene** out) {
    if (!out) return fail(SR_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!devices || n < 1 || n > 64) return fail(SR_ERR_INVALID_ARG, "sr_create_multi needs 1..64 device ordinals");
    sr_scene* m = new sr_scene();
    m->device = -2;
    for (int i = 0; i < n; ++i) {
        sr_scene* part = nullptr;
        int rc = devices[i] >= 0 ? sr_create(devices[i], &part) : fail(SR_ERR_INVALID_ARG, "device ordinals must be >= 0");
        if (rc) { for (sr_scene* q : m->parts) sr_destroy(q); delete m; return rc; }
        m->parts.push_back(part);
    }
    // sr_render_device gathers the strips into a surface on the first part's device: peer-to-peer where that device can read the
    // part's memory (asked and enabled here, the answer kept per part), through pinned host staging where it cannot
    for (int i = 1; i < n; ++i) {
        sr_scene* q = m->parts[i];
        if (devices[i] == devices[0]) { q->can_peer = true; continue; }
        int can = 0;
        q->can_peer = false;
        if (hipDeviceCanAccessPeer(&can, devices[0], devices[i]) != hipSuccess) { (void)hipGetLastError(); continue; }
        if (!can) continue;
        hipError_t e = hipSetDevice(devices[0]);
        if (e == hipSuccess) e = hipDeviceEnablePeerAccess(devices[i], 0);
        if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) { q->can_peer = true; (void)hipGetLastError(); continue; }
        // the runtime said the devices can be peers and then refused: report it instead of running with half a configuration
        for (sr_scene* p : m->parts) sr_destroy(p);
        delete m;
        return hip_fail(e, "hipDeviceEnablePeerAccess");
    }
    *out = m;
    return SR_OK;
}

int32_t sr_device_count(const sr_scene* s) { return !s ? 0 : (s->parts.empty() ? (s->device >= 0 ? 1 : 0) : (int32_t)s->parts.size()); }
int32_t sr_last_frame_parts(const sr_scene* s) { return !s ? 0 : (s->parts.empty() ? 1 : s->last_parts); }

void sr_destroy(sr_scene* s) {
    if (!s) return;
    if (!s->parts.empty()) {
        if (!s->comms.empty()) {
            const sr::RcclApi* api = sr::rccl_api(nullptr);
            for (size_t g = 0; api && g < s->comms.size(); ++g)
                if (s->comms[g] && use_device(s->parts[g]) == SR_OK) (void)api->CommDestroy(s->comms[g]);
        }
        if (s->multi_done && use_device(s->parts[0]) == SR_OK) (void)hipEventDestroy(s->multi_done);
        if (use_device(s->parts[0]) == SR_OK) s->d_gather.release();
        for (sr_scene* q : s->parts) sr_destroy(q);                 // (frees device memory: whatever still read the pinned counts has run)
        if (s->pt_counts_host) (void)hipHostFree(s->pt_counts_host);
        delete s;
        return;
    }
    if (s->device >= 0 && hipSetDevice(s->device) == hipSuccess) {
        DBuf* bufs[] = {&s->d_tris, &s->d_extra, &s->d_rnodes, &s->d_rboxes, &s->d_rleaf, &s->d_bnodes, &s->d_btris, &s->d_bslab, &s->d_binter,
                        &s->d_v9, &s->d_bcam, &s->d_blight, &s->d_b4, &s->d_b4cam, &s->d_b4light, &s->d_rng_cam, &s->d_rng_light, &s->d_shadow_cache, &s->d_static_claim, &s->d_static_hits, &s->d_ao_cache, &s->d_ao_claim, &s->d_aop_table, &s->d_aop_rows, &s->d_aop_state, &s->d_pp_state, &s->d_lf_cache, &s->d_lf_claim, &s->d_lf_points, &s->d_lft_cache, &s->d_lft_claim, &s->d_rhandle, &s->d_pt_table, &s->d_pt_row_hits, &s->d_pt_row_k0, &s->d_pixels, &s->d_aa, &s->d_stats,
                        &s->d_vox_colors, &s->d_vox_normals, &s->d_vox_mask, &s->d_vox_bricks, &s->d_vox_coarse, &s->d_bounds, &s->d_bdepth, &s->d_tbox};
        for (DBuf* b : bufs) b->release();
        for (auto& sc : s->scratch) sc.release();
        for (auto& t : s->tables) { t.dev.release(); if (t.host) (void)hipHostFree(t.host); if (t.used) (void)hipEventDestroy(t.used); if (t.ready) (void)hipEventDestroy(t.ready); }
        if (s->fork) (void)hipEventDestroy(s->fork);
        if (s->io_stream) (void)hipStreamDestroy(s->io_stream);
        if (s->copy_stream) (void)hipStreamDestroy(s->copy_stream);
        for (hipEvent_t e : s->band_ev_pool) (void)hipEventDestroy(e);
        if (s->stage_host) (void)hipHostFree(s->stage_host);
        if (s->staged) (void)hipEventDestroy(s->staged);
        if (s->pre_ready) (void)hipEventDestroy(s->pre_ready);
        if (s->pre_used) (void)hipEventDestroy(s->pre_used);
        if (s->multi_done) (void)hipEventDestroy(s->multi_done);
        if (s->pt_counted) (void)hipEventDestroy(s->pt_counted);
        for (DBuf& b : s->d_io) b.release();
        s->d_gather.release();
        if (s->comm) { const sr::RcclApi* api = sr::rccl_api(nullptr); if (api) (void)api->CommDestroy(s->comm); s->comm = nullptr; }
        for (int k = 0; k < sr::K_COUNT; ++k)
            for (hipEvent_t e : s->ev[k]) (void)hipEventDestroy(e);
    }
    delete s;
}

int sr_set_triangles(sr_scene* s, const double* v9, const uint32_t* argb, int64_t n, const double box_min[3], const double box_max[3]) {
    if (s && !s->parts.empty()) {                                  // host work once, the records are replicated
        int rc = sr_set_triangles(s->parts[0], v9, argb, n, box_min, box_max);
        for (size_t i = 1; i < s->parts.size() && !rc; ++i) share_host_model(s->parts[i], s->parts[0]);
        return rc;
    }
    if (!s || n < 0 || (n > 0 && (!v9 || !argb)) || !box_min || !box_max) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_set_triangles");
    if (n > 0x7fffff00) return fail(SR_ERR_INVALID_ARG, "too many triangles");
    s->shadow_cache_empty = true; s->shadow_cache_host.clear();   // new model: what a new ShadowMethod starts with
    s->ao_cache_empty = true; s->ao_cache_host.clear();   // ... and a new AmbientOcclusion
    s->lf_cache_empty = true; s->lf_cache_host.clear();   // ... and a new LightFieldColorMethod
    s->lft_cache_empty = true; s->lft_cache_host.clear(); // ... and a new LightFieldTriMethod
    s->vox_valid = false;                                 // ... and a new VoxelGrid
    s->host_model_stale = false;
    s->v9.assign(v9, v9 + 9 * n);
    s->argb.assign(argb, argb + n);
    for (int a = 0; a < 3; ++a) { s->bmin[a] = box_min[a]; s->bmax[a] = box_max[a]; }
    s->root = sr::make_root_box(box_min, box_max);
    for (int a = 0; a < 3; ++a) { s->vmin[a] = box_min[a]; s->vmax[a] = box_max[a]; }
    for (int64_t i = 0; i < 3 * n; ++i)
        for (int a = 0; a < 3; ++a) { s->vmin[a] = std::min(s->vmin[a], v9[3 * i + a]); s->vmax[a] = std::max(s->vmax[a], v9[3 * i + a]); }
    s->ntris = (size_t)n;
    s->tri_recs.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const double* p = &s->v9[9 * i];
        s->tri_recs[i] = sr::make_triangle_record({p[0], p[1], p[2]}, {p[3], p[4], p[5]}, {p[6], p[7], p[8]}, argb[i], (int32_t)i);
    }
    s->have_model = true;
    s->ref = sr::RefTree();
    s->bvh = sr::Bvh();
    s->bvh_on_device = false;
    s->tris_dirty = s->ref_dirty = s->bvh_dirty = true;
    return SR_OK;
}

int sr_set_triangles_device(sr_scene* s, const double* d_v9, const uint32_t* d_argb, int64_t n, const double box_min[3], const double box_max[3],
                            void* hip_stream) {
    if (!s || n < 0 || (n > 0 && !d_v9) || !box_min || !box_max) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_set_triangles_device");
    if (n > 0x7fffff00) return fail(SR_ERR_INVALID_ARG, "too many triangles");
    sr_scene* first = s->parts.empty() ? s : s->parts[0];
    if (n > 0 && !d_argb && (!first->have_model || (int64_t)first->ntris != n))      // (n == 0 needs no array, as in sr_set_triangles)
        return fail(SR_ERR_INVALID_ARG, "sr_set_triangles_device without colours needs a model of the same number of triangles");
    // keep-colours reads the colours out of the device records: a model that sr_set_triangles / sr_load_3ds left on the host only (the
    // upload waits for the next sr_build or frame) is uploaded first -- by every part, before the first part's host arrays are dropped
    if (!d_argb && n > 0) {
        std::vector<sr_scene*> one{s};
        for (sr_scene* q : s->parts.empty() ? one : s->parts) {
            if (!q->tris_dirty) continue;
            int rc = use_device(q);
            if (rc) return rc;
            if (q->pre_used_set) SR_HIP(hipEventSynchronize(q->pre_used));   // (the upload may free the arrays a frame in flight reads)
            if ((rc = sync_geometry(q, SR_MODE_BRUTE))) return rc;
        }
    }
    if (s->parts.empty()) return set_triangles_from_device(s, d_v9, d_argb, n, box_min, box_max, (hipStream_t)hip_stream, s->device, false);
    // the arrays live on the first part's device: it takes them on the caller's stream (and waits for it: they are complete then);
    // every other part copies them to its own device and makes its own records
    int rc = set_triangles_from_device(first, d_v9, d_argb, n, box_min, box_max, (hipStream_t)hip_stream, first->device, false);
    for (size_t i = 1; i < s->parts.size() && !rc; ++i) {
        rc = set_triangles_from_device(s->parts[i], d_v9, d_argb, n, box_min, box_max, nullptr, first->device, true);
        if (!rc) s->parts[i]->host_src = first;                  // the host arrays, once something asks for them, live with the first part
    }
    if (rc) {                                                    // no part keeps a model the others do not have
        const std::string why = g_err;
        for (sr_scene* q : s->parts) drop_model(q);
        g_err = why;
    }
    return rc;
}

int sr_refit_triangles_device(sr_scene* s, const double* d_v9, const uint32_t* d_argb, int64_t n, const double box_min[3], const double box_max[3],
                              void* hip_stream) {
    if (!s || n < 0 || (n > 0 && !d_v9) || !box_min || !box_max) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_refit_triangles_device");
    if (n > 0x7fffff00) return fail(SR_ERR_INVALID_ARG, "too many triangles");
    if (s->parts.empty() && s->device < 0) return fail(SR_ERR_NO_DEVICE, "host-only scene: no HIP device bound (compute is never emulated on the CPU)");
    std::vector<sr_scene*> one{s};
    const std::vector<sr_scene*>& parts = s->parts.empty() ? one : s->parts;
    sr_scene* first = parts[0];
    // ---- every refusal before anything is enqueued: the scene stays as it is ----
    if ((int64_t)first->ntris != n) return fail(SR_ERR_INVALID_ARG, "sr_refit_triangles_device: n differs from the model's triangle count (a refit keeps the topology)");
    if (!first->have_model || n == 0) return fail(SR_ERR_NO_MODEL, "sr_refit_triangles_device before sr_set_triangles");
    for (const sr_scene* q : parts)
        if (!q->bvh.built || (q->bvh_on_device && (q->bvh_num_nodes == 0 || q->b4_num == 0 || q->d_btris.cap < (size_t)n * sizeof(sr::Rec128))))
            return fail(SR_ERR_NOT_BUILT, "sr_refit_triangles_device: the scene has no own BVH (sr_build(1 << SR_MODE_BVH) first)");
    for (const sr_scene* q : parts)
        if (!q->bvh_on_device || q->bvh_dirty || q->tris_dirty || q->b4_level_first.size() < 2)
            return fail(SR_ERR_UNSUPPORTED, "sr_refit_triangles_device: the own BVH was built on the host (SR_BUILD_ON_HOST, or n <= 64): rebuild instead");
    if (parts.size() == 1) return refit_from_device(first, d_v9, d_argb, n, box_min, box_max, (hipStream_t)hip_stream, first->device, false);
    // as in sr_set_triangles_device: the first part takes the arrays on the caller's stream (and waits for it), every other part copies
    // them to its own device and refits its own tree
    int rc = refit_from_device(first, d_v9, d_argb, n, box_min, box_max, (hipStream_t)hip_stream, first->device, false);
    for (size_t i = 1; i < parts.size() && !rc; ++i) {
        rc = refit_from_device(parts[i], d_v9, d_argb, n, box_min, box_max, nullptr, first->device, true);
        if (!rc) parts[i]->host_src = first;
    }
    if (rc) {                                                    // no part keeps a model the others do not have
        const std::string why = g_err;
        for (sr_scene* q : parts) drop_model(q);
        g_err = why;
    }
    return rc;
}

int sr_set_extra_geometry(sr_scene* s, const sr_prim* prims, int32_t n) {
    if (s && !s->parts.empty()) {
        for (sr_scene* q : s->parts) { int rc = sr_set_extra_geometry(q, prims, n); if (rc) return rc; }
        return SR_OK;
    }
    if (!s || n < 0 || (n > 0 && !prims)) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_set_extra_geometry");
    std::vector<sr::Rec128> recs;
    for (int i = 0; i < n; ++i) {
        const sr_prim& q = prims[i];
        switch (q.kind) {
            case 0:
                if (!(q.p[3] > 0)) return fail(SR_ERR_INVALID_ARG, "sphere radius must be > 0 (Sphere.cs:28)");
                recs.push_back(sr::make_sphere_record({q.p[0], q.p[1], q.p[2]}, q.p[3], q.argb));
                break;
            case 1: recs.push_back(sr::make_plane_record({q.p[0], q.p[1], q.p[2]}, {q.p[3], q.p[4], q.p[5]}, q.argb)); break;
            case 3: {                                              // an existing Plane object: its stored unit normal and originDist, verbatim
                sr::Rec128 r;
                std::memset(&r, 0, sizeof(r));
                r.p[0] = q.p[0]; r.p[1] = q.p[1]; r.p[2] = q.p[2]; r.p[3] = q.p[3];
                r.color = q.argb; r.aux = 1;
                recs.push_back(r);
                break;
            }
            case 2: {
                sr::Rec128 r = sr::make_triangle_record({q.p[0], q.p[1], q.p[2]}, {q.p[3], q.p[4], q.p[5]}, {q.p[6], q.p[7], q.p[8]}, q.argb, 2);
                recs.push_back(r);
                break;
            }
            case 4:                                                // AxisAlignedBox(min, max), AxisAlignedBox.cs:15-28
                if (!(q.p[0] < q.p[3] && q.p[1] < q.p[4] && q.p[2] < q.p[5])) return fail(SR_ERR_INVALID_ARG, "Axis aligned bounding box has bad coordinates (AxisAlignedBox.cs:17-19)");
                recs.push_back(sr::make_box_record({q.p[0], q.p[1], q.p[2]}, {q.p[3], q.p[4], q.p[5]}));
                break;
            default: return fail(SR_ERR_INVALID_ARG, "unknown primitive kind");
        }
    }
    s->extra_recs.swap(recs);
    s->extra_dirty = true;
    return SR_OK;
}

int sr_build(sr_scene* s, uint32_t modes, int32_t max_depth, int32_t max_per_leaf) {
    if (s && !s->parts.empty()) {
        // the host structures (reference tree, SAH BVH) are built once and copied; a device-built BVH is built by every part
        int rc = sr_build(s->parts[0], modes, max_depth, max_per_leaf);
        for (size_t i = 1; i < s->parts.size() && !rc; ++i) {
            sr_scene* q = s->parts[i];
            if (!(modes & SR_BUILD_ON_HOST) && (modes & (1u << SR_MODE_BVH)) && s->parts[0]->bvh_on_device) {
                share_ref_tree(q, s->parts[0]);
                rc = sr_build(q, modes & ~(1u << SR_MODE_REF_TREE), max_depth, max_per_leaf);
                if (!rc && (modes & (1u << SR_MODE_REF_TREE)) && (rc = use_device(q)) == SR_OK) rc = sync_geometry(q, SR_MODE_REF_TREE);
                continue;
            }
            if (modes & (1u << SR_MODE_REF_TREE)) share_ref_tree(q, s->parts[0]);
            if (modes & (1u << SR_MODE_BVH)) share_host_bvh(q, s->parts[0]);
            if ((rc = use_device(q))) break;
            if (modes & (1u << SR_MODE_REF_TREE)) if ((rc = sync_geometry(q, SR_MODE_REF_TREE))) break;
            if (modes & (1u << SR_MODE_BVH)) if ((rc = sync_geometry(q, SR_MODE_BVH))) break;
            rc = sync_geometry(q, SR_MODE_BRUTE);
        }
        if (rc && (modes & (1u << SR_MODE_BVH))) {
            // a part that refused the own BVH has none left: no part keeps the tree of an earlier build (the parts render one frame together)
            bool refused = false;
            for (sr_scene* q : s->parts) refused = refused || !q->bvh.built;
            if (refused) for (sr_scene* q : s->parts) drop_bvh(q);
            // ... and the reference tree that the first part built in the same call stands, as in a scene of one device
            if (refused && rc == SR_ERR_UNSUPPORTED && (modes & (1u << SR_MODE_REF_TREE)) && s->parts[0]->ref.built)
                for (size_t i = 1; i < s->parts.size(); ++i) share_ref_tree(s->parts[i], s->parts[0]);
        }
        return rc;
    }
    if (!s) return fail(SR_ERR_INVALID_ARG, "scene is NULL");
    if (!s->have_model) return fail(SR_ERR_NO_MODEL, "sr_build before sr_set_triangles");
    // leaves are packed as (first record | count << 27) and traversal stack words as (node | bound << bits): 2^28 records / 2^26 nodes
    if ((modes & (1u << SR_MODE_BVH)) && s->ntris >= (1u << 26))
        return fail(SR_ERR_UNSUPPORTED, "the library's BVH holds at most 2^26 - 1 triangles");
    const bool on_device = s->device >= 0 && !(modes & SR_BUILD_ON_HOST) && s->ntris > 64;
    // the reference tree and the SAH tree are built by the host from the host arrays: a model set from device memory is read back first
    if ((modes & (1u << SR_MODE_REF_TREE)) || ((modes & (1u << SR_MODE_BVH)) && !on_device)) {
        int rc = ensure_host_model(s);
        if (rc) return rc;
    }
    if (modes & (1u << SR_MODE_REF_TREE)) {
        int md = max_depth > 0 ? max_depth : 15, mg = max_per_leaf > 0 ? max_per_leaf : 25;   // SpatialSubdivision.cs:269-270
        if (!sr::build_ref_tree(s->v9, s->bmin, s->bmax, md, mg, s->ref))
            return fail(SR_ERR_OUT_OF_RANGE, "A triangle vertex is outside the bounding box");
        s->ref_dirty = true;
    }
    // the own BVH is built where the triangles are: on the device (LBVH, sr_lbvh.hip), unless the scene has none, is tiny, or the
    // caller asks for the host's binned-SAH builder (SR_BUILD_ON_HOST)
    if ((modes & SR_BUILD_ON_DEVICE) && s->device < 0) return fail(SR_ERR_NO_DEVICE, "SR_BUILD_ON_DEVICE needs a HIP device");
    if ((modes & (1u << SR_MODE_BVH)) && on_device) {
        // ---- LBVH built by the GPU (sr_lbvh.hip) ----
        int rc = use_device(s);
        if (rc) return rc;
        if ((rc = sync_geometry(s, SR_MODE_BRUTE))) return rc;            // d_tris
        const size_t n = s->ntris;
        DBuf d_slab;
        DBuf& d_v9 = s->d_v9;                                             // uploaded by sync_geometry with the records
        SR_HIP(d_slab.reserve(n * sizeof(sr::TriSlab)));
        SR_HIP(sr::make_slabs_device((const double*)d_v9.p, (int)n, s->root, (sr::TriSlab*)d_slab.p, nullptr));   // (the host loop + upload cost 0.4 s at 10 M)
        SR_HIP(s->d_bnodes.reserve(n * sizeof(sr::BvhNode)));
        SR_HIP(s->d_btris.reserve(n * sizeof(sr::Rec128)));
        SR_HIP(s->d_bslab.reserve(n * sizeof(sr::TriSlab)));
        int nn = 0, depth = 0;
        if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));          // a frame in flight may still be walking the old tree
        drop_bvh(s);                                                          // the build overwrites the old tree's buffers: from here on the scene has no tree until this one is accepted
        hipError_t e = sr::build_bvh_device((const double*)d_v9.p, (int)n, s->root, (const sr::Rec128*)s->d_tris.p, (const sr::TriSlab*)d_slab.p,
                                            (sr::BvhNode*)s->d_bnodes.p, (sr::Rec128*)s->d_btris.p, (sr::TriSlab*)s->d_bslab.p, &nn, &depth, nullptr,
                                            s->dbg[SR_DBG_BVH_LEAF] > 0 ? (int)std::min<int64_t>(15, s->dbg[SR_DBG_BVH_LEAF]) : 0);
        d_slab.release();
        if (e != hipSuccess) return hip_fail(e, "build_bvh_device");
        if (depth > kMaxTreeDepth) return fail(SR_ERR_UNSUPPORTED, "BVH deeper than 62 levels does not fit the LDS traversal stacks");
        s->bvh = sr::Bvh();
        s->bvh.built = true;
        s->bvh.depth = depth;
        s->bvh_num_nodes = (size_t)nn;
        s->bvh_on_device = true;
        s->bvh_dirty = false;
        {   // the four-wide tree of the packet walks, collapsed where the binary nodes are
            SR_HIP(s->d_b4.reserve((size_t)nn * sizeof(sr::Bvh4Node)));
            int n4 = 0, d4 = 0;
            e = sr::collapse_bvh4_device((const sr::BvhNode*)s->d_bnodes.p, nn, (sr::Bvh4Node*)s->d_b4.p, &n4, &d4, nullptr, &s->b4_level_first);
            if (e != hipSuccess) { drop_bvh(s); return hip_fail(e, "collapse_bvh4_device"); }
            s->b4_num = (size_t)n4;
            s->b4_depth = d4;
            SR_HIP(s->d_b4cam.reserve((size_t)n4 * sizeof(sr::Bvh4Node)));
            SR_HIP(s->d_b4light.reserve((size_t)n4 * sizeof(sr::Bvh4Node)));
        }
    } else if (modes & (1u << SR_MODE_BVH)) {
        sr::Bvh built;                                                         // moved into the scene only once it is accepted
        sr::build_bvh(s->v9, s->root, built, s->dbg[SR_DBG_BVH_LEAF] > 0 ? (int)std::min<int64_t>(15, s->dbg[SR_DBG_BVH_LEAF]) : 4,
                      s->dbg[SR_DBG_BUILD_THREADS] > 0 ? (int)std::min<int64_t>(64, s->dbg[SR_DBG_BUILD_THREADS]) : 0);
        drop_bvh(s);                                                           // (an earlier tree, host- or device-built, goes either way)
        if (built.depth > kMaxTreeDepth) return fail(SR_ERR_UNSUPPORTED, "BVH deeper than 62 levels does not fit the LDS traversal stacks");
        s->bvh = std::move(built);
    }
    if (s->device >= 0) {
        int rc = use_device(s);
        if (rc) return rc;
        if (modes & (1u << SR_MODE_REF_TREE)) if ((rc = sync_geometry(s, SR_MODE_REF_TREE))) return rc;
        if ((modes & (1u << SR_MODE_BVH)) && !s->bvh_on_device) if ((rc = sync_geometry(s, SR_MODE_BVH))) return rc;
        if ((rc = sync_geometry(s, SR_MODE_BRUTE))) return rc;
    }
    return SR_OK;
}

int sr_build_voxels(sr_scene* s) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_build_voxels");
    if (!s->parts.empty()) {
        for (sr_scene* q : s->parts) { int rc = sr_build_voxels(q); if (rc) return rc; }
        return SR_OK;
    }
    if (!s->have_model || s->ntris == 0) return fail(SR_ERR_NO_MODEL, "no model");
    if (s->vox_valid) return SR_OK;
    if (s->device < 0) return ensure_voxels(s, nullptr);
    int rc = use_device(s);
    if (rc) return rc;
    if ((rc = sync_geometry(s, ~0u))) return rc;
    return ensure_voxels(s, nullptr);
}

int sr_get_voxels(sr_scene* s, uint32_t* colors, double* normals) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_get_voxels");
    if (!s->vox_valid) return fail(SR_ERR_NOT_BUILT, "no voxel grid: call sr_build_voxels (or render a SR_F_VOXELS frame) after setting the triangles");
    const size_t cells = (size_t)s->vox_res * s->vox_res * s->vox_res;
    if (s->device < 0) {
        if (colors) std::memcpy(colors, s->vox_colors_host.data(), cells * 4);
        if (normals) std::memcpy(normals, s->vox_normals_host.data(), cells * 3 * sizeof(double));
        return SR_OK;
    }
    int rc = use_device(s);
    if (rc) return rc;
    if (colors) SR_HIP(hipMemcpy(colors, s->d_vox_colors.p, cells * 4, hipMemcpyDeviceToHost));
    if (normals) SR_HIP(hipMemcpy(normals, s->d_vox_normals.p, cells * 3 * sizeof(double), hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_set_voxel_res(sr_scene* s, int32_t n) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_set_voxel_res");
    if (n < 1 || n > sr::kVoxelGridMax) return fail(SR_ERR_INVALID_ARG, "voxel grid resolution must be 1..256");
    if (!s->parts.empty()) {                                         // every part builds its own grid
        for (sr_scene* q : s->parts) { int rc = sr_set_voxel_res(q, n); if (rc) return rc; }
        return SR_OK;
    }
    if (n == s->vox_res) return SR_OK;                                // the same value keeps the grid
    s->vox_res = n;
    s->vox_valid = false;                                             // another size is another grid: the next build or voxel frame makes it
    return SR_OK;
}

int32_t sr_get_voxel_res(const sr_scene* s) {
    if (s && !s->parts.empty()) s = s->parts[0];
    return s ? s->vox_res : 0;
}

int sr_tree_stats(const sr_scene* s, int32_t out[4]) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "bad argument");
    if (!s->ref.built) return fail(SR_ERR_NOT_BUILT, "reference tree not built");
    out[0] = s->ref.tree_depth; out[1] = s->ref.num_nodes; out[2] = s->ref.num_leaf_nodes; out[3] = s->ref.num_nodes - s->ref.num_leaf_nodes;
    return SR_OK;
}

int64_t sr_tree_handle_leaf(const sr_scene* s, int64_t tri, double box[6], int32_t* members, int64_t cap) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || !box || cap < 0 || (cap > 0 && !members)) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_tree_handle_leaf");
    const sr_scene* h = s->host_src ? s->host_src : s;              // where the host arrays are
    if (!h->ref.built || h->ref.handle_leaf.empty()) return fail(SR_ERR_NOT_BUILT, "reference tree not built");
    if (tri < 0 || (size_t)tri >= h->ref.handle_leaf.size()) return fail(SR_ERR_INVALID_ARG, "sr_tree_handle_leaf: no such triangle");
    const int32_t leaf = h->ref.handle_leaf[(size_t)tri];
    if (leaf < 0) return fail(SR_ERR_NOT_BUILT, "sr_tree_handle_leaf: the triangle is in no leaf");
    const sr::RefNode& n = h->ref.nodes[(size_t)leaf];
    const sr::LeafBox& lb = h->ref.leaf_boxes[(size_t)n.box];
    for (int a = 0; a < 3; ++a) { box[a] = lb.lo[a]; box[3 + a] = lb.hi[a]; }
    for (int64_t k = 0; k < n.b && k < cap; ++k) members[k] = h->ref.leaf_tris[(size_t)n.a + (size_t)k];
    return n.b;
}

int sr_bvh_stats(const sr_scene* s, int64_t out[4]) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "bad argument");
    if (!s->bvh.built) return fail(SR_ERR_NOT_BUILT, "BVH not built");
    out[0] = s->bvh.depth; out[1] = (int64_t)(s->bvh_on_device ? s->bvh_num_nodes : s->bvh.nodes.size()); out[2] = (int64_t)s->ntris; out[3] = s->bvh_on_device ? 1 : 0;
    return SR_OK;
}

int sr_wide_tree_stats(const sr_scene* s, int64_t out[5]) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "bad argument");
    if (!s->bvh.built) return fail(SR_ERR_NOT_BUILT, "BVH not built");
    std::vector<sr::Bvh4Node> wide;
    if (s->bvh_on_device) {                                            // collapsed on the device: its nodes are read back
        SR_HIP(hipSetDevice(s->device));
        wide.resize(s->b4_num);
        SR_HIP(hipDeviceSynchronize());
        if (s->b4_num) SR_HIP(hipMemcpy(wide.data(), s->d_b4.p, s->b4_num * sizeof(sr::Bvh4Node), hipMemcpyDeviceToHost));
        out[0] = s->b4_depth;
    } else {
        out[0] = sr::collapse_bvh4(s->bvh.nodes.data(), s->bvh.nodes.size(), wide);
    }
    out[1] = (int64_t)wide.size();
    out[2] = out[3] = out[4] = 0;
    std::vector<char> linked(wide.size(), 0);
    for (const sr::Bvh4Node& n : wide)
        for (const sr::Bvh4Child& c : n.ch) {
            if (c.n < 0) continue;
            out[2]++;                                                  // child slots in use
            if (c.n > 0) { out[3]++; out[4] += c.n; }                  // leaves, triangles in leaves
            else if (c.c <= 0 || (size_t)c.c >= wide.size() || linked[(size_t)c.c]++) return fail(SR_ERR_UNSUPPORTED, "wide tree: bad inner link");
        }
    return SR_OK;
}

int sr_bvh_digest(const sr_scene* s, uint64_t out[2]) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "bad argument");
    if (!s->bvh.built || s->bvh_on_device) return fail(SR_ERR_NOT_BUILT, "no host-built BVH");
    auto fnv = [](const void* p, size_t bytes) {
        uint64_t h = 1469598103934665603ull;
        const unsigned char* c = (const unsigned char*)p;
        for (size_t i = 0; i < bytes; ++i) { h ^= c[i]; h *= 1099511628211ull; }
        return h;
    };
    out[0] = fnv(s->bvh.nodes.data(), s->bvh.nodes.size() * sizeof(sr::BvhNode));
    out[1] = fnv(s->bvh.order.data(), s->bvh.order.size() * sizeof(int32_t));
    return SR_OK;
}

int64_t sr_frame_pixel_count(const sr_frame* f) {
    if (!f || f->width <= 0 || f->height <= 0) return 0;
    int a, b;
    clamp_rows(f, a, b);
    if (f->strip_count <= 0) return (int64_t)f->width * f->height;
    int64_t rows = 0;
    for (int r = a; r <= b; ++r) if (row_owned(f, r)) rows++;
    return rows * f->width;
}

int sr_reset_shadow_cache(sr_scene* s) {
    if (s && !s->parts.empty()) { for (sr_scene* q : s->parts) { q->shadow_cache_empty = true; q->shadow_cache_host.clear(); } return SR_OK; }
    if (!s) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_reset_shadow_cache");
    s->shadow_cache_empty = true;
    s->shadow_cache_host.clear();
    return SR_OK;
}

// the static shadow cache as the reference's .cache file holds it (a multi-device scene keeps it on the first part, where static frames run)
int sr_get_shadow_cache(sr_scene* s, uint8_t* out) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_get_shadow_cache");
    const size_t cells = sr::pipeline_static_cells();
    if (s->device < 0) {
        if (s->shadow_cache_host.empty()) std::memset(out, 0, cells);
        else std::memcpy(out, s->shadow_cache_host.data(), cells);
        return SR_OK;
    }
    if (s->shadow_cache_empty || !s->d_shadow_cache.p) { std::memset(out, 0, cells); return SR_OK; }
    int rc = use_device(s);
    if (rc) return rc;
    if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));       // a frame in flight may still be filling cells
    SR_HIP(hipMemcpy(out, s->d_shadow_cache.p, cells, hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_set_shadow_cache(sr_scene* s, const uint8_t* in) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || !in) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_set_shadow_cache");
    const size_t cells = sr::pipeline_static_cells();
    if (s->device < 0) { s->shadow_cache_host.assign(in, in + cells); return SR_OK; }
    int rc = use_device(s);
    if (rc) return rc;
    if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));       // a frame in flight may still read the old bytes
    SR_HIP(s->d_shadow_cache.reserve(cells));
    SR_HIP(hipMemcpy(s->d_shadow_cache.p, in, cells, hipMemcpyHostToDevice));
    s->shadow_cache_empty = false;                                       // (the next static frame must not zero what was set)
    return SR_OK;
}

int sr_reset_ao_cache(sr_scene* s) {
    if (s && !s->parts.empty()) s = s->parts[0];                    // (a multi-device scene renders its AO frames on the first part)
    if (!s) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_reset_ao_cache");
    s->ao_cache_empty = true;
    s->ao_cache_host.clear();
    return SR_OK;
}

int sr_get_ao_cache(sr_scene* s, uint8_t* out) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_get_ao_cache");
    if (s->device < 0) {
        if (s->ao_cache_host.empty()) std::memset(out, 0, kAoCells);
        else std::memcpy(out, s->ao_cache_host.data(), kAoCells);
        return SR_OK;
    }
    if (s->ao_cache_empty || !s->d_ao_cache.p) { std::memset(out, 0, kAoCells); return SR_OK; }
    int rc = use_device(s);
    if (rc) return rc;
    if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));       // a frame in flight may still be filling cells
    SR_HIP(hipMemcpy(out, s->d_ao_cache.p, kAoCells, hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_set_ao_cache(sr_scene* s, const uint8_t* in) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || !in) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_set_ao_cache");
    if (s->device < 0) { s->ao_cache_host.assign(in, in + kAoCells); return SR_OK; }
    int rc = use_device(s);
    if (rc) return rc;
    if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));       // a frame in flight may still read the old bytes
    SR_HIP(s->d_ao_cache.reserve(kAoCells));
    SR_HIP(hipMemcpy(s->d_ao_cache.p, in, kAoCells, hipMemcpyHostToDevice));
    s->ao_cache_empty = false;
    return SR_OK;
}

int sr_set_light_field_res(sr_scene* s, int32_t n) {
    if (s && !s->parts.empty()) s = s->parts[0];                    // (a multi-device scene renders its light-field frames on the first part)
    if (!s) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_set_light_field_res");
    if (n < 1 || n > kMaxLightFieldRes) return fail(SR_ERR_INVALID_ARG, "light field resolution must be 1..128");
    if (n == s->lf_res) return SR_OK;
    if (s->device >= 0 && s->d_lf_cache.p) {                        // another resolution is another table: the old one goes (4 GiB at 128)
        int rc = use_device(s);
        if (rc) return rc;
        if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));
        s->d_lf_cache.release(); s->d_lf_claim.release();
    }
    if (s->device >= 0 && s->d_lft_cache.p) {                       // ... and the triangle table's
        int rc = use_device(s);
        if (rc) return rc;
        if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));
        s->d_lft_cache.release(); s->d_lft_claim.release();
    }
    s->lf_res = n;
    s->lf_cache_empty = true;
    s->lf_cache_host.clear();
    s->lft_cache_empty = true;
    s->lft_cache_host.clear();
    return SR_OK;
}

int32_t sr_get_light_field_res(const sr_scene* s) {
    if (s && !s->parts.empty()) s = s->parts[0];
    return s ? s->lf_res : 0;
}

int sr_set_light_field_shadows(sr_scene* s, int32_t on) {
    if (!s || (on != 0 && on != 1)) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_set_light_field_shadows (0 or 1)");
    s->lf_shadows = on != 0;                                        // (the table stays: an entry keeps what the frame that filled it stored)
    for (sr_scene* part : s->parts) part->lf_shadows = on != 0;
    return SR_OK;
}

int32_t sr_get_light_field_shadows(const sr_scene* s) {
    return (s && s->lf_shadows) ? 1 : 0;
}

int sr_set_light_field_interpolation(sr_scene* s, int32_t on) {
    if (!s || (on != 0 && on != 1)) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_set_light_field_interpolation (0 or 1)");
    s->lf_interp = on != 0;                                         // (the table stays: both lookups read and fill the same entries)
    for (sr_scene* part : s->parts) part->lf_interp = on != 0;
    return SR_OK;
}

int32_t sr_get_light_field_interpolation(const sr_scene* s) {
    return (s && s->lf_interp) ? 1 : 0;
}

int sr_set_light_field_triangles(sr_scene* s, int32_t on) {
    if (!s || (on != 0 && on != 1)) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_set_light_field_triangles (0 or 1)");
    s->lf_tris = on != 0;                                           // (both tables stay: the switch selects which one a frame reads and fills)
    for (sr_scene* part : s->parts) part->lf_tris = on != 0;
    return SR_OK;
}

int32_t sr_get_light_field_triangles(const sr_scene* s) {
    return (s && s->lf_tris) ? 1 : 0;
}

int sr_get_light_field_tris(sr_scene* s, uint32_t* out, uint64_t first, uint64_t count) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || (!out && count)) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_get_light_field_tris");
    const uint64_t entries = lf_entries(s->lf_res);
    if (first > entries || count > entries - first) return fail(SR_ERR_INVALID_ARG, "sr_get_light_field_tris: the range exceeds the 4 N^4 entries");
    if (count == 0) return SR_OK;
    if (s->device < 0) {
        if (s->lft_cache_host.empty()) std::memset(out, 0, (size_t)count * 4);
        else std::memcpy(out, s->lft_cache_host.data() + first, (size_t)count * 4);
        return SR_OK;
    }
    if (s->lft_cache_empty || !s->d_lft_cache.p) { std::memset(out, 0, (size_t)count * 4); return SR_OK; }
    int rc = use_device(s);
    if (rc) return rc;
    if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));      // a frame in flight may still be filling cells
    SR_HIP(hipMemcpy(out, (const uint32_t*)s->d_lft_cache.p + first, (size_t)count * 4, hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_set_light_field_tris(sr_scene* s, const uint32_t* in, uint64_t first, uint64_t count) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || (!in && count)) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_set_light_field_tris");
    const uint64_t entries = lf_entries(s->lf_res);
    if (first > entries || count > entries - first) return fail(SR_ERR_INVALID_ARG, "sr_set_light_field_tris: the range exceeds the 4 N^4 entries");
    if (count == 0) return SR_OK;
    if (s->device < 0) {
        if (s->lft_cache_host.empty()) s->lft_cache_host.assign((size_t)entries, 0u);
        std::memcpy(s->lft_cache_host.data() + first, in, (size_t)count * 4);
        return SR_OK;
    }
    int rc = use_device(s);
    if (rc) return rc;
    if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));
    if (!s->d_lft_cache.p || !s->d_lft_claim.p) s->lft_cache_empty = true;
    SR_HIP(s->d_lft_cache.reserve((size_t)entries * 4));
    SR_HIP(s->d_lft_claim.reserve((size_t)((entries + 31) / 32 * 4)));
    if (s->lft_cache_empty) {                                            // the entries outside the range are those of a new Renderer
        SR_HIP(hipMemset(s->d_lft_cache.p, 0, (size_t)entries * 4));
        SR_HIP(hipMemset(s->d_lft_claim.p, 0, (size_t)((entries + 31) / 32 * 4)));
        s->lft_cache_empty = false;
    }
    SR_HIP(hipMemcpy((uint32_t*)s->d_lft_cache.p + first, in, (size_t)count * 4, hipMemcpyHostToDevice));
    return SR_OK;
}

int sr_light_field_coords(sr_scene* s, int64_t n, const double* starts, const double* dirs, double* coords, uint8_t* inside) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || n < 0 || (n > 0 && (!starts || !dirs || !coords || !inside))) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_light_field_coords");
    int rc = use_device(s);
    if (rc) return rc;
    if (n == 0) return SR_OK;
    size_t sizes[4] = {(size_t)n * 24, (size_t)n * 24, (size_t)n * 32, (size_t)n};
    for (int i = 0; i < 4; ++i) SR_HIP(s->d_io[i].reserve(sizes[i]));
    SR_HIP(hipMemcpy(s->d_io[0].p, starts, sizes[0], hipMemcpyHostToDevice));
    SR_HIP(hipMemcpy(s->d_io[1].p, dirs, sizes[1], hipMemcpyHostToDevice));
    SR_HIP(sr::launch_lf_coords(n, (const double*)s->d_io[0].p, (const double*)s->d_io[1].p, s->lf_res, (double*)s->d_io[2].p, (uint8_t*)s->d_io[3].p, nullptr));
    SR_HIP(hipStreamSynchronize(nullptr));
    SR_HIP(hipMemcpy(coords, s->d_io[2].p, sizes[2], hipMemcpyDeviceToHost));
    SR_HIP(hipMemcpy(inside, s->d_io[3].p, sizes[3], hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_reset_light_field(sr_scene* s) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_reset_light_field");
    s->lf_cache_empty = true;
    s->lf_cache_host.clear();
    s->lft_cache_empty = true;                                      // (both tables: a new Renderer has neither)
    s->lft_cache_host.clear();
    return SR_OK;
}

int sr_get_light_field(sr_scene* s, uint32_t* out, uint64_t first, uint64_t count) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || (!out && count)) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_get_light_field");
    const uint64_t entries = lf_entries(s->lf_res);
    if (first > entries || count > entries - first) return fail(SR_ERR_INVALID_ARG, "sr_get_light_field: the range exceeds the 4 N^4 entries");
    if (count == 0) return SR_OK;
    if (s->device < 0) {
        if (s->lf_cache_host.empty()) std::memset(out, 0, (size_t)count * 4);
        else std::memcpy(out, s->lf_cache_host.data() + first, (size_t)count * 4);
        return SR_OK;
    }
    if (s->lf_cache_empty || !s->d_lf_cache.p) { std::memset(out, 0, (size_t)count * 4); return SR_OK; }
    int rc = use_device(s);
    if (rc) return rc;
    if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));       // a frame in flight may still be filling cells
    SR_HIP(hipMemcpy(out, (const uint32_t*)s->d_lf_cache.p + first, (size_t)count * 4, hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_set_light_field(sr_scene* s, const uint32_t* in, uint64_t first, uint64_t count) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || (!in && count)) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_set_light_field");
    const uint64_t entries = lf_entries(s->lf_res);
    if (first > entries || count > entries - first) return fail(SR_ERR_INVALID_ARG, "sr_set_light_field: the range exceeds the 4 N^4 entries");
    if (count == 0) return SR_OK;
    if (s->device < 0) {
        if (s->lf_cache_host.empty()) s->lf_cache_host.assign((size_t)entries, 0u);
        std::memcpy(s->lf_cache_host.data() + first, in, (size_t)count * 4);
        return SR_OK;
    }
    int rc = use_device(s);
    if (rc) return rc;
    if (s->pre_used_set) SR_HIP(hipEventSynchronize(s->pre_used));       // a frame in flight may still read the old entries
    if (!s->d_lf_cache.p || !s->d_lf_claim.p) s->lf_cache_empty = true;
    SR_HIP(s->d_lf_cache.reserve((size_t)entries * 4));
    SR_HIP(s->d_lf_claim.reserve((size_t)((entries + 31) / 32 * 4)));
    if (s->lf_cache_empty) {                                             // the entries outside the range are those of a new Renderer
        SR_HIP(hipMemset(s->d_lf_cache.p, 0, (size_t)entries * 4));
        SR_HIP(hipMemset(s->d_lf_claim.p, 0, (size_t)((entries + 31) / 32 * 4)));
        s->lf_cache_empty = false;
    }
    SR_HIP(hipMemcpy((uint32_t*)s->d_lf_cache.p + first, in, (size_t)count * 4, hipMemcpyHostToDevice));
    return SR_OK;
}

// cells per k_lf_bake launch: 2^24 (2048 origin patches at N = 64, four launches for that table).  Measured on 1 M triangles: 38 ms per
// launch, and the launches' event times add up to the call's time within 0.1 ms -- the cut costs nothing measurable
const uint64_t kBakeLaunchCells = 1ull << 24;

int sr_bake_light_field(sr_scene* m, const sr_frame* f, uint64_t first, uint64_t count, uint64_t* filled) {
    sr_scene* s = (m && !m->parts.empty()) ? m->parts[0] : m;       // (a multi-device scene keeps its light field on the first part)
    if (!s || !f) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_bake_light_field");
    if (!(f->flags & SR_F_LIGHT_FIELD)) return fail(SR_ERR_INVALID_ARG, "sr_bake_light_field: the frame must carry SR_F_LIGHT_FIELD");
    const uint64_t entries = lf_entries(s->lf_res);
    if (first > entries || count > entries - first) return fail(SR_ERR_INVALID_ARG, "sr_bake_light_field: the range exceeds the 4 N^4 entries");
    int rc = validate_frame(f, s);
    if (rc) return rc;
    if ((rc = check_frame_mode(s, f))) return rc;
    if ((rc = use_device(s))) return rc;
    if (filled) *filled = 0;
    for (uint64_t& v : s->last_stats) v = 0;
    if (m != s) std::memcpy(m->last_stats, s->last_stats, sizeof(m->last_stats));
    if (count == 0) return SR_OK;
    if ((rc = ensure_io_streams(s))) return rc;
    hipStream_t stream = s->io_stream;
    sr::FrameConst fc;
    if ((rc = prepare_frame(s, f, fc))) return rc;
    if ((rc = sync_geometry(s, (uint32_t)f->trace_mode))) return rc;
    // [0 .. SR_STATS_COUNT) the ray statistics, [SR_STATS_COUNT] the entries written
    uint64_t back[SR_STATS_COUNT + 1];
    SR_HIP(s->d_stats.reserve(sizeof(back)));
    if (f->flags & SR_F_SHADOWS) {
        // with shadows (validate_frame: the scene's switch is on): a frame's set-up, then passes of canonical rays + shadow stage + k_lf_store
        SR_HIP(hipMemsetAsync(s->d_stats.p, 0, sizeof(back), stream));
        const LfBakeReq req{first, count, (unsigned long long*)s->d_stats.p + SR_STATS_COUNT};
        if ((rc = render_common(s, f, nullptr, stream, (unsigned long long*)s->d_stats.p, &req))) { (void)hipStreamSynchronize(stream); return rc; }
    } else {
        // ordered like a frame: after whatever frame is in flight (it may be filling cells), and the next frame after the bake
        StreamOrder order(s, stream);
        if (order.entered) return order.entered;
        SR_HIP(hipMemsetAsync(s->d_stats.p, 0, sizeof(back), stream));
        const bool lft = s->lf_tris;
        if (lft && (rc = sync_geometry(s, SR_MODE_REF_TREE))) return rc;
        if ((rc = lft ? ensure_light_field_tris(s, stream) : ensure_light_field(s, stream))) return rc;
        sr::BakeLaunch B{};
        B.tris = lft;
        B.sc = dev_scene(s);
        B.fc = fc;
        B.mode = f->trace_mode;
        B.points = (const double*)s->d_lf_points.p;
        B.res = s->lf_res;
        B.cache = (uint32_t*)(lft ? s->d_lft_cache.p : s->d_lf_cache.p);
        B.first = first; B.count = count;
        B.launch_cells = kBakeLaunchCells;
        B.packet = s->dbg[SR_DBG_KERNEL_SWITCH] == 35;              // (hook 35: the measured-and-rejected packet walk, same table)
        B.walk_stats = !(f->flags & SR_F_PRIMARY_STATS_ONLY);
        B.stats = (unsigned long long*)s->d_stats.p;
        B.filled = (unsigned long long*)s->d_stats.p + SR_STATS_COUNT;
        B.stream = stream;
        B.user = s;
        B.get_events = timing_events;
        const hipError_t e = sr::launch_lf_bake(B);
        if (e != hipSuccess) { (void)hipStreamSynchronize(stream); SR_HIP(e); }
    }
    SR_HIP(hipMemcpyAsync(back, s->d_stats.p, sizeof(back), hipMemcpyDeviceToHost, stream));
    SR_HIP(hipStreamSynchronize(stream));
    std::memcpy(s->last_stats, back, sizeof(s->last_stats));
    if (m != s) std::memcpy(m->last_stats, s->last_stats, sizeof(m->last_stats));
    if (filled) *filled = back[SR_STATS_COUNT];
    return SR_OK;
}

static int multi_render(sr_scene* m, const sr_frame* f, int32_t* host_pixels, void* d_pixels, hipStream_t user_stream, uint64_t* stats4, uint64_t* d_stats) {
    int rc = validate_frame(f, m);
    if (rc) return rc;
    if (d_stats) return fail(SR_ERR_UNSUPPORTED, "device-side statistics are per device: use sr_render / sr_last_ray_stats with a multi-device scene");
    const int n = (int)m->parts.size();
    m->last_parts = 1;
    if (!multi_splittable(f)) {                                     // static shadow cache / caller-made strips: the first part renders it
        rc = host_pixels ? sr_render(m->parts[0], f, host_pixels, stats4) : sr_render_device(m->parts[0], f, d_pixels, user_stream, nullptr);
        std::memcpy(m->last_stats, m->parts[0]->last_stats, sizeof(m->last_stats));     // sr_last_ray_stats(multi scene) reports this frame
        return rc;
    }
    if ((rc = check_frame_mode(m->parts[0], f))) return rc;
    int a, b;
    clamp_rows(f, a, b);
    if (b < a) { m->last_parts = 0; if (stats4) std::memset(stats4, 0, 4 * sizeof(uint64_t)); return SR_OK; }
    // ---- every part enqueues its strips on its own device and stream (nothing below waits for a GPU until all have been enqueued) ----
    std::vector<sr_frame> fg(n, *f);
    std::vector<int64_t> counts(n, 0);
    m->last_parts = 0;
    for (int g = 0; g < n; ++g) {
        fg[g].strip_rows = kMultiStripRows; fg[g].strip_count = n; fg[g].strip_index = g;
        counts[g] = sr_frame_pixel_count(&fg[g]);
        if (counts[g]) m->last_parts++;
    }
    // a path-traced frame runs in two phases per part, with the exchange of the rows' hit counts between them (sr_pipeline.hip k_pt_row_hits)
    const bool path = (f->flags & SR_F_PATH_TRACING) != 0;
    const size_t range_rows = (size_t)(b - a + 1);
    if (path && range_rows * 4 > m->pt_counts_cap) {
        if (m->pt_counts_host) {                                    // an earlier frame's copies may still read the old array
            for (sr_scene* q : m->parts) if (q->io_stream) { if ((rc = use_device(q))) return rc; SR_HIP(hipStreamSynchronize(q->io_stream)); }
            SR_HIP(hipHostFree(m->pt_counts_host));
        }
        m->pt_counts_host = nullptr; m->pt_counts_cap = 0;
        SR_HIP(hipHostMalloc(&m->pt_counts_host, range_rows * 4, hipHostMallocPortable));
        m->pt_counts_cap = range_rows * 4;
    }
    std::vector<hipEvent_t> exchanged(n, nullptr);                 // (SR_DBG_KERNEL_TIMING) stop events of the parts' exchange
    for (int g = 0; g < n; ++g) {
        sr_scene* q = m->parts[g];
        if (counts[g] == 0) continue;
        if ((rc = check_frame_mode(q, f))) return rc;
        if ((rc = use_device(q))) return rc;
        if ((rc = ensure_io_streams(q))) return rc;
        // the previous frame's gather may still be reading this part's strips (sr_render_device returns before the copies have run)
        if (m->multi_done) SR_HIP(hipStreamWaitEvent(q->io_stream, m->multi_done, 0));
        SR_HIP(q->d_pixels.reserve((size_t)counts[g] * 4));
        unsigned long long* ds = nullptr;
        if (stats4) {
            SR_HIP(q->d_stats.reserve(SR_STATS_COUNT * sizeof(uint64_t)));
            SR_HIP(hipMemsetAsync(q->d_stats.p, 0, SR_STATS_COUNT * sizeof(uint64_t), q->io_stream));
            ds = (unsigned long long*)q->d_stats.p;
        }
        if (path) {
            // phase 1, then the part's own rows of the counts travel to the pinned array (the rows of the other parts stay theirs)
            if ((rc = render_common(q, &fg[g], (uint32_t*)q->d_pixels.p, q->io_stream, ds, RenderAsk::phase(1)))) return rc;
            std::vector<StripRun> runs = strip_runs(a, b, n, g);
            for (StripRun& r : runs) { r.image_row -= a; r.compact_row = r.image_row; }
            hipEvent_t x0 = nullptr;                                // the exchange as this part sees it: its copy out, the wait for the others, the copy back
            if ((rc = next_events(q, sr::K_PT_EXCHANGE, x0, exchanged[g]))) return rc;
            if (x0) SR_HIP(hipEventRecord(x0, q->io_stream));
            SR_HIP(copy_runs(runs, n, 1, (const uint32_t*)q->d_pt_row_hits.p, (uint32_t*)m->pt_counts_host, hipMemcpyDeviceToHost, q->io_stream, true));
            if (!q->pt_counted) SR_HIP(hipEventCreateWithFlags(&q->pt_counted, hipEventDisableTiming));
            SR_HIP(hipEventRecord(q->pt_counted, q->io_stream));
            continue;
        }
        if ((rc = render_common(q, &fg[g], (uint32_t*)q->d_pixels.p, q->io_stream, ds))) return rc;
        if (!q->multi_done) SR_HIP(hipEventCreateWithFlags(&q->multi_done, hipEventDisableTiming));
        SR_HIP(hipEventRecord(q->multi_done, q->io_stream));
    }
    if (path) {
        // every part's first phase is enqueued: now each part waits for all the counts (events only), takes the complete array and goes on.
        // The rows of a part that owns none stay zero.  Through host memory whatever the devices can read of each other: 4 bytes per row
        // (every row of the range has exactly one owner, so the array is rewritten whole each frame; a part without rows records no event)
        for (int g = 0; g < n; ++g) {
            sr_scene* q = m->parts[g];
            if (counts[g] == 0) continue;
            if ((rc = use_device(q))) return rc;
            for (int h = 0; h < n; ++h) if (h != g && counts[h]) SR_HIP(hipStreamWaitEvent(q->io_stream, m->parts[h]->pt_counted, 0));
            SR_HIP(hipMemcpyAsync(q->d_pt_row_hits.p, m->pt_counts_host, range_rows * 4, hipMemcpyHostToDevice, q->io_stream));
            if (exchanged[g]) SR_HIP(hipEventRecord(exchanged[g], q->io_stream));
            if ((rc = render_common(q, &fg[g], (uint32_t*)q->d_pixels.p, q->io_stream, stats4 ? (unsigned long long*)q->d_stats.p : nullptr, RenderAsk::phase(2)))) return rc;
            if (!q->multi_done) SR_HIP(hipEventCreateWithFlags(&q->multi_done, hipEventDisableTiming));
            SR_HIP(hipEventRecord(q->multi_done, q->io_stream));
        }
    }
    // ---- the strips go straight to the caller's surface ----
    if (host_pixels) {
        // every device copies its own strips over its own link, all of them at once, into the (pinned for this call) surface
        HostPin pin(host_pixels + (size_t)a * f->width, (size_t)(b - a + 1) * f->width * 4);
        for (int g = 0; g < n; ++g) {
            sr_scene* q = m->parts[g];
            const std::vector<StripRun> runs = strip_runs(a, b, n, g);
            if (runs.empty() || counts[g] == 0) continue;
            if ((rc = use_device(q))) return rc;
            SR_HIP(hipStreamWaitEvent(q->copy_stream, q->multi_done, 0));
            SR_HIP(copy_runs(runs, n, f->width, (const uint32_t*)q->d_pixels.p, (uint32_t*)host_pixels, hipMemcpyDeviceToHost, q->copy_stream));
        }
        for (int k = 0; k < SR_STATS_COUNT; ++k) m->last_stats[k] = 0;
        for (int g = 0; g < n; ++g) {                               // one wait per device, after everything has been queued
            sr_scene* q = m->parts[g];
            if (counts[g] == 0) continue;
            if ((rc = use_device(q))) return rc;
            SR_HIP(hipStreamSynchronize(q->copy_stream));
            SR_HIP(hipStreamSynchronize(q->io_stream));
            if (stats4) {
                SR_HIP(hipMemcpy(q->last_stats, q->d_stats.p, SR_STATS_COUNT * sizeof(uint64_t), hipMemcpyDeviceToHost));
                for (int k = 0; k < SR_STATS_COUNT; ++k) m->last_stats[k] += q->last_stats[k];
            }
        }
        if (stats4) std::memcpy(stats4, m->last_stats, 4 * sizeof(uint64_t));
        return SR_OK;
    }
    // device surface on the first part's device.  SR_GATHER_RCCL: the one exchange step of SURVEY 8e -- grouped ncclSend (every other
    // part, on the stream its strips were rendered on) / ncclRecv (the first part, on the caller's stream) of the compact strip
    // buffers over xGMI, then the row de-interleave as strided device copies on the first device
    if (m->gather_kind == SR_GATHER_RCCL && n > 1) {
        const sr::RcclApi* api = sr::rccl_api(nullptr);
        if (!api || (int)m->comms.size() != n) return fail(SR_ERR_NOT_BUILT, "SR_GATHER_RCCL: sr_set_gather has not created the communicators");
        std::vector<size_t> off(n, 0);
        size_t total = 0;
        for (int g = 1; g < n; ++g) { off[g] = total; total += (size_t)counts[g]; }
        if ((rc = use_device(m->parts[0]))) return rc;
        SR_HIP(m->d_gather.reserve(std::max<size_t>(total, 1) * 4));
        SR_RCCL(api, api->GroupStart());
        for (int g = 1; g < n; ++g) {
            if (counts[g] == 0) continue;
            if ((rc = use_device(m->parts[g]))) { (void)api->GroupEnd(); return rc; }
            SR_RCCL(api, api->Send(m->parts[g]->d_pixels.p, (size_t)counts[g], sr::kRcclInt32, 0, m->comms[g], m->parts[g]->io_stream));
        }
        if ((rc = use_device(m->parts[0]))) { (void)api->GroupEnd(); return rc; }
        for (int g = 1; g < n; ++g) {
            if (counts[g] == 0) continue;
            SR_RCCL(api, api->Recv((uint32_t*)m->d_gather.p + off[g], (size_t)counts[g], sr::kRcclInt32, g, m->comms[0], user_stream));
        }
        SR_RCCL(api, api->GroupEnd());
        if (counts[0]) SR_HIP(hipStreamWaitEvent(user_stream, m->parts[0]->multi_done, 0));
        for (int g = 0; g < n; ++g) {
            const std::vector<StripRun> runs = strip_runs(a, b, n, g);
            if (runs.empty() || counts[g] == 0) continue;
            const uint32_t* src = g == 0 ? (const uint32_t*)m->parts[0]->d_pixels.p : (const uint32_t*)m->d_gather.p + off[g];
            SR_HIP(copy_runs(runs, n, f->width, src, (uint32_t*)d_pixels, hipMemcpyDeviceToDevice, user_stream));
        }
        if (!m->multi_done) SR_HIP(hipEventCreateWithFlags(&m->multi_done, hipEventDisableTiming));
        SR_HIP(hipEventRecord(m->multi_done, user_stream));
        return SR_OK;
    }
    // SR_GATHER_COPY (default): peer-to-peer over xGMI where the first device can read the part's memory, through pinned host
    // staging where it cannot (sr_create_multi asked; nothing is assumed)
    for (int g = 0; g < n; ++g) {
        sr_scene* q = m->parts[g];
        const std::vector<StripRun> runs = strip_runs(a, b, n, g);
        if (runs.empty() || counts[g] == 0) continue;
        if (q->can_peer && q->dbg[SR_DBG_NO_PEER] <= 0) {
            if ((rc = use_device(m->parts[0]))) return rc;
            SR_HIP(hipStreamWaitEvent(user_stream, q->multi_done, 0));
            SR_HIP(copy_runs(runs, n, f->width, (const uint32_t*)q->d_pixels.p, (uint32_t*)d_pixels, hipMemcpyDefault, user_stream));
        } else {
            const size_t bytes = (size_t)counts[g] * 4;
            if ((rc = use_device(q))) return rc;
            if (bytes > q->stage_cap) {
                if (q->stage_host) SR_HIP(hipHostFree(q->stage_host));
                q->stage_host = nullptr; q->stage_cap = 0;
                SR_HIP(hipHostMalloc(&q->stage_host, bytes, hipHostMallocPortable));
                q->stage_cap = bytes;
            }
            if (!q->staged) SR_HIP(hipEventCreateWithFlags(&q->staged, hipEventDisableTiming));
            SR_HIP(hipStreamWaitEvent(q->copy_stream, q->multi_done, 0));
            SR_HIP(hipMemcpyAsync(q->stage_host, q->d_pixels.p, bytes, hipMemcpyDeviceToHost, q->copy_stream));
            SR_HIP(hipEventRecord(q->staged, q->copy_stream));
            if ((rc = use_device(m->parts[0]))) return rc;
            SR_HIP(hipStreamWaitEvent(user_stream, q->staged, 0));
            SR_HIP(copy_runs(runs, n, f->width, (const uint32_t*)q->stage_host, (uint32_t*)d_pixels, hipMemcpyHostToDevice, user_stream));
        }
    }
    if ((rc = use_device(m->parts[0]))) return rc;
    if (!m->multi_done) SR_HIP(hipEventCreateWithFlags(&m->multi_done, hipEventDisableTiming));
    SR_HIP(hipEventRecord(m->multi_done, user_stream));
    return SR_OK;
}

int sr_render_device(sr_scene* s, const sr_frame* f, void* d_pixels, void* hip_stream, uint64_t* d_stats) {
    if (s && !s->parts.empty()) {
        if (!d_pixels) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_render_device");
        return multi_render(s, f, nullptr, d_pixels, (hipStream_t)hip_stream, nullptr, d_stats);
    }
    if (!s || !d_pixels) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_render_device");
    int rc = validate_frame(f, s);
    if (rc) return rc;
    if ((rc = check_frame_mode(s, f))) return rc;
    if ((rc = use_device(s))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (d_stats) SR_HIP(hipMemsetAsync(d_stats, 0, SR_STATS_COUNT * sizeof(uint64_t), stream));
    return render_common(s, f, (uint32_t*)d_pixels, stream, (unsigned long long*)d_stats);
}

int sr_render(sr_scene* s, const sr_frame* f, int32_t* pixels, uint64_t stats[4]) {
    if (s && !s->parts.empty()) {
        if (!pixels) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_render");
        return multi_render(s, f, pixels, nullptr, nullptr, stats, nullptr);
    }
    if (!s || !pixels) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_render");
    int rc = validate_frame(f, s);
    if (rc) return rc;
    if ((rc = check_frame_mode(s, f))) return rc;
    if ((rc = use_device(s))) return rc;
    int64_t count = sr_frame_pixel_count(f);
    {
        int a, b;
        clamp_rows(f, a, b);
        if (b < a || count == 0) { if (stats) std::memset(stats, 0, 4 * sizeof(uint64_t)); return SR_OK; }   // rayTraceStartRow > EndRow: nothing is drawn
    }
    SR_HIP(s->d_pixels.reserve((size_t)count * 4));
    if ((rc = ensure_io_streams(s))) return rc;
    unsigned long long* d_stats = nullptr;
    if (stats) {
        SR_HIP(s->d_stats.reserve(SR_STATS_COUNT * sizeof(uint64_t)));
        SR_HIP(hipMemsetAsync(s->d_stats.p, 0, SR_STATS_COUNT * sizeof(uint64_t), s->io_stream));
        d_stats = (unsigned long long*)s->d_stats.p;
    }
    // rows the reference would have drawn: [a, b] of the surface, or this call's strips as one compact block
    int a, b;
    clamp_rows(f, a, b);
    const bool strips = f->strip_count > 0;
    const size_t first_px = strips ? 0 : (size_t)a * f->width;
    const size_t total_px = strips ? (size_t)count : (size_t)(b - a + 1) * f->width;
    HostPin pin(pixels + first_px, total_px * 4);                  // (hidden behind the frame: nothing has been enqueued yet that we wait for)
    // ---- enqueue the frame; every row band leaves an event behind ----
    s->band_recs.clear();
    s->band_ev_used = 0;
    s->collect_bands = true;
    rc = render_common(s, f, (uint32_t*)s->d_pixels.p, s->io_stream, d_stats);
    const bool banded = s->collect_bands && !s->band_recs.empty();
    s->collect_bands = false;
    if (rc) { (void)hipStreamSynchronize(s->io_stream); return rc; }
    // ---- its way back: band by band on the copy stream, earliest bands first (the two half-frame pipelines run side by side) ----
    size_t covered = 0;
    if (banded) {
        std::stable_sort(s->band_recs.begin(), s->band_recs.end(), [](const sr_scene::BandRec& x, const sr_scene::BandRec& y) { return x.band < y.band; });
        for (const sr_scene::BandRec& r : s->band_recs) covered += (size_t)r.row_count * f->width;
    }
    if (banded && covered == total_px) {
        for (const sr_scene::BandRec& r : s->band_recs) {
            const size_t off = first_px + (size_t)r.row_begin * f->width, n = (size_t)r.row_count * f->width;
            SR_HIP(hipStreamWaitEvent(s->copy_stream, r.ev, 0));
            SR_HIP(hipMemcpyAsync(pixels + off, (const int32_t*)s->d_pixels.p + off, n * 4, hipMemcpyDeviceToHost, s->copy_stream));
        }
        SR_HIP(hipStreamSynchronize(s->copy_stream));
        SR_HIP(hipStreamSynchronize(s->io_stream));                 // (the join of the halves, the statistics)
    } else {
        // one-kernel frames (no bands): the whole range after the frame
        SR_HIP(hipStreamSynchronize(s->io_stream));
        SR_HIP(hipMemcpyAsync(pixels + first_px, (const int32_t*)s->d_pixels.p + first_px, total_px * 4, hipMemcpyDeviceToHost, s->copy_stream));
        SR_HIP(hipStreamSynchronize(s->copy_stream));
    }
    if (stats) {
        SR_HIP(hipMemcpy(s->last_stats, s->d_stats.p, SR_STATS_COUNT * sizeof(uint64_t), hipMemcpyDeviceToHost));
        std::memcpy(stats, s->last_stats, 4 * sizeof(uint64_t));
    }
    return SR_OK;
}

static int trace_prepare(sr_scene*& s, int32_t target, int64_t n, bool have_rays, int& mode, bool& with_extra) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || n < 0 || (n > 0 && !have_rays)) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_trace_rays");
    with_extra = (target & SR_TARGET_ROOT) != 0;
    mode = target & 0xff;
    if (!s->have_model) return fail(SR_ERR_NO_MODEL, "no model");
    int rc;
    if (target == SR_TARGET_VOXELS) {                               // VoxelGrid.IntersectRay: needs triangles only
        mode = -1; with_extra = false;
        if (s->ntris == 0) return fail(SR_ERR_NO_MODEL, "no model");
        if ((rc = use_device(s))) return rc;
        if ((rc = sync_geometry(s, ~0u))) return rc;
        return ensure_voxels(s, nullptr);
    }
    if (s->ntris == 0 && mode == SR_MODE_BRUTE) { /* empty model is fine for brute force */ }
    else if ((rc = check_mode(s, mode))) return rc;
    if ((rc = use_device(s))) return rc;
    return sync_geometry(s, (uint32_t)mode);
}

int sr_trace_rays_device(sr_scene* s, int32_t target, int64_t n, const double* d_starts, const double* d_dirs, uint8_t* d_hit, double* d_ray_frac,
                         double* d_pos, double* d_normal, uint32_t* d_color, int32_t* d_tri_index, int32_t* d_counters, void* hip_stream) {
    int mode; bool with_extra;
    int rc = trace_prepare(s, target, n, d_starts && d_dirs, mode, with_extra);
    if (rc || n == 0) return rc;
    sr::TraceLaunch L{};
    L.sc = dev_scene(s);
    L.mode = mode;
    L.with_extra = with_extra && !s->extra_recs.empty();
    L.n = n;
    L.starts = d_starts; L.dirs = d_dirs;
    L.hit = d_hit; L.ray_frac = d_ray_frac; L.pos = d_pos; L.normal = d_normal; L.color = d_color; L.tri = d_tri_index; L.counters = d_counters;
    L.stream = (hipStream_t)hip_stream;
    hipEvent_t e0, e1;
    if ((rc = next_events(s, sr::K_TRACE, e0, e1))) return rc;
    if (e0) SR_HIP(hipEventRecord(e0, L.stream));
    if (mode < 0) {
        if (s->pre_used_set) SR_HIP(hipStreamWaitEvent(L.stream, s->pre_used, 0));
        SR_HIP(sr::launch_voxel_trace(L, s->vox_box, voxel_grid_dev(s), 256 * 4, s->dbg[SR_DBG_KERNEL_SWITCH] == 42));
    } else
    SR_HIP(sr::launch_trace(L));
    if (e1) SR_HIP(hipEventRecord(e1, L.stream));
    return SR_OK;
}

int sr_trace_rays(sr_scene* s, int32_t target, int64_t n, const double* starts, const double* dirs, uint8_t* hit, double* ray_frac,
                  double* pos, double* normal, uint32_t* color, int32_t* tri_index, int32_t* counters) {
    int mode; bool with_extra;
    int rc = trace_prepare(s, target, n, starts && dirs, mode, with_extra);
    if (rc || n == 0) return rc;
    size_t sizes[9] = {(size_t)n * 24, (size_t)n * 24, (size_t)n, (size_t)n * 8, (size_t)n * 24, (size_t)n * 24, (size_t)n * 4, (size_t)n * 4, (size_t)n * 12};
    for (int i = 0; i < 9; ++i) SR_HIP(s->d_io[i].reserve(sizes[i]));
    SR_HIP(hipMemcpy(s->d_io[0].p, starts, sizes[0], hipMemcpyHostToDevice));
    SR_HIP(hipMemcpy(s->d_io[1].p, dirs, sizes[1], hipMemcpyHostToDevice));
    if ((rc = sr_trace_rays_device(s, target, n, (const double*)s->d_io[0].p, (const double*)s->d_io[1].p, (uint8_t*)s->d_io[2].p, (double*)s->d_io[3].p,
                                   (double*)s->d_io[4].p, (double*)s->d_io[5].p, (uint32_t*)s->d_io[6].p, (int32_t*)s->d_io[7].p, (int32_t*)s->d_io[8].p, nullptr)))
        return rc;
    SR_HIP(hipStreamSynchronize(nullptr));
    void* outs[7] = {hit, ray_frac, pos, normal, color, tri_index, counters};
    for (int i = 0; i < 7; ++i)
        if (outs[i]) SR_HIP(hipMemcpy(outs[i], s->d_io[2 + i].p, sizes[2 + i], hipMemcpyDeviceToHost));
    return SR_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Ray batches from one origin (sr_trace_origin_rays): sr_trace_rays' answers on the walk of a frame's primary stage
// ------------------------------------------------------------------------------------------------------------------
// what sr_trace_origin_rays[_device] refuses before the device is looked at, in the header's order; `s`: the scene that runs the call (the
// first part of a multi-device scene)
static int origin_rays_check(sr_scene*& s, int32_t target, const double* origin, int64_t n, const void* dirs, uint32_t options, int& mode, bool& with_extra) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || !origin || n < 0 || (n > 0 && !dirs) || (options & ~(uint32_t)SR_RAYS_COHERENT) || !std::isfinite(origin[0]) || !std::isfinite(origin[1]) ||
        !std::isfinite(origin[2]))
        return fail(SR_ERR_INVALID_ARG, "bad argument to sr_trace_origin_rays");
    if (target & SR_TARGET_VOXELS) return fail(SR_ERR_UNSUPPORTED, "sr_trace_origin_rays: the voxel grid (SR_TARGET_VOXELS) has no tree for a packet to walk; use sr_trace_rays");
    with_extra = (target & SR_TARGET_ROOT) != 0;
    mode = target & 0xff;
    if (!s->have_model) return fail(SR_ERR_NO_MODEL, "no model");
    return check_mode(s, mode);
}

// the frame render_common sets the call up as: one pixel, no decorator, the identity camera (render_common puts `origin` in its place)
static void origin_rays_frame(sr_frame& fs, int mode) {
    std::memset(&fs, 0, sizeof(fs));
    fs.width = fs.height = 1;
    fs.sub_pixel_res = 1;
    fs.trace_mode = mode;
    fs.transform[0] = fs.transform[5] = fs.transform[10] = 1.0;
    fs.inv_transform[0] = fs.inv_transform[5] = fs.inv_transform[10] = 1.0;
    fs.fov_depth = 1.0;
}

int sr_trace_origin_rays_device(sr_scene* m, int32_t target, const double origin[3], int64_t n, const double* d_dirs, uint8_t* d_hit, double* d_ray_frac,
                                double* d_pos, double* d_normal, uint32_t* d_color, int32_t* d_tri_index, uint32_t options, void* hip_stream, uint64_t* d_stats) {
    sr_scene* s = m;
    int mode; bool with_extra;
    int rc = origin_rays_check(s, target, origin, n, d_dirs, options, mode, with_extra);
    if (rc || n == 0) return rc;
    if ((rc = use_device(s))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (d_stats) SR_HIP(hipMemsetAsync(d_stats, 0, SR_STATS_COUNT * sizeof(uint64_t), stream));
    sr_frame fs;
    origin_rays_frame(fs, mode);
    const OriginReq req{{origin[0], origin[1], origin[2]}, n, d_dirs, {nullptr, nullptr, d_hit, d_ray_frac, d_pos, d_normal, d_color, d_tri_index},
                        (options & SR_RAYS_COHERENT) != 0, with_extra};
    return render_common(s, &fs, nullptr, stream, (unsigned long long*)d_stats, &req);
}

int sr_trace_origin_rays(sr_scene* m, int32_t target, const double origin[3], int64_t n, const double* dirs, uint8_t* hit, double* ray_frac, double* pos,
                         double* normal, uint32_t* color, int32_t* tri_index, uint32_t options, uint64_t stats[4]) {
    sr_scene* s = m;
    int mode; bool with_extra;
    int rc = origin_rays_check(s, target, origin, n, dirs, options, mode, with_extra);
    if (rc || n == 0) return rc;
    if ((rc = use_device(s))) return rc;
    Staged io[] = {{dirs, nullptr, (size_t)n * 24}, {nullptr, hit, (size_t)n}, {nullptr, ray_frac, (size_t)n * 8}, {nullptr, pos, (size_t)n * 24},
                   {nullptr, normal, (size_t)n * 24}, {nullptr, color, (size_t)n * 4}, {nullptr, tri_index, (size_t)n * 4}};
    return run_staged(m, s, io, 7, true, stats, [&](hipStream_t stream, unsigned long long* d_stats) {
        sr_frame fs;
        origin_rays_frame(fs, mode);
        const OriginReq req{{origin[0], origin[1], origin[2]}, n, (const double*)io[0].dev,
                            {nullptr, nullptr, (uint8_t*)io[1].dev, (double*)io[2].dev, (double*)io[3].dev, (double*)io[4].dev, (uint32_t*)io[5].dev, (int32_t*)io[6].dev},
                            (options & SR_RAYS_COHERENT) != 0, with_extra};
        return render_common(s, &fs, nullptr, stream, d_stats, &req);
    });
}

// ------------------------------------------------------------------------------------------------------------------
// The batch calls without a frame, on item_call_check / item_call / item_call_setup (above)
// ------------------------------------------------------------------------------------------------------------------
// ---- Any-hit ray batches with a distance limit (sr_occluded_rays): sr_trace_rays' hit && ray_frac <= limit, with early exit on the own BVH
static const ItemCall kOccludedRaysCall = {
    "sr_occluded_rays", "starts, dirs and occluded must not be NULL when n > 0", false,
    SR_RAYS_COHERENT | SR_RAYS_ENDPOINTS, "unknown option bits (SR_RAYS_COHERENT and SR_RAYS_ENDPOINTS are the options)",
    "a hit on the voxel grid (SR_TARGET_VOXELS) has rayFrac 0, so a distance limit decides nothing; use sr_trace_rays", nullptr, nullptr};

static int occluded_rays_common(sr_scene* s, int mode, bool with_extra, int64_t n, const double* d_starts, const double* d_dirs, const double* d_limits,
                                uint8_t* d_occluded, uint32_t options, hipStream_t stream, unsigned long long* d_stats) {
    sr::OccludedLaunch L{};
    std::unique_ptr<StreamOrder> order;
    size_t slots;
    int rc = item_call_setup(s, mode, n, sr::kBatchMaxPass, mode == SR_MODE_BVH, stream, d_stats, order, L, slots);
    if (rc) return rc;
    const int64_t hook = s->dbg[SR_DBG_KERNEL_SWITCH];
    L.sc = dev_scene(s);
    L.mode = mode;
    L.with_extra = with_extra && !s->extra_recs.empty();
    L.starts = d_starts; L.dirs = d_dirs; L.limits = d_limits; L.occluded = d_occluded;
    L.endpoints = (options & SR_RAYS_ENDPOINTS) != 0;
    L.input_order = (options & SR_RAYS_COHERENT) != 0 || hook == 46;                            // (hook: input order whatever the options say)
    L.nearest_walks = hook == 47;                                                               // (hook: nearest-hit walks plus the comparison)
    L.refill_at = (hook >= 100 && hook <= 163) ? (int)(hook - 100) : -1;                       // (hook: persistent lanes, refilled at T busy ones)
    if (mode == SR_MODE_BVH) {
        if ((rc = ensure_num_cus(s))) return rc;
        L.persistent_blocks = s->num_cus * 4;
    }
    SR_HIP(sr::launch_occluded(L));
    return SR_OK;
}

int sr_occluded_rays_device(sr_scene* m, int32_t target, int64_t n, const double* d_starts, const double* d_dirs, const double* d_limits, uint8_t* d_occluded,
                            uint32_t options, void* hip_stream, uint64_t* d_stats) {
    return item_call(kOccludedRaysCall, m, target, n, d_starts && d_dirs && d_occluded, 0, options, {nullptr, 0, nullptr, hip_stream, d_stats},
                     [&](sr_scene* s, int mode, bool with_extra, hipStream_t stream, unsigned long long* stats) {
                         return occluded_rays_common(s, mode, with_extra, n, d_starts, d_dirs, d_limits, d_occluded, options, stream, stats);
                     });
}

int sr_occluded_rays(sr_scene* m, int32_t target, int64_t n, const double* starts, const double* dirs, const double* limits, uint8_t* occluded,
                     uint32_t options, uint64_t stats[4]) {
    Staged io[] = {{starts, nullptr, (size_t)n * 24}, {dirs, nullptr, (size_t)n * 24}, {limits, nullptr, (size_t)n * 8}, {nullptr, occluded, (size_t)n}};
    return item_call(kOccludedRaysCall, m, target, n, starts && dirs && occluded, 0, options, {io, 4, stats, nullptr, nullptr},
                     [&](sr_scene* s, int mode, bool with_extra, hipStream_t stream, unsigned long long* d_stats) {
                         return occluded_rays_common(s, mode, with_extra, n, (const double*)io[0].dev, (const double*)io[1].dev, (const double*)io[2].dev,
                                                     (uint8_t*)io[3].dev, options, stream, d_stats);
                     });
}

// ---- Nearest-hit ray batches with a distance limit (sr_nearest_rays): sr_trace_rays' answers on the mirror extension's incoherent-ray route
static const ItemCall kNearestRaysCall = {
    "sr_nearest_rays", "starts and dirs must not be NULL when n > 0", false,
    SR_RAYS_COHERENT | SR_RAYS_ENDPOINTS, "unknown option bits (SR_RAYS_COHERENT and SR_RAYS_ENDPOINTS are the options)",
    "the voxel grid (SR_TARGET_VOXELS) has no tree to walk and its hits have rayFrac 0; use sr_trace_rays", nullptr, nullptr};

struct NearestOut { uint8_t* hit; double* ray_frac; double* pos; double* normal; uint32_t* color; int32_t* tri; };

// (on the first scratch set's bounce buffers too)
static int nearest_rays_common(sr_scene* s, int mode, bool with_extra, int64_t n, const double* d_starts, const double* d_dirs, const double* d_limits,
                               const NearestOut& out, uint32_t options, hipStream_t stream, unsigned long long* d_stats) {
    const int64_t hook = s->dbg[SR_DBG_KERNEL_SWITCH];
    sr::NearestLaunch L{};
    L.lane_walks = hook == 49;                                                                  // (hook: every ray through k_nr_lane)
    const bool walked = mode == SR_MODE_BVH && !L.lane_walks;
    std::unique_ptr<StreamOrder> order;
    size_t slots;
    int rc = item_call_setup(s, mode, n, sr::kBatchMaxPass, walked, stream, d_stats, order, L, slots);
    if (rc) return rc;
    L.sc = dev_scene(s);
    L.mode = mode;
    L.with_extra = with_extra && !s->extra_recs.empty();
    L.starts = d_starts; L.dirs = d_dirs; L.limits = d_limits;
    L.hit = out.hit; L.ray_frac = out.ray_frac; L.pos = out.pos; L.normal = out.normal; L.color = out.color; L.tri = out.tri;
    L.endpoints = (options & SR_RAYS_ENDPOINTS) != 0;
    L.input_order = (options & SR_RAYS_COHERENT) != 0 || hook == 48;                            // (hook: input order whatever the options say)
    L.bvh2 = s->dbg[SR_DBG_BVH2_PACKETS] > 0;
    L.refill_at = (hook >= 100 && hook <= 163) ? (int)(hook - 100) : sr::kNearestRefillAt;     // (hook)
    L.lds_levels = (hook >= 200 && hook < 300) ? std::max(1, (int)(hook - 200)) : sr::pipeline_bounce_lds_levels();   // (hook)
    if (walked) {
        if ((rc = ensure_num_cus(s))) return rc;
        L.persistent_blocks = s->num_cus * 8;
        sr_scene::BandScratch& B = s->scratch[0];
        SR_HIP(B.bounce_prep.reserve(slots * 64));
        SR_HIP(B.bounce_res.reserve(slots * 16));
        // (k_nr_walk keeps L.lds_levels stack levels per lane in LDS, the rest of the worst case here: [level][lane of the grid])
        const long long deep = std::max(3 * (long long)s->b4_depth + 2, (long long)s->bvh.depth + 2) - L.lds_levels;
        if (deep > 0) SR_HIP(B.bounce_stack.reserve((size_t)deep * (size_t)s->num_cus * 8 * 256 * 4));
        L.prep = B.bounce_prep.p;
        L.res = B.bounce_res.p;
        L.deep = (int32_t*)B.bounce_stack.p;
        L.deep_bytes = B.bounce_stack.cap;
    }
    SR_HIP(sr::launch_nearest(L));
    return SR_OK;
}

int sr_nearest_rays_device(sr_scene* m, int32_t target, int64_t n, const double* d_starts, const double* d_dirs, const double* d_limits, uint8_t* d_hit,
                           double* d_ray_frac, double* d_pos, double* d_normal, uint32_t* d_color, int32_t* d_tri_index, uint32_t options, void* hip_stream,
                           uint64_t* d_stats) {
    return item_call(kNearestRaysCall, m, target, n, d_starts && d_dirs, 0, options, {nullptr, 0, nullptr, hip_stream, d_stats},
                     [&](sr_scene* s, int mode, bool with_extra, hipStream_t stream, unsigned long long* stats) {
                         const NearestOut out{d_hit, d_ray_frac, d_pos, d_normal, d_color, d_tri_index};
                         return nearest_rays_common(s, mode, with_extra, n, d_starts, d_dirs, d_limits, out, options, stream, stats);
                     });
}

int sr_nearest_rays(sr_scene* m, int32_t target, int64_t n, const double* starts, const double* dirs, const double* limits, uint8_t* hit, double* ray_frac,
                    double* pos, double* normal, uint32_t* color, int32_t* tri_index, uint32_t options, uint64_t stats[4]) {
    Staged io[] = {{starts, nullptr, (size_t)n * 24}, {dirs, nullptr, (size_t)n * 24}, {limits, nullptr, (size_t)n * 8}, {nullptr, hit, (size_t)n},
                   {nullptr, ray_frac, (size_t)n * 8}, {nullptr, pos, (size_t)n * 24}, {nullptr, normal, (size_t)n * 24}, {nullptr, color, (size_t)n * 4},
                   {nullptr, tri_index, (size_t)n * 4}};
    return item_call(kNearestRaysCall, m, target, n, starts && dirs, 0, options, {io, 9, stats, nullptr, nullptr},
                     [&](sr_scene* s, int mode, bool with_extra, hipStream_t stream, unsigned long long* d_stats) {
                         const NearestOut out{(uint8_t*)io[3].dev, (double*)io[4].dev, (double*)io[5].dev, (double*)io[6].dev, (uint32_t*)io[7].dev, (int32_t*)io[8].dev};
                         return nearest_rays_common(s, mode, with_extra, n, (const double*)io[0].dev, (const double*)io[1].dev, (const double*)io[2].dev, out, options,
                                                    stream, d_stats);
                     });
}

// ---- All hits along a ray, nearest first, with a count (sr_all_hits_rays): the walk that never stops at the first hit
static const ItemCall kAllHitsRaysCall = {
    "sr_all_hits_rays", "starts and dirs must not be NULL when n > 0", true,
    SR_RAYS_COHERENT | SR_RAYS_ENDPOINTS, "unknown option bits (SR_RAYS_COHERENT and SR_RAYS_ENDPOINTS are the options)",
    "the voxel grid (SR_TARGET_VOXELS) has no tree to walk and its hits have rayFrac 0; use sr_trace_rays", nullptr,
    "SR_MODE_REF_TREE has no notion of all hits (the literal walk ends in the first leaf that holds a hit inside its box, and a triangle lives in several "
    "leaves); use SR_MODE_BVH or SR_MODE_BRUTE"};

struct AllHitsOut { uint32_t* count; int32_t* index; double* ray_frac; };

// (a row the caller does not want lives in the first scratch set's bounce buffers)
static int all_hits_common(sr_scene* s, int mode, bool with_extra, int64_t n, const double* d_starts, const double* d_dirs, const double* d_limits,
                           int32_t max_hits, const AllHitsOut& out, uint32_t options, hipStream_t stream, unsigned long long* d_stats) {
    const bool own_rows = max_hits > 0 && (!out.index || !out.ray_frac);
    const int64_t max_pass = own_rows ? std::min<int64_t>(sr::kBatchMaxPass, (1ll << 24) / max_hits) : sr::kBatchMaxPass;   // (at most 2^24 slots of scratch rows: 128 + 64 MiB)
    sr::AllHitsLaunch L{};
    std::unique_ptr<StreamOrder> order;
    size_t slots;
    int rc = item_call_setup(s, mode, n, max_pass, mode == SR_MODE_BVH, stream, d_stats, order, L, slots);
    if (rc) return rc;
    const int64_t hook = s->dbg[SR_DBG_KERNEL_SWITCH];
    L.sc = dev_scene(s);
    L.mode = mode;
    L.with_extra = with_extra && !s->extra_recs.empty();
    L.starts = d_starts; L.dirs = d_dirs; L.limits = d_limits;
    L.max_hits = max_hits;
    L.count = out.count;
    L.index = max_hits > 0 ? out.index : nullptr;
    L.ray_frac = max_hits > 0 ? out.ray_frac : nullptr;
    L.endpoints = (options & SR_RAYS_ENDPOINTS) != 0;
    L.input_order = (options & SR_RAYS_COHERENT) != 0 || hook == 50;                            // (hook: input order whatever the options say)
    L.loop_all = hook == 51;                                                                    // (hook: every ray through the per-record loop)
    sr_scene::BandScratch& B = s->scratch[0];
    if (max_hits > 0 && !out.index) {
        SR_HIP(B.bounce_res.reserve(slots * (size_t)max_hits * sizeof(int32_t)));
        L.scratch_index = (int32_t*)B.bounce_res.p;
    }
    if (max_hits > 0 && !out.ray_frac) {
        SR_HIP(B.bounce_prep.reserve(slots * (size_t)max_hits * sizeof(double)));
        L.scratch_frac = (double*)B.bounce_prep.p;
    }
    SR_HIP(sr::launch_all_hits(L));
    return SR_OK;
}

int sr_all_hits_rays_device(sr_scene* m, int32_t target, int64_t n, const double* d_starts, const double* d_dirs, const double* d_limits, int32_t max_hits,
                            uint32_t* d_count, int32_t* d_index, double* d_ray_frac, uint32_t options, void* hip_stream, uint64_t* d_stats) {
    return item_call(kAllHitsRaysCall, m, target, n, d_starts && d_dirs, max_hits, options, {nullptr, 0, nullptr, hip_stream, d_stats},
                     [&](sr_scene* s, int mode, bool with_extra, hipStream_t stream, unsigned long long* stats) {
                         const AllHitsOut out{d_count, d_index, d_ray_frac};
                         return all_hits_common(s, mode, with_extra, n, d_starts, d_dirs, d_limits, max_hits, out, options, stream, stats);
                     });
}

int sr_all_hits_rays(sr_scene* m, int32_t target, int64_t n, const double* starts, const double* dirs, const double* limits, int32_t max_hits, uint32_t* count,
                     int32_t* index, double* ray_frac, uint32_t options, uint64_t stats[4]) {
    const size_t rows = (size_t)n * (size_t)max_hits;
    Staged io[] = {{starts, nullptr, (size_t)n * 24}, {dirs, nullptr, (size_t)n * 24}, {limits, nullptr, (size_t)n * 8}, {nullptr, count, (size_t)n * 4},
                   {nullptr, max_hits > 0 ? index : nullptr, rows * 4}, {nullptr, max_hits > 0 ? ray_frac : nullptr, rows * 8}};
    return item_call(kAllHitsRaysCall, m, target, n, starts && dirs, max_hits, options, {io, 6, stats, nullptr, nullptr},
                     [&](sr_scene* s, int mode, bool with_extra, hipStream_t stream, unsigned long long* d_stats) {
                         const AllHitsOut out{(uint32_t*)io[3].dev, (int32_t*)io[4].dev, (double*)io[5].dev};
                         return all_hits_common(s, mode, with_extra, n, (const double*)io[0].dev, (const double*)io[1].dev, (const double*)io[2].dev, max_hits, out,
                                                options, stream, d_stats);
                     });
}

// ---- The closest point of the mesh for a batch of points (sr_closest_points): the distance query of the own BVH
static const ItemCall kClosestPointsCall = {
    "sr_closest_points", "points must not be NULL when n > 0", false,
    SR_POINTS_COHERENT, "unknown option bits (SR_POINTS_COHERENT is the only option)",
    "the voxel grid (SR_TARGET_VOXELS) has no triangles to measure a distance to",
    "the closest points of the extra geometry (SR_TARGET_ROOT) are not part of the call; pass the mode alone",
    "SR_MODE_REF_TREE has no distance query (a triangle lives in several leaves of the reference tree); use SR_MODE_BVH or SR_MODE_BRUTE"};

struct ClosestOut { int32_t* tri; double* dist; double* pos; double* uv; };

static int closest_common(sr_scene* s, int mode, int64_t n, const double* d_points, const double* d_limits, const ClosestOut& out, uint32_t options,
                          hipStream_t stream, unsigned long long* d_stats) {
    sr::ClosestLaunch L{};
    std::unique_ptr<StreamOrder> order;
    size_t slots;
    int rc = item_call_setup(s, mode, n, sr::kBatchMaxPass, mode == SR_MODE_BVH, stream, d_stats, order, L, slots);
    if (rc) return rc;
    const int64_t hook = s->dbg[SR_DBG_KERNEL_SWITCH];
    L.sc = dev_scene(s);
    L.mode = mode;
    L.points = d_points; L.limits = d_limits;
    L.tri = out.tri; L.dist = out.dist; L.pos = out.pos; L.uv = out.uv;
    L.input_order = (options & SR_POINTS_COHERENT) != 0 || hook == 52;                          // (hook: input order whatever the options say)
    L.loop_all = hook == 53;                                                                    // (hook: every point through the per-record loop)
    SR_HIP(sr::launch_closest(L));
    return SR_OK;
}

int sr_closest_points_device(sr_scene* m, int32_t target, int64_t n, const double* d_points, const double* d_max_dist, int32_t* d_tri_index, double* d_dist,
                             double* d_pos, double* d_uv, uint32_t options, void* hip_stream, uint64_t* d_stats) {
    return item_call(kClosestPointsCall, m, target, n, d_points != nullptr, 0, options, {nullptr, 0, nullptr, hip_stream, d_stats},
                     [&](sr_scene* s, int mode, bool, hipStream_t stream, unsigned long long* stats) {
                         const ClosestOut out{d_tri_index, d_dist, d_pos, d_uv};
                         return closest_common(s, mode, n, d_points, d_max_dist, out, options, stream, stats);
                     });
}

int sr_closest_points(sr_scene* m, int32_t target, int64_t n, const double* points, const double* max_dist, int32_t* tri_index, double* dist, double* pos,
                      double* uv, uint32_t options, uint64_t stats[4]) {
    Staged io[] = {{points, nullptr, (size_t)n * 24}, {max_dist, nullptr, (size_t)n * 8}, {nullptr, tri_index, (size_t)n * 4}, {nullptr, dist, (size_t)n * 8},
                   {nullptr, pos, (size_t)n * 24}, {nullptr, uv, (size_t)n * 16}};
    return item_call(kClosestPointsCall, m, target, n, points != nullptr, 0, options, {io, 6, stats, nullptr, nullptr},
                     [&](sr_scene* s, int mode, bool, hipStream_t stream, unsigned long long* d_stats) {
                         const ClosestOut out{(int32_t*)io[2].dev, (double*)io[3].dev, (double*)io[4].dev, (double*)io[5].dev};
                         return closest_common(s, mode, n, (const double*)io[0].dev, (const double*)io[1].dev, out, options, stream, d_stats);
                     });
}

// ---- The triangles within reach of a point, nearest first, with a count (sr_near_triangles): sr_closest_points with a list
static const ItemCall kNearTrianglesCall = {
    "sr_near_triangles", "points must not be NULL when n > 0", true,
    SR_POINTS_COHERENT, "unknown option bits (SR_POINTS_COHERENT is the only option)",
    "the voxel grid (SR_TARGET_VOXELS) has no triangles to be near to",
    "the extra geometry (SR_TARGET_ROOT) has no triangle indices to list; pass the mode alone",
    "SR_MODE_REF_TREE has no distance query (a triangle lives in several leaves of the reference tree and would be listed twice); use SR_MODE_BVH or "
    "SR_MODE_BRUTE"};

struct NearOut { uint32_t* count; int32_t* index; double* dist; double* pos; double* uv; };

// (a row the walk needs and the caller does not want lives in the first scratch set's bounce buffers, as sr_all_hits_rays' rows)
static int near_common(sr_scene* s, int mode, int64_t n, const double* d_points, const double* d_limits, int32_t max_hits, const NearOut& out,
                       uint32_t options, hipStream_t stream, unsigned long long* d_stats) {
    const bool own_rows = max_hits > 0 && (!out.index || !out.dist);
    const int64_t max_pass = own_rows ? std::min<int64_t>(sr::kBatchMaxPass, (1ll << 24) / max_hits) : sr::kBatchMaxPass;   // (at most 2^24 slots of scratch rows)
    sr::NearLaunch L{};
    std::unique_ptr<StreamOrder> order;
    size_t slots;
    int rc = item_call_setup(s, mode, n, max_pass, mode == SR_MODE_BVH, stream, d_stats, order, L, slots);
    if (rc) return rc;
    const int64_t hook = s->dbg[SR_DBG_KERNEL_SWITCH];
    L.sc = dev_scene(s);
    L.mode = mode;
    L.points = d_points; L.limits = d_limits;
    L.max_hits = max_hits;
    L.count = out.count;
    L.index = max_hits > 0 ? out.index : nullptr;
    L.dist = max_hits > 0 ? out.dist : nullptr;
    L.pos = max_hits > 0 ? out.pos : nullptr;
    L.uv = max_hits > 0 ? out.uv : nullptr;
    L.input_order = (options & SR_POINTS_COHERENT) != 0 || hook == 54;                          // (hook: input order whatever the options say)
    L.loop_all = hook == 55;                                                                    // (hook: every point through the per-record loop)
    sr_scene::BandScratch& B = s->scratch[0];
    if (max_hits > 0 && !out.index) {
        SR_HIP(B.bounce_res.reserve(slots * (size_t)max_hits * sizeof(int32_t)));
        L.scratch_index = (int32_t*)B.bounce_res.p;
    }
    if (max_hits > 0 && !out.dist) {
        SR_HIP(B.bounce_prep.reserve(slots * (size_t)max_hits * sizeof(double)));
        L.scratch_dist = (double*)B.bounce_prep.p;
    }
    SR_HIP(sr::launch_near(L));
    return SR_OK;
}

int sr_near_triangles_device(sr_scene* m, int32_t target, int64_t n, const double* d_points, const double* d_max_dist, int32_t max_hits, uint32_t* d_count,
                             int32_t* d_index, double* d_dist, double* d_pos, double* d_uv, uint32_t options, void* hip_stream, uint64_t* d_stats) {
    return item_call(kNearTrianglesCall, m, target, n, d_points != nullptr, max_hits, options, {nullptr, 0, nullptr, hip_stream, d_stats},
                     [&](sr_scene* s, int mode, bool, hipStream_t stream, unsigned long long* stats) {
                         const NearOut out{d_count, d_index, d_dist, d_pos, d_uv};
                         return near_common(s, mode, n, d_points, d_max_dist, max_hits, out, options, stream, stats);
                     });
}

int sr_near_triangles(sr_scene* m, int32_t target, int64_t n, const double* points, const double* max_dist, int32_t max_hits, uint32_t* count, int32_t* index,
                      double* dist, double* pos, double* uv, uint32_t options, uint64_t stats[4]) {
    const size_t rows = (size_t)n * (size_t)max_hits;
    const bool k = max_hits > 0;
    Staged io[] = {{points, nullptr, (size_t)n * 24}, {max_dist, nullptr, (size_t)n * 8}, {nullptr, count, (size_t)n * 4}, {nullptr, k ? index : nullptr, rows * 4},
                   {nullptr, k ? dist : nullptr, rows * 8}, {nullptr, k ? pos : nullptr, rows * 24}, {nullptr, k ? uv : nullptr, rows * 16}};
    return item_call(kNearTrianglesCall, m, target, n, points != nullptr, max_hits, options, {io, 7, stats, nullptr, nullptr},
                     [&](sr_scene* s, int mode, bool, hipStream_t stream, unsigned long long* d_stats) {
                         const NearOut out{(uint32_t*)io[2].dev, (int32_t*)io[3].dev, (double*)io[4].dev, (double*)io[5].dev, (double*)io[6].dev};
                         return near_common(s, mode, n, (const double*)io[0].dev, (const double*)io[1].dev, max_hits, out, options, stream, d_stats);
                     });
}

// ---- The triangles of the model that cross a triangle of the caller's, with a count and the masks of the pairs (sr_overlap_triangles)
static const ItemCall kOverlapTrianglesCall = {
    "sr_overlap_triangles", "tris must not be NULL when n > 0", true,
    SR_POINTS_COHERENT | SR_OVERLAP_ANY, "unknown option bits (SR_POINTS_COHERENT and SR_OVERLAP_ANY are the options)",
    "the voxel grid (SR_TARGET_VOXELS) has no triangles to cross",
    "the extra geometry (SR_TARGET_ROOT) is not made of triangles with indices; pass the mode alone",
    "SR_MODE_REF_TREE has no overlap query (a triangle lives in several leaves of the reference tree and would be listed twice); use SR_MODE_BVH or "
    "SR_MODE_BRUTE",
    SR_OVERLAP_ANY, "SR_OVERLAP_ANY answers with a count of 0 or 1 and keeps no rows: max_hits must be 0"};

struct OverlapOut { uint32_t* count; int32_t* index; uint8_t* mask; };

// (an index row the masks need and the caller does not want lives in the first scratch set's bounce buffer, as sr_near_triangles' rows)
static int overlap_common(sr_scene* s, int mode, int64_t n, const double* d_tris, int32_t max_hits, const OverlapOut& out, uint32_t options, hipStream_t stream,
                          unsigned long long* d_stats) {
    const bool own_rows = max_hits > 0 && !out.index && out.mask;
    const int64_t max_pass = own_rows ? std::min<int64_t>(sr::kBatchMaxPass, (1ll << 24) / max_hits) : sr::kBatchMaxPass;   // (at most 2^24 slots of scratch rows)
    sr::OverlapLaunch L{};
    std::unique_ptr<StreamOrder> order;
    size_t slots;
    int rc = item_call_setup(s, mode, n, max_pass, mode == SR_MODE_BVH, stream, d_stats, order, L, slots);
    if (rc) return rc;
    const int64_t hook = s->dbg[SR_DBG_KERNEL_SWITCH];
    L.sc = dev_scene(s);
    L.mode = mode;
    L.tris = d_tris;
    L.max_hits = max_hits;
    L.any = (options & SR_OVERLAP_ANY) != 0;
    L.count = out.count;
    L.index = max_hits > 0 ? out.index : nullptr;
    L.mask = max_hits > 0 ? out.mask : nullptr;
    L.input_order = (options & SR_POINTS_COHERENT) != 0 || hook == 56;                          // (hook: input order whatever the options say)
    L.loop_all = hook == 57;                                                                    // (hook: every query through the per-record loop)
    if (own_rows) {
        sr_scene::BandScratch& B = s->scratch[0];
        SR_HIP(B.bounce_res.reserve(slots * (size_t)max_hits * sizeof(int32_t)));
        L.scratch_index = (int32_t*)B.bounce_res.p;
    }
    SR_HIP(sr::launch_overlap(L));
    return SR_OK;
}

int sr_overlap_triangles_device(sr_scene* m, int32_t target, int64_t n, const double* d_tris, int32_t max_hits, uint32_t* d_count, int32_t* d_index, uint8_t* d_mask,
                                uint32_t options, void* hip_stream, uint64_t* d_stats) {
    return item_call(kOverlapTrianglesCall, m, target, n, d_tris != nullptr, max_hits, options, {nullptr, 0, nullptr, hip_stream, d_stats},
                     [&](sr_scene* s, int mode, bool, hipStream_t stream, unsigned long long* stats) {
                         const OverlapOut out{d_count, d_index, d_mask};
                         return overlap_common(s, mode, n, d_tris, max_hits, out, options, stream, stats);
                     });
}

int sr_overlap_triangles(sr_scene* m, int32_t target, int64_t n, const double* tris, int32_t max_hits, uint32_t* count, int32_t* index, uint8_t* mask,
                         uint32_t options, uint64_t stats[4]) {
    const size_t rows = (size_t)n * (size_t)max_hits;
    const bool k = max_hits > 0;
    Staged io[] = {{tris, nullptr, (size_t)n * 72}, {nullptr, count, (size_t)n * 4}, {nullptr, k ? index : nullptr, rows * 4}, {nullptr, k ? mask : nullptr, rows}};
    return item_call(kOverlapTrianglesCall, m, target, n, tris != nullptr, max_hits, options, {io, 4, stats, nullptr, nullptr},
                     [&](sr_scene* s, int mode, bool, hipStream_t stream, unsigned long long* d_stats) {
                         const OverlapOut out{(uint32_t*)io[1].dev, (int32_t*)io[2].dev, (uint8_t*)io[3].dev};
                         return overlap_common(s, mode, n, (const double*)io[0].dev, max_hits, out, options, stream, d_stats);
                     });
}

// ------------------------------------------------------------------------------------------------------------------
// The RCCL strip gather, native: no PyTorch in the data path.
// ------------------------------------------------------------------------------------------------------------------
int sr_set_gather(sr_scene* m, int32_t kind) {
    if (!m || (kind != SR_GATHER_COPY && kind != SR_GATHER_RCCL)) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_set_gather");
    if (m->parts.empty()) return fail(SR_ERR_INVALID_ARG, "sr_set_gather: not a multi-device scene (sr_create_multi)");
    if (kind == SR_GATHER_RCCL && m->comms.empty() && m->parts.size() > 1) {
        std::string why;
        const sr::RcclApi* api = sr::rccl_api(&why);
        if (!api) return fail(SR_ERR_UNSUPPORTED, why);
        std::vector<int> devs;
        for (sr_scene* q : m->parts) devs.push_back(q->device);
        for (size_t i = 0; i < devs.size(); ++i)
            for (size_t j = i + 1; j < devs.size(); ++j)
                if (devs[i] == devs[j]) return fail(SR_ERR_UNSUPPORTED, "SR_GATHER_RCCL needs distinct devices (RCCL refuses two ranks on one GPU)");
        std::vector<sr::RcclComm> comms(devs.size(), nullptr);
        SR_RCCL(api, api->CommInitAll(comms.data(), (int)devs.size(), devs.data()));
        for (sr_scene* q : m->parts) { int rc = use_device(q); if (rc) return rc; rc = ensure_io_streams(q); if (rc) return rc; }
        m->comms.swap(comms);
    }
    m->gather_kind = kind;
    return SR_OK;
}

int sr_rccl_unique_id(uint8_t out[SR_RCCL_ID_BYTES]) {
    if (!out) return fail(SR_ERR_INVALID_ARG, "out is NULL");
    std::string why;
    const sr::RcclApi* api = sr::rccl_api(&why);
    if (!api) return fail(SR_ERR_UNSUPPORTED, why);
    static_assert(SR_RCCL_ID_BYTES == sr::kRcclIdBytes, "ncclUniqueId is 128 bytes");
    sr::RcclId id;
    SR_RCCL(api, api->GetUniqueId(&id));
    std::memcpy(out, id.internal, SR_RCCL_ID_BYTES);
    return SR_OK;
}

int sr_rccl_init(sr_scene* s, const uint8_t id_bytes[SR_RCCL_ID_BYTES], int32_t world, int32_t rank) {
    if (!s || !id_bytes || world < 1 || rank < 0 || rank >= world) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_rccl_init");
    if (!s->parts.empty()) return fail(SR_ERR_INVALID_ARG, "sr_rccl_init: one scene = one rank = one device (use sr_set_gather for a multi-device scene)");
    std::string why;
    const sr::RcclApi* api = sr::rccl_api(&why);
    if (!api) return fail(SR_ERR_UNSUPPORTED, why);
    int rc = use_device(s);
    if (rc) return rc;
    if (s->comm) { SR_RCCL(api, api->CommDestroy(s->comm)); s->comm = nullptr; }
    sr::RcclId id;
    std::memcpy(id.internal, id_bytes, SR_RCCL_ID_BYTES);
    SR_RCCL(api, api->CommInitRank(&s->comm, world, id, rank));
    s->rccl_world = world; s->rccl_rank = rank;
    return SR_OK;
}

int sr_rccl_gather(sr_scene* s, const sr_frame* f, const void* d_strips, void* d_full, void* hip_stream) {
    if (!s || !s->parts.empty()) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_rccl_gather");
    if (!s->comm) return fail(SR_ERR_NOT_BUILT, "sr_rccl_gather before sr_rccl_init");
    int rc = validate_frame(f, s);
    if (rc) return rc;
    const sr::RcclApi* api = sr::rccl_api(nullptr);
    if (!api) return fail(SR_ERR_UNSUPPORTED, "librccl is not loaded");
    if ((rc = use_device(s))) return rc;
    const int n = s->rccl_world, me = s->rccl_rank;
    if (me == 0 && !d_full) return fail(SR_ERR_INVALID_ARG, "rank 0 needs the full surface");
    int a, b;
    clamp_rows(f, a, b);
    if (b < a) return SR_OK;
    std::vector<size_t> counts(n, 0), off(n, 0);
    size_t total = 0;
    for (int g = 0; g < n; ++g) {
        sr_frame fg = *f;
        fg.strip_rows = kMultiStripRows; fg.strip_count = n; fg.strip_index = g;
        counts[g] = (size_t)sr_frame_pixel_count(&fg);
        if (g > 0) { off[g] = total; total += counts[g]; }
    }
    if (counts[me] && !d_strips) return fail(SR_ERR_INVALID_ARG, "this rank owns rows but passed no strip buffer");
    hipStream_t stream = (hipStream_t)hip_stream;
    if (me != 0) {
        if (counts[me] == 0) return SR_OK;
        SR_RCCL(api, api->GroupStart());
        SR_RCCL(api, api->Send(d_strips, counts[me], sr::kRcclInt32, 0, s->comm, stream));
        SR_RCCL(api, api->GroupEnd());
        return SR_OK;
    }
    SR_HIP(s->d_gather.reserve(std::max<size_t>(total, 1) * 4));
    if (n > 1) {
        SR_RCCL(api, api->GroupStart());
        for (int g = 1; g < n; ++g)
            if (counts[g]) SR_RCCL(api, api->Recv((uint32_t*)s->d_gather.p + off[g], counts[g], sr::kRcclInt32, g, s->comm, stream));
        SR_RCCL(api, api->GroupEnd());
    }
    for (int g = 0; g < n; ++g) {                                     // the row de-interleave: strided device copies behind the receives
        const std::vector<StripRun> runs = strip_runs(a, b, n, g);
        if (runs.empty() || counts[g] == 0) continue;
        const uint32_t* src = g == 0 ? (const uint32_t*)d_strips : (const uint32_t*)s->d_gather.p + off[g];
        SR_HIP(copy_runs(runs, n, f->width, src, (uint32_t*)d_full, hipMemcpyDeviceToDevice, stream));
    }
    return SR_OK;
}

int sr_rccl_render(sr_scene* s, const sr_frame* f, void* d_full, void* hip_stream) {
    if (!s || !s->parts.empty()) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_rccl_render");
    if (!s->comm) return fail(SR_ERR_NOT_BUILT, "sr_rccl_render before sr_rccl_init");
    int rc = validate_frame(f, s);
    if (rc) return rc;
    if (f->strip_count > 0) return fail(SR_ERR_INVALID_ARG, "sr_rccl_render splits the frame itself: strip_count must be 0");
    if ((f->flags & SR_F_STATIC_SHADOWS) && (f->flags & SR_F_SHADOWS)) return fail(SR_ERR_UNSUPPORTED, "static shadows need the whole frame on one device");
    if (f->flags & SR_F_AMBIENT_OCCLUSION) return fail(SR_ERR_UNSUPPORTED, "ambient occlusion needs the whole frame on one device (sr_rccl_render splits it into strips)");
    if (f->flags & SR_F_LIGHT_FIELD) return fail(SR_ERR_UNSUPPORTED, "light field needs the whole frame on one device (sr_rccl_render splits it into strips)");
    if ((rc = use_device(s))) return rc;
    sr_frame fg = *f;
    fg.strip_rows = kMultiStripRows; fg.strip_count = s->rccl_world; fg.strip_index = s->rccl_rank;
    const int64_t mine = sr_frame_pixel_count(&fg);
    if (mine > 0) {
        SR_HIP(s->d_pixels.reserve((size_t)mine * 4));
        if ((rc = sr_render_device(s, &fg, s->d_pixels.p, hip_stream, nullptr))) return rc;
    }
    return sr_rccl_gather(s, f, mine > 0 ? s->d_pixels.p : nullptr, d_full, hip_stream);
}

int sr_shade_points(sr_scene* s, const sr_frame* f, int64_t n, const double* pos, const double* normal, const uint32_t* color, uint32_t* out) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || n < 0 || (n > 0 && (!pos || !normal || !color || !out))) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_shade_points");
    int rc = validate_frame(f, s);
    if (rc) return rc;
    if ((rc = use_device(s))) return rc;
    if (n == 0) return SR_OK;
    sr::FrameConst fc;
    if ((rc = prepare_frame(s, f, fc))) return rc;
    size_t sizes[4] = {(size_t)n * 24, (size_t)n * 24, (size_t)n * 4, (size_t)n * 4};
    for (int i = 0; i < 4; ++i) SR_HIP(s->d_io[i].reserve(sizes[i]));
    SR_HIP(hipMemcpy(s->d_io[0].p, pos, sizes[0], hipMemcpyHostToDevice));
    SR_HIP(hipMemcpy(s->d_io[1].p, normal, sizes[1], hipMemcpyHostToDevice));
    SR_HIP(hipMemcpy(s->d_io[2].p, color, sizes[2], hipMemcpyHostToDevice));
    SR_HIP(sr::launch_shade_points(fc, n, (const double*)s->d_io[0].p, (const double*)s->d_io[1].p, (const uint32_t*)s->d_io[2].p, (uint32_t*)s->d_io[3].p, nullptr));
    SR_HIP(hipStreamSynchronize(nullptr));
    SR_HIP(hipMemcpy(out, s->d_io[3].p, sizes[3], hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_shade_points_device(sr_scene* s, const sr_frame* f, int64_t n, const double* d_pos, const double* d_normal, const uint32_t* d_color, uint32_t* d_out,
                           void* hip_stream) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || n < 0 || (n > 0 && (!d_pos || !d_normal || !d_color || !d_out))) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_shade_points_device");
    int rc = validate_frame(f, s);
    if (rc) return rc;
    if ((rc = use_device(s))) return rc;
    if (n == 0) return SR_OK;
    sr::FrameConst fc;
    if ((rc = prepare_frame(s, f, fc))) return rc;
    SR_HIP(sr::launch_shade_points(fc, n, d_pos, d_normal, d_color, d_out, (hipStream_t)hip_stream));
    return SR_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// The frame G-buffer (sr_render_hits): the primary stage's answer per camera sample
// ------------------------------------------------------------------------------------------------------------------
int64_t sr_frame_sample_count(const sr_frame* f) {
    if (!f || f->width <= 0 || f->height <= 0 || f->sub_pixel_res < 1) return 0;
    int a, b;
    clamp_rows(f, a, b);
    if (b < a) return 0;
    return (int64_t)(b - a + 1) * f->width * f->sub_pixel_res * f->sub_pixel_res;
}

// `fs`: the frame without the decorator switches, which the call does not read
static const BatchCall kRenderHitsCall = {
    "bad argument to sr_render_hits",
    {{SR_F_VOXELS, "sr_render_hits: voxel rendering (SR_F_VOXELS) replaces the root geometry; a voxel hit has no position or triangle"},
     {SR_F_LIGHT_FIELD, "sr_render_hits: the light field (SR_F_LIGHT_FIELD) replaces the primary stage: a cell stores a colour, not a hit"},
     {SR_F_SINGLE_KERNEL, "sr_render_hits: the one-kernel renderer (SR_F_SINGLE_KERNEL) has no primary stage to read"}},
    nullptr,
    "sr_render_hits: row strips (strip_count > 0) lay the rows out compactly; pass a row range",
    0, true};

int sr_render_hits_device(sr_scene* m, const sr_frame* f, double* d_starts, double* d_dirs, uint8_t* d_hit, double* d_ray_frac, double* d_pos, double* d_normal,
                          uint32_t* d_color, int32_t* d_tri_index, void* hip_stream, uint64_t* d_stats) {
    sr_scene* s = m;
    sr_frame fs;
    int rc = batch_call_check(kRenderHitsCall, s, f, true, fs);
    if (rc || sr_frame_sample_count(&fs) == 0) return rc;          // (an empty row range: nothing is drawn, no device is asked for)
    if ((rc = use_device(s))) return rc;
    if (m != s) m->last_parts = 1;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (d_stats) SR_HIP(hipMemsetAsync(d_stats, 0, SR_STATS_COUNT * sizeof(uint64_t), stream));
    const HitsReq req{{d_starts, d_dirs, d_hit, d_ray_frac, d_pos, d_normal, d_color, d_tri_index}};
    return render_common(s, &fs, nullptr, stream, (unsigned long long*)d_stats, &req);
}

int sr_render_hits(sr_scene* m, const sr_frame* f, double* starts, double* dirs, uint8_t* hit, double* ray_frac, double* pos, double* normal, uint32_t* color,
                   int32_t* tri_index, uint64_t stats[4]) {
    sr_scene* s = m;
    sr_frame fs;
    int rc = batch_call_check(kRenderHitsCall, s, f, true, fs);
    const int64_t n = sr_frame_sample_count(&fs);
    if (rc || n == 0) return rc;
    if ((rc = use_device(s))) return rc;
    if (m != s) m->last_parts = 1;
    Staged io[] = {{nullptr, starts, (size_t)n * 24}, {nullptr, dirs, (size_t)n * 24}, {nullptr, hit, (size_t)n}, {nullptr, ray_frac, (size_t)n * 8},
                   {nullptr, pos, (size_t)n * 24}, {nullptr, normal, (size_t)n * 24}, {nullptr, color, (size_t)n * 4}, {nullptr, tri_index, (size_t)n * 4}};
    return run_staged(m, s, io, 8, false, stats, [&](hipStream_t stream, unsigned long long* d_stats) {
        const HitsReq req{{(double*)io[0].dev, (double*)io[1].dev, (uint8_t*)io[2].dev, (double*)io[3].dev, (double*)io[4].dev, (double*)io[5].dev,
                           (uint32_t*)io[6].dev, (int32_t*)io[7].dev}};
        return render_common(s, &fs, nullptr, stream, d_stats, &req);
    });
}

// ---- sr_light_field_rays ----
// `fs`: the frame with SR_F_LIGHT_FIELD implied.  (Shadows are validate_frame's to refuse: the scene's switch decides)
static const BatchCall kLightFieldRaysCall = {
    "bad argument to sr_light_field_rays",
    {{SR_F_AMBIENT_OCCLUSION, "sr_light_field_rays: ambient occlusion (SR_F_AMBIENT_OCCLUSION) needs a surface point per ray; a cell stores a colour"},
     {SR_F_PATH_TRACING, "sr_light_field_rays: path tracing (SR_F_PATH_TRACING) needs a surface point per ray; a cell stores a colour"},
     {SR_F_VOXELS, "sr_light_field_rays: voxel rendering (SR_F_VOXELS) replaces the root geometry the canonical rays are traced through"},
     {SR_F_SINGLE_KERNEL, "sr_light_field_rays: the light field is not built into the one-kernel renderer (SR_F_SINGLE_KERNEL)"}},
    "sr_light_field_rays: mirror bounces (max_bounces > 0) need a surface point per ray; a cell stores a colour",
    "sr_light_field_rays: row strips (strip_count > 0) divide a frame's rows, not a batch of rays",
    SR_F_LIGHT_FIELD, false};
static int light_field_rays_check(sr_scene*& s, const sr_frame* f, int64_t n, const void* starts, const void* dirs, const void* out, uint32_t options, sr_frame& fs) {
    const bool args_ok = n >= 0 && (n == 0 || (starts && dirs && out)) && options == 0u;
    sr_scene* q = (s && !s->parts.empty()) ? s->parts[0] : s;
    if (q && f && args_ok && q->lf_tris)
        return fail(SR_ERR_UNSUPPORTED, "sr_light_field_rays: the triangle light field (sr_set_light_field_triangles) runs LightFieldTriMethod's three stages per ray, which is not part of this call");
    return batch_call_check(kLightFieldRaysCall, s, f, args_ok, fs);
}

int sr_light_field_rays_device(sr_scene* m, const sr_frame* f, int64_t n, const double* d_starts, const double* d_dirs, uint32_t* d_out, uint8_t* d_inside,
                               uint32_t options, void* hip_stream, uint64_t* d_filled, uint64_t* d_stats) {
    sr_scene* s = m;
    sr_frame fs;
    int rc = light_field_rays_check(s, f, n, d_starts, d_dirs, d_out, options, fs);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n == 0) return zero_generators_device(s, d_filled, stream);
    if ((rc = use_device(s))) return rc;
    if (d_stats) SR_HIP(hipMemsetAsync(d_stats, 0, SR_STATS_COUNT * sizeof(uint64_t), stream));
    if (d_filled) SR_HIP(hipMemsetAsync(d_filled, 0, sizeof(uint64_t), stream));
    const LfRaysReq req{n, d_starts, d_dirs, d_out, d_inside, (unsigned long long*)d_filled};
    return render_common(s, &fs, nullptr, stream, (unsigned long long*)d_stats, &req);
}

int sr_light_field_rays(sr_scene* m, const sr_frame* f, int64_t n, const double* starts, const double* dirs, uint32_t* out, uint8_t* inside, uint32_t options,
                        uint64_t* filled) {
    sr_scene* s = m;
    sr_frame fs;
    int rc = light_field_rays_check(s, f, n, starts, dirs, out, options, fs);
    if (rc) return rc;
    if (n == 0) { if (filled) *filled = 0; return SR_OK; }
    if ((rc = use_device(s))) return rc;
    uint64_t made = 0;
    Staged io[] = {{starts, nullptr, (size_t)n * 24}, {dirs, nullptr, (size_t)n * 24}, {nullptr, out, (size_t)n * 4}, {nullptr, inside, (size_t)n},
                   {nullptr, &made, sizeof(uint64_t)}};
    rc = run_staged(m, s, io, 5, false, nullptr, [&](hipStream_t stream, unsigned long long* d_stats) {
        SR_HIP(hipMemsetAsync(io[4].dev, 0, sizeof(uint64_t), stream));
        const LfRaysReq req{n, (const double*)io[0].dev, (const double*)io[1].dev, (uint32_t*)io[2].dev, (uint8_t*)io[3].dev, (unsigned long long*)io[4].dev};
        return render_common(s, &fs, nullptr, stream, d_stats, &req);
    });
    if (!rc && filled) *filled = made;
    return rc;
}

// ---- sr_shadow_points ----
// `fs`: the frame with SR_F_SHADOWS implied
static const BatchCall kShadowPointsCall = {
    "bad argument to sr_shadow_points",
    {{SR_F_STATIC_SHADOWS, "sr_shadow_points: static shadows (SR_F_STATIC_SHADOWS) are a cache over a frame's fill order, not a step on a point"},
     {SR_F_AMBIENT_OCCLUSION, "sr_shadow_points: ambient occlusion (SR_F_AMBIENT_OCCLUSION) is another decorator, not ShadowMethod's step"},
     {SR_F_PATH_TRACING, "sr_shadow_points: path tracing (SR_F_PATH_TRACING) replaces the decorator chain ShadowMethod is part of"},
     {SR_F_VOXELS, "sr_shadow_points: voxel rendering (SR_F_VOXELS) has no shadow step"},
     {SR_F_LIGHT_FIELD, "sr_shadow_points: the light field (SR_F_LIGHT_FIELD) stores colours of canonical rays, not of a caller's points"},
     {SR_F_SINGLE_KERNEL, "sr_shadow_points: the one-kernel renderer (SR_F_SINGLE_KERNEL) has no stage to enter"}},
    "sr_shadow_points: mirror bounces (max_bounces > 0) belong to a camera ray, not to a point",
    "sr_shadow_points: row strips (strip_count > 0) divide a frame's rows, not a batch of points",
    SR_F_SHADOWS, false};
static int shadow_points_check(sr_scene*& s, const sr_frame* f, int64_t n, const void* pos, const void* normal, const void* out, uint32_t options, sr_frame& fs) {
    const bool args_ok = n >= 0 && (n == 0 || (pos && normal && out)) && !(options & ~(uint32_t)SR_POINTS_COHERENT);
    return batch_call_check(kShadowPointsCall, s, f, args_ok, fs);
}

int sr_shadow_points_device(sr_scene* m, const sr_frame* f, int64_t n, const double* d_pos, const double* d_normal, const uint32_t* d_color, uint32_t* d_out,
                            uint32_t options, void* hip_stream, uint64_t* d_stats) {
    sr_scene* s = m;
    sr_frame fs;
    int rc = shadow_points_check(s, f, n, d_pos, d_normal, d_out, options, fs);
    if (rc || n == 0) return rc;
    if ((rc = use_device(s))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (d_stats) SR_HIP(hipMemsetAsync(d_stats, 0, SR_STATS_COUNT * sizeof(uint64_t), stream));
    const PtsReq req{n, d_pos, d_normal, d_color, d_out, (options & SR_POINTS_COHERENT) != 0};
    return render_common(s, &fs, nullptr, stream, (unsigned long long*)d_stats, &req);
}

int sr_shadow_points(sr_scene* m, const sr_frame* f, int64_t n, const double* pos, const double* normal, const uint32_t* color, uint32_t* out, uint32_t options) {
    sr_scene* s = m;
    sr_frame fs;
    int rc = shadow_points_check(s, f, n, pos, normal, out, options, fs);
    if (rc || n == 0) return rc;
    if ((rc = use_device(s))) return rc;
    // (the colours are modulated where they lie: the device variant's `out` aliasing `color`)
    Staged io[] = {{pos, nullptr, (size_t)n * 24}, {normal, nullptr, (size_t)n * 24}, {color, out, (size_t)n * 4}};
    return run_staged(m, s, io, 3, false, nullptr, [&](hipStream_t stream, unsigned long long* d_stats) {
        const PtsReq req{n, (const double*)io[0].dev, (const double*)io[1].dev, color ? (const uint32_t*)io[2].dev : nullptr, (uint32_t*)io[2].dev,
                         (options & SR_POINTS_COHERENT) != 0};
        return render_common(s, &fs, nullptr, stream, d_stats, &req);
    });
}

// ---- sr_static_shadow_points ----
// `fs`: the frame with SR_F_SHADOWS | SR_F_STATIC_SHADOWS implied (a multi-device scene: the cache lives on the first part)
static const BatchCall kStaticShadowPointsCall = {
    "bad argument to sr_static_shadow_points",
    {{SR_F_AMBIENT_OCCLUSION, "sr_static_shadow_points: ambient occlusion (SR_F_AMBIENT_OCCLUSION) is another decorator, not ShadowMethod's step"},
     {SR_F_PATH_TRACING, "sr_static_shadow_points: path tracing (SR_F_PATH_TRACING) replaces the decorator chain ShadowMethod is part of"},
     {SR_F_VOXELS, "sr_static_shadow_points: voxel rendering (SR_F_VOXELS) has no shadow step"},
     {SR_F_LIGHT_FIELD, "sr_static_shadow_points: the light field (SR_F_LIGHT_FIELD) stores colours of canonical rays, not of a caller's points"},
     {SR_F_SINGLE_KERNEL, "sr_static_shadow_points: the one-kernel renderer (SR_F_SINGLE_KERNEL) has no stage to enter"}},
    "sr_static_shadow_points: mirror bounces (max_bounces > 0) belong to a camera ray, not to a point",
    "sr_static_shadow_points: row strips (strip_count > 0) divide a frame's rows, not a batch of points",
    SR_F_SHADOWS | SR_F_STATIC_SHADOWS, false};
static int static_shadow_points_check(sr_scene*& s, const sr_frame* f, int64_t n, const void* pos, const void* normal, const void* out, const void* amount,
                                      uint32_t options, sr_frame& fs) {
    const bool args_ok = n >= 0 && (n == 0 || (pos && normal && (out || amount))) && !(options & ~(uint32_t)SR_POINTS_COHERENT);
    return batch_call_check(kStaticShadowPointsCall, s, f, args_ok, fs);
}

int sr_static_shadow_points_device(sr_scene* m, const sr_frame* f, int64_t n, const double* d_pos, const double* d_normal, const uint32_t* d_color, uint32_t* d_out,
                                   uint8_t* d_amount, uint32_t options, void* hip_stream, uint64_t* d_generators, uint64_t* d_stats) {
    sr_scene* s = m;
    sr_frame fs;
    int rc = static_shadow_points_check(s, f, n, d_pos, d_normal, d_out, d_amount, options, fs);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n == 0) return zero_generators_device(s, d_generators, stream);
    if ((rc = use_device(s))) return rc;
    if (d_stats) SR_HIP(hipMemsetAsync(d_stats, 0, SR_STATS_COUNT * sizeof(uint64_t), stream));
    if (d_generators) SR_HIP(hipMemsetAsync(d_generators, 0, sizeof(uint64_t), stream));
    const PtsReq req{n, d_pos, d_normal, d_color, d_out, (options & SR_POINTS_COHERENT) != 0, true, d_amount, (unsigned long long*)d_generators};
    return render_common(s, &fs, nullptr, stream, (unsigned long long*)d_stats, &req);
}

int sr_static_shadow_points(sr_scene* m, const sr_frame* f, int64_t n, const double* pos, const double* normal, const uint32_t* color, uint32_t* out, uint8_t* amount,
                            uint32_t options, uint64_t* generators) {
    sr_scene* s = m;
    sr_frame fs;
    int rc = static_shadow_points_check(s, f, n, pos, normal, out, amount, options, fs);
    if (rc) return rc;
    if (n == 0) { if (generators) *generators = 0; return SR_OK; }
    if ((rc = use_device(s))) return rc;
    // (the colours are modulated where they lie: the device variant's `out` aliasing `color`)
    uint64_t made = 0;
    Staged io[] = {{pos, nullptr, (size_t)n * 24}, {normal, nullptr, (size_t)n * 24}, {color, out, (size_t)n * 4}, {nullptr, amount, (size_t)n},
                   {nullptr, &made, sizeof(uint64_t)}};
    rc = run_staged(m, s, io, 5, false, nullptr, [&](hipStream_t stream, unsigned long long* d_stats) {
        SR_HIP(hipMemsetAsync(io[4].dev, 0, sizeof(uint64_t), stream));
        const PtsReq req{n, (const double*)io[0].dev, (const double*)io[1].dev, color ? (const uint32_t*)io[2].dev : nullptr,
                         out ? (uint32_t*)io[2].dev : nullptr, (options & SR_POINTS_COHERENT) != 0, true, (uint8_t*)io[3].dev, (unsigned long long*)io[4].dev};
        return render_common(s, &fs, nullptr, stream, d_stats, &req);
    });
    if (!rc && generators) *generators = made;
    return rc;
}

// ---- sr_ao_points ----
const uint64_t kAoPointsMaxGenerators = 1ull << 40;
// `fs`: the frame with SR_F_AMBIENT_OCCLUSION implied
static const BatchCall kAoPointsCall = {
    "bad argument to sr_ao_points",
    {{SR_F_STATIC_SHADOWS, "sr_ao_points: static shadows (SR_F_STATIC_SHADOWS) are another decorator's cache, not AmbientOcclusionMethod's step"},
     {SR_F_PATH_TRACING, "sr_ao_points: path tracing (SR_F_PATH_TRACING) replaces the decorator chain AmbientOcclusionMethod is part of"},
     {SR_F_VOXELS, "sr_ao_points: voxel rendering (SR_F_VOXELS) has no occlusion step"},
     {SR_F_LIGHT_FIELD, "sr_ao_points: the light field (SR_F_LIGHT_FIELD) stores colours of canonical rays, not of a caller's points"},
     {SR_F_SINGLE_KERNEL, "sr_ao_points: the one-kernel renderer (SR_F_SINGLE_KERNEL) has no stage to enter"}},
    "sr_ao_points: mirror bounces (max_bounces > 0) belong to a camera ray, not to a point",
    "sr_ao_points: row strips (strip_count > 0) divide a frame's rows, not a batch of points",
    SR_F_AMBIENT_OCCLUSION, false};
static int ao_points_check(sr_scene*& s, const sr_frame* f, int64_t n, const void* pos, const void* normal, const void* out, const void* amount,
                           uint64_t first_generator, uint32_t options, sr_frame& fs) {
    const bool args_ok = n >= 0 && (n == 0 || (pos && normal && (out || amount))) && options == 0 && first_generator <= kAoPointsMaxGenerators &&
                         (uint64_t)n <= kAoPointsMaxGenerators - first_generator;
    return batch_call_check(kAoPointsCall, s, f, args_ok, fs);
}

// the jump coefficients of the table kernels' chunk strides (k_aop_states), uploaded once per scene
static int ensure_aop_rows(sr_scene* s) {
    if (s->aop_rows_ready) return SR_OK;
    // entry [j][i] = coefficient j of x^(stride + i): the 55 lanes of a product read consecutive words
    std::vector<uint32_t> rows((size_t)2 * 55 * 55), t((size_t)55 * 55);
    const uint64_t strides[2] = {64ull * 300ull, 64ull * 64ull * 300ull};
    for (int k = 0; k < 2; ++k) {
        sr::net_jump_rows(strides[k], t.data());
        for (int i = 0; i < 55; ++i)
            for (int j = 0; j < 55; ++j) rows[(size_t)k * 55 * 55 + (size_t)j * 55 + i] = t[(size_t)i * 55 + j];
    }
    SR_HIP(s->d_aop_rows.upload(rows));
    s->aop_rows_ready = true;
    return SR_OK;
}

struct AoPtsReq { int64_t n; const double* pos; const double* nrm; const uint32_t* color; uint32_t* out; uint8_t* amount; uint64_t first_generator; unsigned long long* generators; };

// the passes of one call, enqueued on `stream` (device arrays): ordered like a frame, on the first scratch set
static int ao_points_common(sr_scene* s, const sr_frame* f, const AoPtsReq& q, hipStream_t stream, unsigned long long* d_stats) {
    int rc = sync_geometry(s, (uint32_t)f->trace_mode);
    if (rc) return rc;
    const bool cached = !(f->flags & SR_F_AO_UNCACHED);
    sr::AoPointsLaunch L{};
    bool host_table = s->dbg[SR_DBG_KERNEL_SWITCH] == 44;
    if (!host_table && !sr::net_random_window(f->random_seed, L.window.s)) host_table = true;   // (not the recurrence for this seed: sr_host.h)
    if (!host_table && (rc = ensure_aop_rows(s))) return rc;
    // ---- ordered like a frame (render_common) ----
    StreamOrder order(s, stream);
    if (order.entered) return order.entered;
    if (s->pre_ready_set) SR_HIP(hipStreamWaitEvent(stream, s->pre_ready, 0));      // the records' order, written on another stream perhaps
    if (cached) {
        SR_HIP(s->d_ao_cache.reserve(kAoCells));
        SR_HIP(s->d_ao_claim.reserve(kAoCells * 8));
        if (s->ao_cache_empty) {
            SR_HIP(hipMemsetAsync(s->d_ao_cache.p, 0, kAoCells, stream));
            s->ao_cache_empty = false;
        }
    }
    const int64_t want = s->dbg[SR_DBG_BAND_SAMPLES] > 0 ? std::min<int64_t>(s->dbg[SR_DBG_BAND_SAMPLES], sr::kAopMaxPass) : sr::kAopMaxPass;
    const int64_t pass = std::max<int64_t>(1, std::min<int64_t>(want, q.n));
    if ((rc = ensure_num_cus(s))) return rc;
    sr_scene::BandScratch& B = s->scratch[0];                        // (sr_debug_counters keeps describing the last frame: the call has no queue counters)
    const size_t slots = (size_t)(pass + 255) / 256 * 256;
    SR_HIP(B.hits.reserve(slots * sr::pipeline_hit_record_bytes()));
    SR_HIP(B.hits2.reserve(slots * sr::pipeline_hit_record_bytes()));
    SR_HIP(B.pt_flags.reserve(slots));
    SR_HIP(B.pt_index.reserve(slots * 4));
    SR_HIP(B.pt_totals.reserve((slots / (size_t)sr::pipeline_pt_chunk() + 2) * 4));
    SR_HIP(B.ao_escapes.reserve(slots * 4));
    SR_HIP(s->d_aop_table.reserve(sr::ao_points_table_bytes(pass)));
    SR_HIP(s->d_aop_state.reserve(512));
    L.sc = dev_scene(s);
    L.mode = f->trace_mode;
    L.n = q.n; L.pass = pass;
    L.pos = q.pos; L.nrm = q.nrm; L.color = q.color; L.out = q.out; L.amount = q.amount;
    L.first_generator = q.first_generator;
    L.cache = cached ? (uint8_t*)s->d_ao_cache.p : nullptr;
    L.claim = cached ? (unsigned long long*)s->d_ao_claim.p : nullptr;
    L.recs = B.hits.p; L.gen = B.hits2.p;
    L.flags = (uint8_t*)B.pt_flags.p; L.index = (uint32_t*)B.pt_index.p; L.totals = (uint32_t*)B.pt_totals.p;
    L.escapes = (uint32_t*)B.ao_escapes.p;
    L.table = (int32_t*)s->d_aop_table.p;
    L.stride_rows = (const uint32_t*)s->d_aop_rows.p;
    L.running = (unsigned long long*)s->d_aop_state.p;
    L.base_window = (int32_t*)((char*)s->d_aop_state.p + 256);
    L.generators_out = q.generators;
    L.nearest_walks = s->dbg[SR_DBG_KERNEL_SWITCH] == 34;
    L.stats = (f->flags & SR_F_PRIMARY_STATS_ONLY) ? nullptr : d_stats;
    L.persistent_blocks = s->num_cus * 8;
    L.stream = stream;
    L.user = s;
    L.get_events = timing_events;
    if (host_table) {
        start_host_table(s, f->random_seed, q.first_generator, 300);   // from the call's first generator on
        L.host_table = fill_host_table;
    }
    const hipError_t pe = sr::launch_ao_points(L);
    s->aop_host_random.reset();
    SR_HIP(pe);
    return SR_OK;
}

int sr_ao_points_device(sr_scene* m, const sr_frame* f, int64_t n, const double* d_pos, const double* d_normal, const uint32_t* d_color, uint32_t* d_out,
                        uint8_t* d_amount, uint64_t first_generator, uint32_t options, void* hip_stream, uint64_t* d_generators, uint64_t* d_stats) {
    sr_scene* s = m;
    sr_frame fs;
    int rc = ao_points_check(s, f, n, d_pos, d_normal, d_out, d_amount, first_generator, options, fs);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n == 0) return zero_generators_device(s, d_generators, stream);
    if ((rc = use_device(s))) return rc;
    if (d_stats) SR_HIP(hipMemsetAsync(d_stats, 0, SR_STATS_COUNT * sizeof(uint64_t), stream));
    const AoPtsReq req{n, d_pos, d_normal, d_color, d_out, d_amount, first_generator, (unsigned long long*)d_generators};
    return ao_points_common(s, &fs, req, stream, (unsigned long long*)d_stats);
}

int sr_ao_points(sr_scene* m, const sr_frame* f, int64_t n, const double* pos, const double* normal, const uint32_t* color, uint32_t* out, uint8_t* amount,
                 uint64_t first_generator, uint32_t options, uint64_t* generators) {
    sr_scene* s = m;
    sr_frame fs;
    int rc = ao_points_check(s, f, n, pos, normal, out, amount, first_generator, options, fs);
    if (rc) return rc;
    if (n == 0) { if (generators) *generators = 0; return SR_OK; }
    if ((rc = use_device(s))) return rc;
    // (the colours are modulated where they lie: the device variant's `out` aliasing `color`)
    uint64_t made = 0;
    Staged io[] = {{pos, nullptr, (size_t)n * 24}, {normal, nullptr, (size_t)n * 24}, {color, out, (size_t)n * 4}, {nullptr, amount, (size_t)n},
                   {nullptr, &made, sizeof(uint64_t)}};
    rc = run_staged(m, s, io, 5, false, nullptr, [&](hipStream_t stream, unsigned long long* d_stats) {
        const AoPtsReq req{n, (const double*)io[0].dev, (const double*)io[1].dev, color ? (const uint32_t*)io[2].dev : nullptr,
                           out ? (uint32_t*)io[2].dev : nullptr, (uint8_t*)io[3].dev, first_generator, (unsigned long long*)io[4].dev};
        return ao_points_common(s, &fs, req, stream, d_stats);
    });
    if (!rc && generators) *generators = made;
    return rc;
}

// ---- sr_path_points ----
const uint64_t kPathPointsMaxSamples = 1ull << 40;
const uint64_t kPathPointsHostTableSamples = 1ull << 30;     // ... where the host makes the table: it draws its way there
// `fs`: the frame with SR_F_PATH_TRACING implied
static const BatchCall kPathPointsCall = {
    "bad argument to sr_path_points",
    {{SR_F_SHADOWS, "sr_path_points: shadows (SR_F_SHADOWS, dynamic or static) are ShadowMethod's step, which follows this one: sr_shadow_points"},
     {SR_F_AMBIENT_OCCLUSION, "sr_path_points: ambient occlusion (SR_F_AMBIENT_OCCLUSION) is AmbientOcclusionMethod's step, which follows this one: sr_ao_points"},
     {SR_F_VOXELS, "sr_path_points: voxel rendering (SR_F_VOXELS) has no surface point to bounce from"},
     {SR_F_LIGHT_FIELD, "sr_path_points: the light field (SR_F_LIGHT_FIELD) stores colours of canonical rays, not of a caller's points"},
     {SR_F_SINGLE_KERNEL, "sr_path_points: the one-kernel renderer (SR_F_SINGLE_KERNEL) has no stage to enter"}},
    "sr_path_points: mirror bounces (max_bounces > 0) belong to a camera ray, not to a point",
    "sr_path_points: row strips (strip_count > 0) divide a frame's rows, not a batch of points",
    SR_F_PATH_TRACING, false};
static int path_points_check(sr_scene*& s, const sr_frame* f, int64_t n, const void* pos, const void* normal, const void* out, const void* incoming,
                             const void* dirs, uint64_t first_sample, uint32_t options, sr_frame& fs) {
    const bool args_ok = n >= 0 && (n == 0 || (pos && normal && (out || incoming || dirs))) && options == 0 && first_sample <= kPathPointsMaxSamples &&
                         (uint64_t)n <= kPathPointsMaxSamples - first_sample;
    return batch_call_check(kPathPointsCall, s, f, args_ok, fs);
}

struct PathPtsReq { int64_t n; const double* pos; const double* nrm; const uint32_t* color; uint32_t* out; uint32_t* incoming; double* dirs; uint64_t first_sample; };

// the passes of one call, enqueued on `stream` (device arrays): ordered like a frame, on the first scratch set
static int path_points_common(sr_scene* s, const sr_frame* f, const PathPtsReq& q, hipStream_t stream, unsigned long long* d_stats) {
    int rc = sync_geometry(s, (uint32_t)f->trace_mode);
    if (rc) return rc;
    sr::PathPointsLaunch L{};
    if ((rc = prepare_frame(s, f, L.fc))) return rc;
    const bool trace = q.out || q.incoming;
    const bool walked = trace && f->trace_mode == SR_MODE_BVH;
    const int64_t want = s->dbg[SR_DBG_BAND_SAMPLES] > 0 ? std::min<int64_t>(s->dbg[SR_DBG_BAND_SAMPLES], sr::kPpMaxPass) : sr::kPpMaxPass;
    const int64_t pass = std::max<int64_t>(1, std::min<int64_t>(want, q.n));
    // the window every pass starts from, by the jump-ahead: the host knows where each pass lies in the sequence
    int32_t window[sr::kNetWindow];
    bool host_table = s->dbg[SR_DBG_KERNEL_SWITCH] == 45;
    if (!host_table && !sr::net_random_window(f->random_seed, window)) host_table = true;   // (not the recurrence for this seed: sr_host.h)
    // (the host walks through every draw before the call's: a path for cross-checks, with a limit -- about ten seconds of drawing)
    if (host_table && q.first_sample + (uint64_t)q.n > kPathPointsHostTableSamples)
        return fail(SR_ERR_UNSUPPORTED, "sr_path_points: the draw table made on the host (SR_DBG_KERNEL_SWITCH 45, or a seed the jump-ahead does not cover) is limited to first_sample + n <= 2^30");
    std::vector<sr::NetState> windows;
    if (!host_table) {
        if ((rc = ensure_aop_rows(s))) return rc;
        windows.resize((size_t)((q.n + pass - 1) / pass));
        for (size_t p = 0; p < windows.size(); ++p) {
            uint32_t c[sr::kNetLag];
            sr::net_jump_poly(3ull * (q.first_sample + (uint64_t)p * (uint64_t)pass), c);
            sr::net_jump_apply(window, c, windows[p].s);
        }
    }
    // ---- ordered like a frame (render_common) ----
    StreamOrder order(s, stream);
    if (order.entered) return order.entered;
    if (s->pre_ready_set) SR_HIP(hipStreamWaitEvent(stream, s->pre_ready, 0));      // the records' order, written on another stream perhaps
    if ((rc = ensure_num_cus(s))) return rc;
    sr_scene::BandScratch& B = s->scratch[0];                        // (sr_debug_counters keeps describing the last frame: the call has counters of its own)
    const size_t slots = (size_t)(pass + 255) / 256 * 256;
    if (trace) SR_HIP(B.hits2.reserve(slots * sr::pipeline_hit_record_bytes()));
    if (walked) {
        // the scratch of a SR_MODE_BVH frame's second rays (render_common)
        SR_HIP(B.bounce_prep.reserve(slots * 64));
        SR_HIP(B.bounce_res.reserve(slots * 16));
        const long long deep = std::max(3 * (long long)s->b4_depth + 2, (long long)s->bvh.depth + 2) - sr::pipeline_bounce_lds_levels();
        if (deep > 0) SR_HIP(B.bounce_stack.reserve((size_t)deep * (size_t)s->num_cus * 8 * 256 * 4));
        SR_HIP(B.ray_sort.reserve(slots * 4 * 4));
        SR_HIP(B.ray_sort_temp.reserve(sr::ray_sort_temp_bytes((unsigned)pass)));
    }
    SR_HIP(s->d_aop_table.reserve(sr::path_points_table_bytes(pass)));
    SR_HIP(s->d_pp_state.reserve(512));
    L.sc = dev_scene(s);
    L.mode = f->trace_mode;
    L.n = q.n; L.pass = pass;
    L.pos = q.pos; L.nrm = q.nrm; L.color = q.color; L.out = q.out; L.incoming = q.incoming; L.dirs = q.dirs;
    L.first_sample = q.first_sample;
    L.rays = trace ? B.hits2.p : nullptr;
    L.table = (int32_t*)s->d_aop_table.p;
    L.windows = host_table ? nullptr : windows.data();
    L.stride_rows = (const uint32_t*)s->d_aop_rows.p;
    L.base_window = (int32_t*)s->d_pp_state.p;
    L.pass_units = (uint32_t*)((char*)s->d_pp_state.p + 256);
    L.counters = (unsigned int*)((char*)s->d_pp_state.p + 272);
    L.ray_sort_buf = walked ? (unsigned int*)B.ray_sort.p : nullptr;
    L.ray_sort_temp = walked ? B.ray_sort_temp.p : nullptr;
    L.ray_sort_temp_bytes = walked ? sr::ray_sort_temp_bytes((unsigned)pass) : 0;
    L.bounce_prep = walked ? B.bounce_prep.p : nullptr;
    L.bounce_res = walked ? B.bounce_res.p : nullptr;
    L.bounce_stack = walked ? (int32_t*)B.bounce_stack.p : nullptr;
    L.bounce_stack_bytes = walked ? B.bounce_stack.cap : 0;
    L.bvh2_packets = s->dbg[SR_DBG_BVH2_PACKETS] > 0;
    L.stats = (f->flags & SR_F_PRIMARY_STATS_ONLY) ? nullptr : d_stats;
    L.persistent_blocks = s->num_cus * 8;
    L.stream = stream;
    L.user = s;
    L.get_events = timing_events;
    if (host_table) {
        start_host_table(s, f->random_seed, q.first_sample, 3);         // from the call's first sample on
        L.host_table = fill_host_table;
    }
    const hipError_t pe = sr::launch_path_points(L);
    s->aop_host_random.reset();
    SR_HIP(pe);
    return SR_OK;
}

int sr_path_points_device(sr_scene* m, const sr_frame* f, int64_t n, const double* d_pos, const double* d_normal, const uint32_t* d_color, uint32_t* d_out,
                          uint32_t* d_incoming, double* d_dirs, uint64_t first_sample, uint32_t options, void* hip_stream, uint64_t* d_stats) {
    sr_scene* s = m;
    sr_frame fs;
    int rc = path_points_check(s, f, n, d_pos, d_normal, d_out, d_incoming, d_dirs, first_sample, options, fs);
    if (rc) return rc;
    if (n == 0) return SR_OK;
    if ((rc = use_device(s))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (d_stats) SR_HIP(hipMemsetAsync(d_stats, 0, SR_STATS_COUNT * sizeof(uint64_t), stream));
    const PathPtsReq req{n, d_pos, d_normal, d_color, d_out, d_incoming, d_dirs, first_sample};
    return path_points_common(s, &fs, req, stream, (unsigned long long*)d_stats);
}

int sr_path_points(sr_scene* m, const sr_frame* f, int64_t n, const double* pos, const double* normal, const uint32_t* color, uint32_t* out,
                   uint32_t* incoming, double* dirs, uint64_t first_sample, uint32_t options) {
    sr_scene* s = m;
    sr_frame fs;
    int rc = path_points_check(s, f, n, pos, normal, out, incoming, dirs, first_sample, options, fs);
    if (rc) return rc;
    if (n == 0) return SR_OK;
    if ((rc = use_device(s))) return rc;
    // (the colours are finished where they lie: the device variant's `out` aliasing `color`)
    Staged io[] = {{pos, nullptr, (size_t)n * 24}, {normal, nullptr, (size_t)n * 24}, {color, out, (size_t)n * 4}, {nullptr, incoming, (size_t)n * 4},
                   {nullptr, dirs, (size_t)n * 24}};
    return run_staged(m, s, io, 5, false, nullptr, [&](hipStream_t stream, unsigned long long* d_stats) {
        const PathPtsReq req{n, (const double*)io[0].dev, (const double*)io[1].dev, color ? (const uint32_t*)io[2].dev : nullptr,
                             out ? (uint32_t*)io[2].dev : nullptr, (uint32_t*)io[3].dev, (double*)io[4].dev, first_sample};
        return path_points_common(s, &fs, req, stream, d_stats);
    });
}

int sr_net_random_jump(int32_t seed, uint64_t skip, int32_t out[55]) {
    if (!out) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_net_random_jump");
    int32_t w[sr::kNetWindow];
    if (!sr::net_random_window(seed, w)) return fail(SR_ERR_UNSUPPORTED, "sr_net_random_jump: one of the seed's first 55 outputs lies outside [0, 2^31 - 2]");
    uint32_t c[sr::kNetLag];
    sr::net_jump_poly(skip, c);
    sr::net_jump_apply(w, c, out);
    return SR_OK;
}

void sr_instance_matrices(const double position[3], double yaw, double pitch, double roll, double transform[12], double inv_transform[12]) {
    sr::instance_matrices(position, yaw, pitch, roll, transform, inv_transform);
}
double sr_default_fov_depth(void) { return sr::default_fov_depth(); }
void sr_area_light_offsets(int32_t seed, int32_t count, double* out3) { sr::area_light_offsets(seed, count, out3); }

int sr_load_3ds(sr_scene* s, const uint8_t* data, size_t len) {
    if (!s || !data) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_load_3ds");
    sr::LoadedModel m;
    std::string err = sr::load_3ds(data, len, m);
    if (!err.empty()) return fail(SR_ERR_FORMAT, err);
    return sr_set_triangles(s, m.v9.data(), m.argb.data(), (int64_t)m.argb.size(), m.bmin, m.bmax);
}
int64_t sr_num_triangles(const sr_scene* s) { if (s && !s->parts.empty()) s = s->parts[0]; return s ? (int64_t)s->ntris : 0; }
int sr_get_triangles(const sr_scene* s, double* v9, uint32_t* argb, double box_min[3], double box_max[3]) {
    if (s && !s->parts.empty()) s = s->parts[0];
    if (!s || !s->have_model) return fail(SR_ERR_NO_MODEL, "no model");
    if (v9 || argb) { int rc = ensure_host_model(const_cast<sr_scene*>(s)); if (rc) return rc; }
    if (v9) std::memcpy(v9, s->v9.data(), s->v9.size() * sizeof(double));
    if (argb) std::memcpy(argb, s->argb.data(), s->argb.size() * sizeof(uint32_t));
    for (int a = 0; a < 3; ++a) { if (box_min) box_min[a] = s->bmin[a]; if (box_max) box_max[a] = s->bmax[a]; }
    return SR_OK;
}

int sr_last_ray_stats(const sr_scene* s, uint64_t out[SR_STATS_COUNT]) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "bad argument");
    std::memcpy(out, s->last_stats, sizeof(s->last_stats));
    return SR_OK;
}

void sr_make_random_triangles(int32_t seed, int64_t n, double space, double extent, double origin, int32_t opaque,
                              double* v9, uint32_t* argb) {
    sr::NetRandom rnd(seed);
    for (int64_t i = 0; i < n; ++i) {
        double* p = v9 + 9 * i;
        for (int a = 0; a < 3; ++a) p[a] = rnd.next_double() * space + origin;          // v1 = MakeRandomVector(space)
        for (int a = 0; a < 3; ++a) p[3 + a] = p[a] + rnd.next_double() * extent;       // v2 = v1 + MakeRandomVector(extent)
        for (int a = 0; a < 3; ++a) p[6 + a] = p[a] + rnd.next_double() * extent;       // v3 = v1 + MakeRandomVector(extent)
        uint32_t c = (uint32_t)rnd.next();                                              // (uint)random.Next()
        argb[i] = opaque ? (0xFF000000u | (c & 0xFFFFFFu)) : c;
    }
}

void sr_net_random_doubles(int32_t seed, int64_t skip, int64_t n, double* out) {
    sr::NetRandom rnd(seed);
    for (int64_t i = 0; i < skip; ++i) (void)rnd.next();           // Next() and NextDouble() both consume one sample
    for (int64_t i = 0; i < n; ++i) out[i] = rnd.next_double();
}

// ---- surface passes, Renderer.cs:765-767 ----
int sr_post_process_device(sr_scene* s, void* d_pixels, int64_t count, int32_t style, uint32_t background_color, void* hip_stream) {
    if (s && !s->parts.empty()) s = s->parts[0];               // surface passes / timings: the first device
    if (!s || count < 0 || (count > 0 && !d_pixels)) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_post_process");
    if (style < SR_STYLE_STANDARD || style > SR_STYLE_DEPTH_BANDED)
        return fail(SR_ERR_UNSUPPORTED, "render style " + std::to_string(style) + " is not a per-pixel colour function (Style.Normals needs the rasteriser's depth buffer)");
    int rc = use_device(s);
    if (rc) return rc;
    if (style == SR_STYLE_STANDARD || count == 0) return SR_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    hipEvent_t e0, e1;
    if ((rc = next_events(s, sr::K_POST, e0, e1))) return rc;
    if (e0) SR_HIP(hipEventRecord(e0, stream));
    SR_HIP(sr::launch_post_process((uint32_t*)d_pixels, count, style, background_color, s->num_cus, stream));
    if (e1) SR_HIP(hipEventRecord(e1, stream));
    return SR_OK;
}

int sr_post_process(sr_scene* s, int32_t* pixels, int64_t count, int32_t style, uint32_t background_color) {
    if (s && !s->parts.empty()) s = s->parts[0];               // surface passes / timings: the first device
    if (!s || count < 0 || (count > 0 && !pixels)) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_post_process");
    if (style < SR_STYLE_STANDARD || style > SR_STYLE_DEPTH_BANDED)
        return fail(SR_ERR_UNSUPPORTED, "render style " + std::to_string(style) + " is not a per-pixel colour function (Style.Normals needs the rasteriser's depth buffer)");
    int rc = use_device(s);
    if (rc) return rc;
    if (style == SR_STYLE_STANDARD || count == 0) return SR_OK;
    SR_HIP(s->d_pixels.reserve((size_t)count * 4));
    SR_HIP(hipMemcpy(s->d_pixels.p, pixels, (size_t)count * 4, hipMemcpyHostToDevice));
    if ((rc = sr_post_process_device(s, s->d_pixels.p, count, style, background_color, nullptr))) return rc;
    SR_HIP(hipMemcpy(pixels, s->d_pixels.p, (size_t)count * 4, hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_anti_alias_device(sr_scene* s, const void* d_src, int32_t dst_width, int32_t dst_height, int32_t resolution, void* d_dst, void* hip_stream) {
    if (s && !s->parts.empty()) s = s->parts[0];               // surface passes / timings: the first device
    if (!s || !d_src || !d_dst || dst_width <= 0 || dst_height <= 0) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_anti_alias");
    if (resolution < 1 || resolution > 64 || (int64_t)dst_width * resolution > INT_MAX || (int64_t)dst_height * resolution > INT_MAX)
        return fail(SR_ERR_INVALID_ARG, "AntiAliasResolution must be in 1..64");           // Renderer.cs:374 (> 0)
    int rc = use_device(s);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    hipEvent_t e0, e1;
    if ((rc = next_events(s, sr::K_ANTI_ALIAS, e0, e1))) return rc;
    if (e0) SR_HIP(hipEventRecord(e0, stream));
    SR_HIP(sr::launch_anti_alias((const uint32_t*)d_src, (uint32_t*)d_dst, dst_width, dst_height, resolution, stream));
    if (e1) SR_HIP(hipEventRecord(e1, stream));
    return SR_OK;
}

int sr_anti_alias(sr_scene* s, const int32_t* src, int32_t dst_width, int32_t dst_height, int32_t resolution, int32_t* dst) {
    if (s && !s->parts.empty()) s = s->parts[0];               // surface passes / timings: the first device
    if (!s || !src || !dst || dst_width <= 0 || dst_height <= 0) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_anti_alias");
    if (resolution < 1 || resolution > 64 || (int64_t)dst_width * resolution > INT_MAX || (int64_t)dst_height * resolution > INT_MAX)
        return fail(SR_ERR_INVALID_ARG, "AntiAliasResolution must be in 1..64");
    int rc = use_device(s);
    if (rc) return rc;
    const size_t dst_bytes = (size_t)dst_width * dst_height * 4;
    const size_t src_bytes = dst_bytes * resolution * resolution;
    SR_HIP(s->d_pixels.reserve(src_bytes));
    SR_HIP(s->d_aa.reserve(dst_bytes));
    SR_HIP(hipMemcpy(s->d_pixels.p, src, src_bytes, hipMemcpyHostToDevice));
    if ((rc = sr_anti_alias_device(s, s->d_pixels.p, dst_width, dst_height, resolution, s->d_aa.p, nullptr))) return rc;
    SR_HIP(hipMemcpy(dst, s->d_aa.p, dst_bytes, hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_debug_counters(sr_scene* s, uint32_t out[8]) {
    if (s && !s->parts.empty() && out) {
        for (int i = 0; i < 8; ++i) out[i] = 0;
        for (sr_scene* q : s->parts) {                              // (the known-axes masks of slot 5 are or-ed, the rest summed)
            uint32_t c[8]; int rc = sr_debug_counters(q, c); if (rc) return rc;
            for (int i = 0; i < 8; ++i) out[i] = i == 5 ? (out[i] | c[i]) : out[i] + c[i];
        }
        return SR_OK;
    }
    /* diagnostics: the pipeline's device counters after the last band of the last frame:
       hit_count, k_shadow work head, fallback_count, fallback work head */
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "bad argument");
    int rc = use_device(s);
    if (rc) return rc;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    SR_HIP(hipDeviceSynchronize());
    for (auto& sc : s->scratch) {                                   // every part-frame pipeline of the last frame (last band of each)
        if (!sc.counters.p || !sc.used_last_frame) continue;
        uint32_t c[8];
        SR_HIP(hipMemcpy(c, sc.counters.p, 32, hipMemcpyDeviceToHost));
        for (int i = 0; i < 5; ++i) out[i] += c[i];
    }
    for (int i = 0; i < 3; ++i) out[5 + i] = s->dbg_frame[i];      // host bookkeeping of the last frame (include/softray.h)
    return SR_OK;
}

int sr_debug_set(sr_scene* s, int32_t key, int64_t value) {
    if (s && !s->parts.empty()) { for (sr_scene* q : s->parts) { int rc = sr_debug_set(q, key, value); if (rc) return rc; } return SR_OK; }
    if (!s || key < 0 || key >= SR_DBG_COUNT) return fail(SR_ERR_INVALID_ARG, "bad argument to sr_debug_set");
    s->dbg[key] = value;
    return SR_OK;
}

void sr_reset_kernel_times(sr_scene* s) {
    if (!s) return;
    if (!s->parts.empty()) { for (sr_scene* q : s->parts) sr_reset_kernel_times(q); return; }
    for (int k = 0; k < sr::K_COUNT; ++k) s->ev_used[k] = 0;
}

int sr_kernel_times(sr_scene* s, sr_kernel_time* out, int32_t cap) {
    if (s && !s->parts.empty()) s = s->parts[0];               // surface passes / timings: the first device
    if (!s || !out || cap <= 0) return 0;
    if (use_device(s)) return 0;
    int n = 0;
    for (int k = 0; k < sr::K_COUNT && n < cap; ++k) {
        if (!s->ev_used[k]) continue;
        double total = 0;
        int ok = 0;
        for (int i = 0; i < s->ev_used[k]; ++i) {
            if (hipEventSynchronize(s->ev[k][2 * i + 1]) != hipSuccess) continue;
            float ms = 0;
            if (hipEventElapsedTime(&ms, s->ev[k][2 * i], s->ev[k][2 * i + 1]) != hipSuccess) continue;
            total += ms;
            ++ok;
        }
        if (!ok) continue;
        out[n].name = sr::kernel_name(k);
        out[n].ms = (float)total;
        out[n].launches = ok;
        ++n;
    }
    return n;
}

}  // extern "C"
