/*
 * softray.h -- C ABI of libsoftray_hip.so: the MI355X (gfx950) implementation of Engine3D's
 * per-pixel raytrace hot path (voidstar69/softray: Engine3D/Raytrace/ + the raytrace half of
 * Engine3D/Renderer.cs).
 *
 * The reference has NO native/FFI boundary (pure C#, single process).  The seam is cut
 * where the reference fans out to worker tasks:
 *
 *     Renderer.RaytraceBlock(instance, geometry, left, top, sizeX, sizeY)      Engine3D/Renderer.cs:1690
 *
 * Everything RaytraceBlock and the decorators below it read is passed in `sr_frame`; everything
 * PreCalculate() builds once per model is held in `sr_scene`.  A C# `[DllImport("softray_hip")]`
 * shim inside a Renderer-compatible class binds exactly these entry points
 * (bindings/csharp/GpuRenderer.cs); so do the ctypes mirror (softray_amd/) and the
 * C++ mirror (softray_amd/host/).
 *
 * Conventions: plain pointers and sizes only; every call is blocking unless it takes a stream; all
 * input arrays are copied; the library never retains a caller pointer after returning; a scene is
 * single-threaded like the reference ("Must only be executed by a single thread at a time",
 * Renderer.cs:1498), distinct scenes are independent.  Return value 0 = ok, <0 = SR_ERR_*;
 * sr_last_error() gives the thread-local message the shim wraps into the matching .NET exception.
 * There is NO CPU fallback: without a usable HIP device every compute call fails with
 * SR_ERR_NO_DEVICE.
 */
#ifndef SOFTRAY_H
#define SOFTRAY_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SR_ABI_VERSION 5
#define SR_STATS_COUNT 24   /* entries of the ray-statistics array (sr_last_ray_stats, sr_render_device's d_stats) */

enum {
    SR_OK                 =  0,
    SR_ERR_INVALID_ARG    = -1,   /* ArgumentException / ArgumentNullException                         */
    SR_ERR_OUT_OF_RANGE   = -2,   /* ArgumentOutOfRangeException: "A triangle vertex is outside the
                                     bounding box" (SpatialSubdivision.cs:287-295)                      */
    SR_ERR_NO_MODEL       = -3,   /* no triangles set: Renderer.Render() returns silently
                                     (Renderer.cs:736-739); the shim does the same                      */
    SR_ERR_NOT_BUILT      = -4,   /* sr_build() not called for the requested trace mode                */
    SR_ERR_UNSUPPORTED    = -5,
    SR_ERR_NO_DEVICE      = -6,   /* no HIP device / host-only scene: compute is refused, never emulated */
    SR_ERR_HIP            = -7,   /* a HIP runtime call failed (message in sr_last_error)               */
    SR_ERR_FORMAT         = -8    /* FormatException (3DS loader, ThreeDSFile.cs:166-169, Model.cs:553) */
};

/* per-frame flags = the public bool fields of Renderer (Renderer.cs:56-57,76-77,84) */
enum {
    SR_F_SHADING     = 1u << 0,   /* rayTraceShading  -> ShadingMethod.Enabled  (Renderer.cs:1614)      */
    SR_F_SHADOWS     = 1u << 1,   /* rayTraceShadows (dynamic) -> ShadowMethod.Enabled (:1632)          */
    SR_F_FOCAL_BLUR  = 1u << 2,   /* rayTraceFocalBlur (only read when sub_pixel_res > 1, :1744-1790)   */
    SR_F_POINT_LIGHT = 1u << 3,   /* pointLighting   (Scene.cs:20)                                      */
    SR_F_SPECULAR    = 1u << 4,   /* specularLighting (Scene.cs:21)                                     */
    SR_F_STATIC_SHADOWS = 1u << 5, /* rayTraceShadowsStatic, with SR_F_SHADOWS (ShadowMethod.cs:75-83,103-108): the light
                                     fraction of a surface point is (byte)(fraction*254+1) looked up in a 128^3 texture over
                                     the unit cube; an empty cell is generated for whoever asks first and then kept by the
                                     scene for later frames (sr_reset_shadow_cache = a new Renderer).  The reference's worker
                                     tasks race for the cells; the library uses the deterministic order that reproduces the
                                     reference's goldens (RendererTests.RaytraceStaticShadow): the `concurrency` row blocks
                                     advance in lock step -- row r of every block, blocks ascending, before row r + 1;
                                     columns ascending; sub-samples in loop order.  Needs the whole frame in one call:
                                     SR_ERR_UNSUPPORTED with strips, mirror bounces or SR_F_SINGLE_KERNEL            */
    SR_F_PATH_TRACING = 1u << 6,  /* rayTracePathTracing -> PathTracingMethod.Enabled (Renderer.cs:1613-1618, PathTracingMethod.cs):
                                     every camera sample that hits fires ONE second ray in a random direction of the hemisphere
                                     about its normal, from pos + n * 0.001 through the same geometry, and stores
                                     incoming * (n . d) + own colour (normalised when a channel exceeds 1.0).  The direction is made
                                     of three NextDouble() of Random(random_seed); the reference restarts that sequence for every
                                     one of its `concurrency` row blocks (Renderer.cs:1655-1666) and draws in scan order (row,
                                     column, subX, subY) for the samples that hit, so sample number k (counting hits only) of a
                                     block uses draws 3k .. 3k + 2: the library finds k with a segmented prefix sum over the hit
                                     flags and looks the draws up in a table the scene keeps per (seed, length) -- 12 bytes per
                                     sample of the largest row block, SR_ERR_UNSUPPORTED above 256 MiB.  Reads random_seed and
                                     concurrency.  SR_ERR_UNSUPPORTED together with SR_F_SHADOWS (dynamic or static),
                                     max_bounces > 0 and SR_F_SINGLE_KERNEL.  A multi-device scene splits the frame like any other: its
                                     parts exchange the hit counts of their rows between the primary pass and the second rays, and
                                     the row blocks stay those of the whole row range.  Caller-made strips (strip_count > 1, also
                                     through sr_rccl_render) stay SR_ERR_UNSUPPORTED: one call on one scene cannot know how many
                                     samples hit in the rows the other ranks render */
    SR_F_VOXELS      = 1u << 7,   /* rayTraceVoxels (Renderer.cs:1568-1588): rootGeometry = the model as an N^3 VoxelGrid (N = sr_set_voxel_res, default 64) instead of the model's tree AND
                                     the extra geometry (both ignored); the decorators above it stay.  A ray is clipped to the box (-1,-1,-1)..(1,1,1),
                                     scaled to grid coordinates (p = (p * 0.5 + 0.5) * ((double)N - 0.001)) and walked in fixed steps of 0.1 along its longest axis (VoxelGrid.cs:125-177,
                                     LineWalker3D.cs:17-35); the first non-empty cell is the hit: its colour (the average of the colours of the triangles
                                     whose box of cells holds it) and the normal of its lowest-index triangle, pos = (0,0,0), rayFrac = 0.  Ignores
                                     trace_mode and needs no sr_build, only triangles: the first such frame calls sr_build_voxels.  Works with
                                     SR_F_SHADING, the lights, sub_pixel_res, SR_F_FOCAL_BLUR, row ranges, strips, multi-device scenes and
                                     sr_rccl_render.  Statistics: one ray and one geometry test per camera sample, no nodes, no leaves.
                                     SR_ERR_UNSUPPORTED together with SR_F_SHADOWS (dynamic or static), SR_F_PATH_TRACING, max_bounces > 0 and
                                     SR_F_SINGLE_KERNEL: the reference's result there is an artefact of rayFrac = 0 that nothing pins */
    SR_F_SINGLE_KERNEL = 1u << 8, /* library option, not a Renderer field: trace the frame with the one-kernel
                                     renderer (k_render) instead of the k_primary/k_shadow/k_resolve pipeline.
                                     Pixels are identical; kept as an independent cross-check               */
    SR_F_NO_SPLIT    = 1u << 10,  /* library option: run the frame as ONE pipeline on the caller's stream instead of two
                                     halves on two internal streams (the default: the latency-bound tail kernels of one
                                     half overlap the other half's work, -5 % frame time).  Same pixels; used to time
                                     kernels that do not share the GPU with another kernel                       */
    SR_F_PER_LANE_SHADOWS = 1u << 9, /* library option: trace shadow samples one lane per hit point (k_shadow)
                                     instead of one wavefront per hit point with a shared shaft walk
                                     (k_shadow_packet).  Pixels are identical; cross-check                  */
    SR_F_LITERAL_SECONDARY = 1u << 11, /* library option: a SR_MODE_REF_TREE frame traces its SHADOW rays through the reference tree
                                     too.  By default (own BVH built, point light, <= 1024 samples) they are answered on the
                                     library's BVH (shaft path): "is there a hit with rayFrac <= 1.0" has the same answer, and the
                                     four statistics of sr_render count the primary rays, which keep the literal traversal either
                                     way.  With the flag the secondary counters of sr_last_ray_stats are the reference tree's  */
    SR_F_AMBIENT_OCCLUSION = 1u << 13, /* rayTraceAmbientOcclusion -> AmbientOcclusionMethod.Enabled (Renderer.cs:1631-1638, AmbientOcclusionMethod.cs:65-99,
                                     AmbientOcclusion.cs:101-230): after shading and (dynamic) shadows, the colour of every camera sample that hits the root
                                     geometry is modulated with a byte 1..255 = (byte)(escapes / 100.0 * 254 + 1), where `escapes` counts the probes, out of
                                     100 fired from pos + n * 0.001 into the hemisphere about the normal, that hit nothing or hit beyond rayFrac 2.0.  pos is
                                     the surface point CLAMPED to the cube [-0.5, 0.5]^3 (extra geometry outside it probes from the cube's surface: literal
                                     reference behaviour).  A probe direction is (2u0 - 1, 2u1 - 1, 2u2 - 1), not normalised, negated when it points below the
                                     surface; the u are NextDouble() of Random(random_seed), which the reference restarts for every one of its `concurrency`
                                     row blocks and draws in scan order (row, column, subX, subY): generator number k of a block uses draws 300 k .. 300 k + 299,
                                     looked up in the table path tracing uses (kept per (seed, length): 1200 bytes per generator of the row block that has the
                                     most, SR_ERR_UNSUPPORTED above 256 MiB).  The byte lives in a 128^3 texture over the unit cube that the scene keeps for
                                     later frames (sr_reset_ao_cache = a new Renderer; sr_get_ao_cache / sr_set_ao_cache = the reference's .ao file): an empty
                                     cell is generated by whoever asks first.  The reference's worker tasks race for the cells; the library takes the
                                     deterministic order of SR_F_STATIC_SHADOWS -- row r of every block, blocks ascending, before row r + 1; columns ascending;
                                     sub-samples in loop order -- and a generator's k is the number of generators before it in scan order inside its own block.
                                     With concurrency = 1 that IS the reference's frame; with more blocks the order is the library's and no golden pins it
                                     (the reference's own tests switch AO off for that reason, RendererTests.cs:402-405), as with the mirror-bounce extension.
                                     Reads random_seed and concurrency.  Works with SR_F_SHADING, SR_F_SHADOWS (dynamic), sub_pixel_res, SR_F_FOCAL_BLUR, row
                                     ranges, extra geometry and all three trace modes.  The frame runs as one pipeline (as with SR_F_NO_SPLIT) and the call
                                     waits for the device once, also sr_render_device: the host sizes the table by the generators found.  A multi-device
                                     scene renders it on devices[0] alone.  SR_ERR_UNSUPPORTED together with SR_F_PATH_TRACING (same Random), SR_F_VOXELS (a
                                     voxel hit has no position), SR_F_STATIC_SHADOWS with SR_F_SHADOWS (the probes would fill that cache), max_bounces > 0,
                                     SR_F_SINGLE_KERNEL, caller-made strips (strip_count > 0), sr_rccl_render, and a row range that does not fit one row band.
                                     Statistics: the probes are secondary rays -- sr_last_ray_stats [4] grows by 100 per generator, [5..7] by what their walks
                                     count (not with SR_F_PRIMARY_STATS_ONLY); [0..3] are unchanged                                     */
    SR_F_AO_UNCACHED = 1u << 14,  /* with SR_F_AMBIENT_OCCLUSION only: AmbientOcclusionMethod.EnableCache = false (Renderer.cs:74) -- every hit sample
                                     generates its own byte, nothing is read from or stored in the cache                                */
    SR_F_LIGHT_FIELD = 1u << 15,  /* rayTraceLightField with LightFieldStoresTriangles = false -> LightFieldColorMethod.Enabled (Renderer.cs:1640-1649,
                                     LightFieldColorMethod.cs:92-217, LightField4D.cs:175-206, 253-273, 304-344, Sphere.cs:69-142): the colour of a camera sample is
                                     the entry of a 4-D table of 4 N^4 uint32 (N = sr_set_light_field_res, default 64) that its line falls into.  In model space,
                                     with R = 0.866 about the origin: d = dir * (1.0 / |dir|), proj = start . d, term = proj * proj - start . start + R * R;
                                     term < 1e-10 is the background colour (nothing checks whether the start lies inside the sphere).  Otherwise the two
                                     points start + d * (-proj -/+ sqrt(term)) give h = atan2(x, z), w = asin(y / R) (not clamped) and the coordinates
                                     u = h1 / pi * 0.5 + 0.5, v = w1 / pi + 0.5, s, t likewise; the cell is ((byte)(u * (2N - 1)), (byte)(v * (N - 1)),
                                     (byte)(s * (2N - 1)), (byte)(t * (N - 1))) (a NaN coordinate counts as 0) and the entry's index u * N*N*N*2 + v * N*N*2 +
                                     s * N + t.  A non-zero entry is the sample's colour.  An empty (0) entry is filled first: the cell's CANONICAL ray, from
                                     the centre of patch (u, v) towards the centre of patch (s, t) -- P(i, j) = (sin H cos W R, sin W R, cos H cos W R) with
                                     H = ((i + 0.5) / (2N - 1) - 0.5) 2 pi, W = ((j + 0.5) / (N - 1) - 0.5) pi, tabulated on the host -- is traced through the
                                     frame's root geometry (extra geometry + the model in trace_mode), shaded with SR_F_SHADING, and its colour (the
                                     background on a miss; 0 is stored as 1) is stored.  Within a frame the colour of a cell depends on the cell alone, so the result
                                     does not depend on which sample fills it or in which order (a later frame reads what an earlier one stored, shaded with
                                     the earlier frame's pose and lights, as in the reference); no camera ray touches geometry.  The table lives in the scene for later
                                     frames (sr_reset_light_field = a new Renderer; sr_get_light_field / sr_set_light_field = the reference's .cache file).
                                     Everything before atan2 / asin is exact FP64 in the reference's operand order; the two angles are the device
                                     library's, so a sample whose scaled coordinate lies within an ulp or so of an integer may fall into the neighbouring cell.
                                     Works with SR_F_SHADING, the lights, sub_pixel_res, SR_F_FOCAL_BLUR, row ranges, extra geometry, all three trace modes,
                                     host- and device-built BVH and frames of more than one row band.  The frame runs as one pipeline (as with SR_F_NO_SPLIT);
                                     a multi-device scene renders it on devices[0] alone.  SR_ERR_UNSUPPORTED together with SR_F_SHADOWS (static always; dynamic unless sr_set_light_field_shadows),
                                     SR_F_AMBIENT_OCCLUSION, SR_F_PATH_TRACING, SR_F_VOXELS, max_bounces > 0, SR_F_SINGLE_KERNEL, strip_count > 0 and
                                     sr_rccl_render.  LightFieldStoresTriangles = true (LightFieldTriMethod) is an opt-in per scene: sr_set_light_field_triangles.  Quad-linear interpolation
                                     (LightFieldColorMethod.Interpolate, hard-wired false in the reference) is an opt-in per scene: sr_set_light_field_interpolation.
                                     Statistics: stats[0] = the camera samples, [1..3] = 0; sr_last_ray_stats [4] grows by one per filled cell, [5..7] by what
                                     the canonical rays' walks count (not with SR_F_PRIMARY_STATS_ONLY)                                  */
    SR_F_PRIMARY_STATS_ONLY = 1u << 12 /* library option: with `stats`, count the primary rays only -- the four statistics of sr_render
                                     (NumRaysFired, NumGeometryTests, NumNodeVisits, NumLeafNodeVisits).  The shadow stage then runs
                                     its uncounted kernels (counting costs atomics per hit point: obj.3DS 1024^2 + shadows 2.3 -> 1.1 ms)
                                     and entries 4.. of sr_last_ray_stats read 0.  What the hosts' Render() sets             */
};

/* how the model's triangles are intersected */
enum {
    SR_MODE_REF_TREE = 0,  /* SpatialSubdivision.IntersectRay, literal (rayTraceSubdivision = true);
                              same tree, same near/far order, same leaf-box containment rule            */
    SR_MODE_BRUTE    = 1,  /* GeometryCollection over geometry_simple (rayTraceSubdivision = false)     */
    SR_MODE_BVH      = 2   /* the library's own BVH: global nearest hit with the reference's per-triangle
                              arithmetic (same root-box clip, same rayFrac offset, hit must lie inside the
                              root box, ties -> lowest triangle index).  Identical to REF_TREE except for
                              hits closer than 1e-10 to a leaf-box face of the reference tree            */
};

/* ExtraGeometryToRaytrace element (Renderer.cs:460,1545-1549).  Order is preserved: the collection is
 * scanned first-to-last with a strict '<' on rayFrac (GeometryCollection.cs:44-69), then the model. */
typedef struct {
    int32_t  kind;      /* 0 Sphere {centre xyz, radius}          Raytrace/Sphere.cs:26-33
                           1 Plane  {point xyz, normal xyz}       Raytrace/Plane.cs:22-29
                           2 Triangle {v1, v2, v3}                Raytrace/Triangle.cs:29-57
                           3 Plane as the object holds it {Plane.Normal xyz (unit), Plane.DistanceToOrigin}
                             (Plane.cs:40-62): what a host passes for an EXISTING Plane -- kind 1 would
                             normalise and project again and could differ in the last bit
                           4 AxisAlignedBox {min xyz, max xyz} (AxisAlignedBox.cs:15-28, IntersectRay :60-95):
                             the nearest of its six one-sided planes' hits that lies on the box; the hit
                             carries the plane's colour (Color.White, Plane.cs:28): argb is not read;
                             NumRayTests = 6                                                            */
    uint32_t argb;      /* Color.ToARGB() of the primitive's Color                                      */
    double   p[9];
} sr_prim;

/* Everything RaytraceGeometry / RaytraceBlock / ShadingMethod / ShadowMethod read per frame
 * (Renderer.cs:1501-1829).  The host side (C# shim, C++ or ctypes mirror) fills it from the public
 * Renderer / Instance fields; the matrices are Instance.InitRender's (Instance.cs:134-135) so that the
 * host's own sin/cos are the ones used.  sr_instance_matrices() builds them for hosts that want it. */
typedef struct {
    int32_t  width, height;          /* SetRenderingSurface (Renderer.cs:593)                            */
    int32_t  start_row, end_row;     /* rayTraceStartRow / rayTraceEndRow, inclusive (:135-136,1652-1653)
                                        rendered EXACTLY (the reference's last task may overshoot by up to
                                        rayTraceConcurrency-1 rows, :1659-1670; those rows are identical) */
    int32_t  sub_pixel_res;          /* rayTraceSubPixelRes (:90)                                        */
    uint32_t background_argb;        /* BackgroundColor (:308); misses store it with alpha 0xFF (:1860)  */
    uint32_t flags;                  /* SR_F_*                                                           */
    int32_t  random_seed;            /* rayTraceRandomSeed (:92): area-light offsets, ShadowMethod.cs:63 */
    int32_t  shadow_samples;         /* 0 => 100 = softShadowQuality (ShadowMethod.cs:9). 1 with a zero
                                        offset table = hard-shadow variant (build-defined, unpinned)      */
    int32_t  trace_mode;             /* SR_MODE_*                                                        */
    int32_t  strip_rows, strip_count, strip_index;
                                     /* multi-GPU row interleave: this call renders rows r in
                                        [start_row,end_row] with (r / strip_rows) % strip_count ==
                                        strip_index into a COMPACT buffer (owned rows in order).
                                        strip_count == 0: off, pixels is the full W*H surface            */
    int32_t  max_bounces;            /* 0 = the reference.  1..16: EXTENSION for config 5 (no reference counterpart,
                                        parity unpinned): mirror bounces r = dir - n*(2 dir.n) from pos + n*0.001,
                                        each level coloured by the same shading/shadow chain, colours blended per
                                        channel ((s*(255-k))>>8) + ((r*k)>>8), k = (byte)(reflectivity*255)       */
    int32_t  concurrency;            /* rayTraceConcurrency (:92), <= 0 => 4.  Only read with SR_F_STATIC_SHADOWS (it fixes
                                        the order in which the shadow cache is filled, see that flag), with
                                        SR_F_PATH_TRACING (the row blocks that each restart the random sequence) and with
                                        SR_F_AMBIENT_OCCLUSION (both)                                                */
    int32_t  reserved0;              /* 0 */
    double   transform[12];          /* rows 0..2 of Instance._transform        (Instance.cs:134)        */
    double   inv_transform[12];      /* rows 0..2 of Instance._inverseTransform (Instance.cs:135)        */
    double   position_z;             /* Instance.Position.z (:1717, Instance.cs:182)                     */
    double   fov_depth;              /* Renderer.fieldOfViewDepth = 0.5 / tan(pi/8) (:101)               */
    double   focal_depth;            /* rayTraceFocalDepth (:87)                                         */
    double   focal_blur_strength;    /* rayTraceFocalBlurStrength (:88)                                  */
    double   ambient, shininess;     /* ambientLight_intensity, specularLight_shininess (:38,:41)        */
    double   light_dir_view[3];      /* directionalLight_dir (:39)                                       */
    double   light_pos_view[3];      /* positionalLight_pos (:40)                                        */
    double   reflectivity;           /* 0..1, only read when max_bounces > 0                              */
    const double* area_light_offsets;/* optional [shadow_samples][3] (e.g. produced by the C# shim with the
                                        real System.Random); NULL => derived from random_seed             */
} sr_frame;

/* Layout contract of the two structs that cross the boundary by value / by reference (x86-64 SysV and Windows x64 agree): the
 * C# shim mirrors it with [StructLayout(LayoutKind.Sequential)] (bindings/csharp/GpuRenderer.cs carries the same offsets
 * as comments), softray_amd/_lib.py with ctypes; tests/test_abi.py checks the three against each other. */
#ifdef __cplusplus
#define SR_LAYOUT_ASSERT(cond, msg) static_assert(cond, msg)
#else
#define SR_LAYOUT_ASSERT(cond, msg) _Static_assert(cond, msg)
#endif
SR_LAYOUT_ASSERT(sizeof(sr_prim) == 80, "sr_prim is 80 bytes: kind@0 argb@4 p@8");
SR_LAYOUT_ASSERT(offsetof(sr_prim, p) == 8, "sr_prim.p@8");
SR_LAYOUT_ASSERT(sizeof(sr_frame) == 368, "sr_frame is 368 bytes");
SR_LAYOUT_ASSERT(offsetof(sr_frame, flags) == 24 && offsetof(sr_frame, trace_mode) == 36 && offsetof(sr_frame, strip_rows) == 40 &&
                 offsetof(sr_frame, max_bounces) == 52 && offsetof(sr_frame, concurrency) == 56, "sr_frame int block");
SR_LAYOUT_ASSERT(offsetof(sr_frame, transform) == 64 && offsetof(sr_frame, inv_transform) == 160 && offsetof(sr_frame, position_z) == 256 &&
                 offsetof(sr_frame, fov_depth) == 264 && offsetof(sr_frame, focal_depth) == 272 && offsetof(sr_frame, ambient) == 288 &&
                 offsetof(sr_frame, light_dir_view) == 304 && offsetof(sr_frame, light_pos_view) == 328 &&
                 offsetof(sr_frame, reflectivity) == 352 && offsetof(sr_frame, area_light_offsets) == 360, "sr_frame double block");

typedef struct sr_scene sr_scene;    /* one per Renderer; freed by Dispose() (Renderer.cs:236)           */

/* device >= 0: HIP device ordinal.  device == -1: host-only scene (sr_set_*, sr_build, sr_tree_stats,
 * sr_load_3ds work; every compute call returns SR_ERR_NO_DEVICE). */
int  sr_create(int32_t device, sr_scene** out);
/* One scene over n HIP devices of this process (SURVEY 8b `sr_create(device_count, ...)`, 8e): the model and its trees are
 * replicated (sr_set_* / sr_build / sr_load_3ds act on every device; host builds run once), sr_render / sr_render_device split
 * the frame's rows into interleaved 16-row strips -- device g renders the strips s with s % n == g, all devices concurrently --
 * and the strips are copied straight into the caller's surface (device -> host over each device's own link, or peer-to-peer over
 * xGMI into the device surface, which lives on devices[0]).  The pixels do not depend on n (no reduction, no RNG).  This is
 * how a single-process host -- the C# Renderer -- uses a whole node.  Frames that need one global order (SR_F_STATIC_SHADOWS)
 * or that already carry strip_* fields are rendered by devices[0] alone (sr_last_frame_parts tells).  The same ordinal may appear more than once. */
int  sr_create_multi(const int32_t* devices, int32_t n, sr_scene** out);
int32_t sr_device_count(const sr_scene*);
/* How many parts (devices) rendered rows of the scene's last frame: 1 for a single-device scene and for a frame that devices[0]
 * rendered whole (static shadows, ambient occlusion, light field, caller-made strips), otherwise the number of parts that owned at least one row of the range. */
int32_t sr_last_frame_parts(const sr_scene*);
void sr_destroy(sr_scene*);

/* MakeRayTracableGeometry_simple (Renderer.cs:1452-1469): v9 = [n][3 vertices][xyz] in model space
 * (after Model.PostProcessGeometry), argb[n] = Surface.PackColorAndAlpha(diffuse, 1.0) (:1463),
 * box = AxisAlignedBox(model.Min, model.Max) (:1487).  TriangleIndex = position in the array (:1465).
 * The box may lie anywhere and need not be the vertex bounds: frames are the reference's bit for bit while |box centre| <= 1e6 x the
 * box's largest extent (beyond that the noise of the reference's FP64 arithmetic on absolute coordinates is no longer covered by the
 * margins of the fp32 shadow classification; tests/test_gpu_placement.py renders at 6e4 and at 2.5e5).
 * The features the reference defines over the unit cube assume the normalised model of Model.PostProcessGeometry (box [-0.5, 0.5]^3
 * about the origin): the static-shadow and ambient-occlusion caches, the light field's 0.866 sphere and the voxel grid's k / N - 0.5 planes. */
int  sr_set_triangles(sr_scene*, const double* v9, const uint32_t* argb, int64_t n,
                      const double box_min[3], const double box_max[3]);
/* The same from DEVICE memory: d_v9 and d_argb are arrays on the scene's device (of a multi-device scene: on devices[0]; every part
 * copies them to its own device), box_min / box_max are host arrays.  The arrays are COPIED (the library keeps no caller pointer) and the
 * triangle records and the bounds of the vertices are computed by kernels (k_tri_records: the very text sr_set_triangles compiles for the
 * host, so the records agree bit for bit), enqueued on `hip_stream` behind what is there and behind a frame of the scene in flight on
 * any stream, which keeps the old geometry.  The call waits for the stream ONCE (it reads the six doubles of the bounds back) and makes no
 * host copy of the geometry: that is made only when something needs the host arrays (sr_get_triangles, the reference-tree build, the
 * host's SAH build, i.e. SR_BUILD_ON_HOST or n <= 64).  Everything sr_set_triangles drops is dropped: the trees (frames answer
 * SR_ERR_NOT_BUILT until the next sr_build), the static-shadow, AO and light-field caches, the voxel grid.
 * Only frames and bakes are ordered for the caller: a sr_trace_rays_device batch of this scene still in flight on ANOTHER stream is the
 * caller's to order before this call (as before sr_build).  A HIP error after the kernels were enqueued leaves the scene without a model
 * (SR_ERR_NO_MODEL until the next set), every part of a multi-device scene alike.
 * d_argb == NULL: every triangle keeps its colour (a mesh that only moves; a model that sr_set_triangles / sr_load_3ds has not
 * uploaded yet is uploaded first); allowed only when n == sr_num_triangles(scene) and the scene has a model, SR_ERR_INVALID_ARG
 * otherwise (n == 0 needs neither array, as in sr_set_triangles).  n < 0, d_v9 == NULL with n > 0, a NULL box and n > 0x7fffff00 are
 * SR_ERR_INVALID_ARG too, and the arguments are checked before the device is looked at: a host-only scene then answers
 * SR_ERR_NO_DEVICE.  A mesh that keeps its triangle count and only moves can keep its tree: sr_refit_triangles_device, below. */
int  sr_set_triangles_device(sr_scene*, const double* d_v9, const uint32_t* d_argb, int64_t n,
                             const double box_min[3], const double box_max[3], void* hip_stream);
/* New vertices for a mesh that only MOVES, without a new build: the scene's own BVH -- built on the device -- is REFIT.  Arguments and
 * conventions are those of sr_set_triangles_device (the arrays are copied, everything runs on `hip_stream` behind a frame of the scene in
 * flight on any stream, one host wait for the six doubles of the vertex bounds, d_argb == NULL keeps the colours), and so is everything
 * that is dropped -- the reference tree (SR_MODE_REF_TREE answers SR_ERR_NOT_BUILT until the next sr_build), the static-shadow, AO and
 * light-field caches, the voxel grid, the host arrays -- EXCEPT the own BVH: its topology, leaf order and node numbering stay, and
 * everything in it that describes geometry is re-made by kernels from the new vertices and the new box: the leaf-order records and shaft
 * records, the fp32 boxes of the binary and of the four-wide nodes (bottom-up, by the build's own rounding), and the per-origin /
 * per-light records of the next frame.  Afterwards SR_MODE_BVH frames and ray batches answer exactly as after sr_set_triangles_device +
 * sr_build(1 << SR_MODE_BVH): pixels never depend on the tree.  sr_bvh_stats and sr_wide_tree_stats are unchanged.
 * A REFIT TREE IS ONLY AS GOOD AS THE BUILD IT CAME FROM.  The tree keeps the neighbourhoods of the vertices it was built for: after a
 * large deformation the boxes of its nodes overlap and frames get slower -- never wrong.  The library does not measure that and never
 * rebuilds by itself: the caller decides when to call sr_set_triangles_device + sr_build (or just sr_build) again.
 * Refused before anything is enqueued, the scene untouched, in this order: bad arguments (as sr_set_triangles_device) SR_ERR_INVALID_ARG;
 * a host-only scene SR_ERR_NO_DEVICE; n != sr_num_triangles(scene) SR_ERR_INVALID_ARG (a change of topology is sr_set_triangles_device +
 * sr_build); no model SR_ERR_NO_MODEL; no own BVH (never built, dropped by a set, refused by sr_build) SR_ERR_NOT_BUILT; an own BVH the
 * HOST built (SR_BUILD_ON_HOST, or n <= 64) SR_ERR_UNSUPPORTED -- its host copy of the nodes and sr_bvh_digest would go stale: rebuild.
 * A HIP error after the first kernel was enqueued leaves the scene without a model, every part of a multi-device scene alike; a
 * multi-device scene forwards to its parts with the peer copy sr_set_triangles_device makes. */
int  sr_refit_triangles_device(sr_scene*, const double* d_v9, const uint32_t* d_argb, int64_t n,
                               const double box_min[3], const double box_max[3], void* hip_stream);
/* ExtraGeometryToRaytrace (Renderer.cs:460); n == 0 clears */
int  sr_set_extra_geometry(sr_scene*, const sr_prim* prims, int32_t n);

/* PreCalculate() (Renderer.cs:673-699).  modes = bit mask (1 << SR_MODE_*) of the structures to build:
 * REF_TREE: new SpatialSubdivision(geom, box, max_depth, max_per_leaf) (SpatialSubdivision.cs:267-315;
 * <=0 => the defaults 15 / 25, :269-270; SR_ERR_OUT_OF_RANGE if a vertex is outside the box);
 * BVH: the library's own BVH; BRUTE needs nothing.  Host work + H2D copies.
 * The traversal stacks live in LDS, one entry per tree level: an own BVH deeper than 62 levels (a pathological scene, e.g. a chain of
 * triangles that halve in size towards one point; 10 M well-spread triangles give about 30) is refused with SR_ERR_UNSUPPORTED.  A
 * refused build of the own BVH leaves the scene with NO own BVH, whatever an earlier sr_build had made (the device build has
 * overwritten the old tree's buffers by then, and a scene never mixes two trees): sr_bvh_stats, sr_bvh_digest, sr_wide_tree_stats and
 * SR_MODE_BVH frames / rays answer SR_ERR_NOT_BUILT, a SR_MODE_REF_TREE frame traces its shadow rays through the reference tree as on
 * a scene that never built the BVH, SR_MODE_BRUTE and the reference tree are untouched (a REF_TREE asked for in the same call has been
 * built).  Every part of a multi-device scene ends up in that state.  A later accepted sr_build works as on a fresh scene. */
int  sr_build(sr_scene*, uint32_t modes, int32_t max_depth, int32_t max_per_leaf);
/* Where the library's own BVH is built.  Default (a scene with a device, more than 64 triangles): ON THE GPU -- Morton-ordered LBVH
 * (sr_lbvh.hip) collapsed to the four-wide form the packet walks traverse, 0.01 s for 1 M and 0.08 s for 10 M triangles (host
 * binned SAH: 0.2 s / 1.2 s); frames are within 2 % of the host tree's (the packet walks order a node's children per frame by
 * their distance from the camera / the light, which is what the Morton order lacked).  Pixels do not depend on the tree (the
 * traversal is exact for any conservative BVH).  SR_BUILD_ON_HOST (OR-ed into `modes`) asks for the host's binned-SAH builder;
 * SR_BUILD_ON_DEVICE insists on the device (SR_ERR_NO_DEVICE for a host-only scene). */
#define SR_BUILD_ON_DEVICE 0x100u
#define SR_BUILD_ON_HOST   0x200u
/* TriMeshToVoxelGrid.Convert(triangles, N, grid) (TriMeshToVoxelGrid.cs:14-114; N = sr_set_voxel_res, default 64 = Renderer.cs:1570): the voxel grid
 * SR_F_VOXELS frames and SR_TARGET_VOXELS walk, made from the triangles in index order.  Cell (x,y,z) spans [k/N - 0.5, (k+1)/N - 0.5] per axis
 * (each plane a division, then a subtraction, in FP64: TriMeshToVoxelGrid.cs:28-29); a triangle is in
 * every cell of the box of cells its vertex ranges touch; a cell's colour is the average of its triangles' colours (summed in ascending
 * triangle index, truncated to bytes, alpha 255; 0 = empty), its normal the plane normal of its lowest-index triangle.  Idempotent; called
 * implicitly by the first voxel frame; sr_set_triangles / sr_load_3ds drop the grid.  A scene with a device builds it there (from the device
 * triangle records: (cell, triangle) pairs, a stable sort, one sum per cell; SR_ERR_UNSUPPORTED beyond 2^30 pairs), a host-only scene with a
 * plain host loop -- two independent implementations of one grid.  The reference's on-disk cache of the grid is not reproduced. */
int  sr_build_voxels(sr_scene*);
/* read-back of the grid in [x][y][z] order: colors[N*N*N], normals[N*N*N][3] (either may be NULL) -- the caller sizes its buffers by
 * sr_get_voxel_res; works for a host-only scene; SR_ERR_NOT_BUILT before sr_build_voxels / the first voxel frame */
int  sr_get_voxels(sr_scene*, uint32_t* colors, double* normals);
/* The grid size N of VoxelGrid(N, ...) / TriMeshToVoxelGrid.Convert(tris, N, grid): 1..256, default 64 = Renderer.cs:1570 (the reference's own
 * voxel tests run at 32); SR_ERR_INVALID_ARG outside 1..256 (three 8-bit coordinates make the 24-bit sort key of the device voxeliser).  A
 * value different from the current one drops the grid: sr_get_voxels answers SR_ERR_NOT_BUILT until the next sr_build_voxels or voxel frame;
 * the same value keeps it.  A multi-device scene forwards the call to its parts; a host-only scene accepts it too.  N <= 64 walks the
 * cells' occupancy bits in LDS, N > 64 a two-level grid (one bit per brick of 4x4x4 cells in LDS, one 64-bit word per brick in memory):
 * the same positions and the same first filled cell at every size. */
int     sr_set_voxel_res(sr_scene*, int32_t n);
int32_t sr_get_voxel_res(const sr_scene*);
/* out = TreeDepth, NumNodes, NumLeafNodes, NumInternalNodes (SpatialSubdivision.cs:317-335) */
int  sr_tree_stats(const sr_scene*, int32_t out[4]);
/* diagnostics: Triangle.HandleToLeafNode of triangle `tri` -- the leaf ProcessLeafNode assigned LAST (SpatialSubdivision.cs:235-243; nodes are built
 * normal side first, so the leaf with the highest node index whose list holds the triangle), which the second stage of the triangle light field
 * searches (sr_set_light_field_triangles).  box = the leaf's box as the containment test uses it (min - 1e-10 x 3, max + 1e-10 x 3); members = the
 * leaf's TriangleIndex list in the leaf's order, at most `cap` of them (members may be NULL with cap 0).  Returns the leaf's member count, or
 * SR_ERR_NOT_BUILT without a reference tree, SR_ERR_INVALID_ARG for a bad argument.  Works on a host-only scene. */
int64_t sr_tree_handle_leaf(const sr_scene*, int64_t tri, double box[6], int32_t* members, int64_t cap);
/* the library's own BVH: out = depth, inner nodes, triangles, 1 if it was built on the device */
int  sr_bvh_stats(const sr_scene*, int64_t out[4]);
/* diagnostics: FNV-1a hashes of the host-built BVH's node array and of its leaf-ordered triangle indices (the host build must not
 * depend on the number of threads it ran on); SR_ERR_NOT_BUILT for a device-built tree */
int  sr_bvh_digest(const sr_scene*, uint64_t out[2]);
/* diagnostics: the four-children-per-node form of the own BVH that the wave-cooperative packet walks traverse (collapsed
 * from the binary tree: same boxes, same leaves, same leaf order): out = depth, nodes, child slots in use, leaves, triangles
 * in leaves; a device-built tree's nodes are read back from the device; SR_ERR_NOT_BUILT without an own BVH, SR_ERR_UNSUPPORTED
 * if a link is broken */
int  sr_wide_tree_stats(const sr_scene*, int64_t out[5]);

/* Renderer.Render() for one Instance, raytrace path (Renderer.cs:701-778 -> RaytraceGeometry :1501 ->
 * RaytraceBlock :1690).  pixels = caller-owned int[W*H] ARGB, row-major pixels[row*W+col]
 * (Surface.DrawPixel, Surface.cs:174-181); only rows start_row..end_row are written; with strips the
 * buffer is the compact strip buffer.  stats (may be NULL) = NumRaysFired, NumGeometryTests,
 * NumNodeVisits, NumLeafNodeVisits (Renderer.cs:465-504) summed over the frame's PRIMARY rays
 * (deterministic, unlike the reference's racy per-block counters, :1695). */
int  sr_render(sr_scene*, const sr_frame*, int32_t* pixels, uint64_t stats[4]);
/* forget the static shadow cache (what a new Renderer / ShadowMethod starts with); sr_set_triangles does it too */
int  sr_reset_shadow_cache(sr_scene*);
/* rayTraceShadowsStatic's cache (SR_F_STATIC_SHADOWS, sr_static_shadow_points): 128^3 bytes in [x][y][z] order (x * 128 * 128 + y * 128 + z),
 * 0 = empty cell -- the bytes the reference's Texture3DCache moves to and from its softShadow_..._res128.cache file (SaveCacheToDisk /
 * LoadCacheFromDisk), so a host can save and load that file itself (the library does no file I/O).  A set cache is what the next static
 * frame and the next sr_static_shadow_points read, and is not zeroed by them.  sr_reset_shadow_cache, sr_set_triangles*, sr_load_3ds and
 * sr_refit_triangles_device drop it.  Both work on a host-only scene; a scene that never rendered a static frame reads back zeros; both wait
 * for a frame of the scene in flight.  A multi-device scene keeps the cache on devices[0]. */
int  sr_get_shadow_cache(sr_scene*, uint8_t out[128 * 128 * 128]);
int  sr_set_shadow_cache(sr_scene*, const uint8_t in[128 * 128 * 128]);
/* rayTraceAmbientOcclusion's cache (SR_F_AMBIENT_OCCLUSION): 128^3 bytes in [x][y][z] order, 0 = empty cell -- exactly the array the
 * reference persists to its .ao file (AmbientOcclusion.cs:232-309), so a host can save and load that file itself (the library does no file
 * I/O).  sr_reset_ao_cache: what a new Renderer starts with; sr_set_triangles / sr_load_3ds drop the cache too.  All three work on a
 * host-only scene; a scene that never rendered an AO frame reads back zeros. */
int  sr_reset_ao_cache(sr_scene*);
int  sr_get_ao_cache(sr_scene*, uint8_t out[128 * 128 * 128]);
int  sr_set_ao_cache(sr_scene*, const uint8_t in[128 * 128 * 128]);
/* rayTraceLightField's table (SR_F_LIGHT_FIELD): 4 N^4 uint32 entries, 0 = empty -- the array the reference persists to its .cache file
 * (LightField4D.cs), so a host can save and load that file itself; `first` / `count` address a range of entries so that the 256 MiB of
 * N = 64 can be streamed.  sr_set_light_field_res: N in 1..128 (default 64, the reference's regression value; 128 is 4 GiB), SR_ERR_INVALID_ARG
 * outside; a change of N drops the table.  sr_reset_light_field: what a new Renderer starts with; sr_set_triangles / sr_load_3ds drop the
 * table too.  The table is allocated on first use (the first SR_F_LIGHT_FIELD frame or sr_set_light_field); a scene that never rendered
 * such a frame reads back zeros.  All of them work on a host-only scene, which keeps a host copy of what sr_set_light_field gave it. */
int  sr_set_light_field_res(sr_scene*, int32_t n);
int32_t sr_get_light_field_res(const sr_scene*);
int  sr_reset_light_field(sr_scene*);
int  sr_get_light_field(sr_scene*, uint32_t* out, uint64_t first, uint64_t count);
int  sr_set_light_field(sr_scene*, const uint32_t* in, uint64_t first, uint64_t count);
/* Pre-compute the table: every entry of [first, first + count) that is 0 gets exactly what a light-field frame would store for its cell -- the
 * colour of the canonical ray from patch centre P(u, v) towards P(s, t), traced through `frame`'s root geometry (extra geometry + the model in
 * frame->trace_mode), shaded with the frame's transform and lights when SR_F_SHADING is set, background_argb | 0xFF000000 on a miss (and for the
 * NaN rays of N = 1, which are not traced), 0 stored as 1.  Non-zero entries stay as they are; *filled (may be NULL) = entries written.  A complete
 * table turns every later light-field frame into look-ups that never touch geometry.  `frame` must carry SR_F_LIGHT_FIELD (SR_ERR_INVALID_ARG
 * otherwise) and passes sr_render's validation (the same SR_ERR_UNSUPPORTED refusals); its camera fields (surface, rows, sub-pixel samples, focal
 * blur) are validated and otherwise unused.  A range beyond the 4 N^4 entries: SR_ERR_INVALID_ARG; count == 0: SR_OK.  Arguments and frame are
 * checked before the device is looked at; a host-only scene then returns SR_ERR_NO_DEVICE.  The call blocks like sr_render, orders itself after a
 * frame in flight, and allocates / zeroes the table as a frame does.  The range is cut into kernel launches of at most 2^24 cells, with no host
 * synchronisation in between.  A multi-device scene bakes on its first device, where the table lives.  sr_last_ray_stats afterwards: [0..3] = 0,
 * [4] = canonical rays traced (one per entry written, none for NaN rays), [5..7] = what their walks counted (0 with SR_F_PRIMARY_STATS_ONLY). */
int  sr_bake_light_field(sr_scene*, const sr_frame* frame, uint64_t first, uint64_t count, uint64_t* filled /* or NULL */);
/* The light field over ShadowMethod, opt-in per scene.  In the reference LightFieldColorMethod is the outermost decorator (Renderer.cs:1640-1649):
 * with rayTraceShadows a cell's canonical ray goes through ShadowMethod and the table stores SHADOWED colours (the active test
 * RaytraceLightField_Colors, RendererTests.cs:240).  The offset table is made once from the seed and the shadow step reads only the hit point,
 * the normal and the light, so the shadowed colour of a cell is still a function of the cell alone.  on = 1: sr_render, sr_render_device and
 * sr_bake_light_field accept SR_F_LIGHT_FIELD | SR_F_SHADOWS without SR_F_STATIC_SHADOWS -- the canonical rays that hit are queued and take the
 * frame's dynamic shadow stage (shadow_samples, area_light_offsets, point or directional light, SR_F_PER_LANE_SHADOWS, SR_F_LITERAL_SECONDARY
 * as in any frame) before their colours are stored; no host synchronisation inside a frame, and the bake cuts its range into passes of at most
 * 2^22 cells so that the stage's scratch does not depend on the size of the table.  Every other refusal of a light-field frame stays: static
 * shadows, SR_F_AMBIENT_OCCLUSION, SR_F_PATH_TRACING, SR_F_VOXELS, max_bounces > 0, SR_F_SINGLE_KERNEL, strip_count > 0, sr_rccl_render.
 * on = 0 (the default): SR_F_LIGHT_FIELD | SR_F_SHADOWS is SR_ERR_UNSUPPORTED, as before.  Anything else: SR_ERR_INVALID_ARG.  A setting like the
 * resolution: it works on a host-only scene, survives sr_set_triangles* / sr_load_3ds, and a multi-device scene forwards it to its parts.  It does
 * not touch the table: an entry keeps whatever the frame that filled it stored -- pose, lights and, now, whether it was shadowed; a frame with the
 * switch on but without SR_F_SHADOWS runs exactly what it ran before.  Statistics of a shadowed light-field frame or bake: [4..7] grow by the
 * canonical rays plus what the shadow stage counts for a frame; all of [4..7] stay 0 with SR_F_PRIMARY_STATS_ONLY. */
int  sr_set_light_field_shadows(sr_scene*, int32_t on);
int32_t sr_get_light_field_shadows(const sr_scene*);
/* Quad-linear interpolation of the colour light field, opt-in per scene (LightFieldColorMethod.Interpolate, LightFieldColorMethod.cs:142-181, which
 * the reference ships hard-wired to false).  on = 1: the SR_F_LIGHT_FIELD frames of sr_render and sr_render_device (a multi-device scene: on devices[0])
 * blend the 16 entries around a sample's 4-D coordinate instead of taking the one its line falls into.  FP64, no contraction:
 *   F = RayToFloat4D (LightField4D.cs:214-245) = (u * (2N), v * N, s * (2N), t * N), u, v, s, t and the sphere test as for the nearest lookup (whose
 *       RayToCoord4D scales by 2N - 1 and N - 1: the reference's mismatch, kept; a cell's canonical ray stays Coord4DToRay's); a line that misses
 *       the sphere (term < 1e-10) gives the background;
 *   b_k = (byte)F_k (truncate, & 255, NaN -> 0), frac_k = F_k - (double)b_k;
 *   for du, dv, ds, dt in {0, 1}, du outermost and dt innermost: c = the entry of cell ((b_u + du) % 2N, (b_v + dv) % N, (b_s + ds) % 2N, (b_t + dt) % N)
 *       -- an empty one is filled first, with exactly what a nearest-lookup frame stores for that cell --, and per channel
 *       acc = acc + ((((byte(c) / 255.0) * wu) * wv) * ws) * wt, w = frac for offset 1 and 1 - frac for offset 0, acc from 0;
 *   sample = 0xFF000000 | (byte)(r * 255.0) << 16 | (byte)(g * 255.0) << 8 | (byte)(b * 255.0).
 * Colours and tables are pinned for inputs with every F_k < 256 and every channel value x * 255 in [0, 256).  on = 0 (the default): nothing changes.
 * Anything else: SR_ERR_INVALID_ARG.  A setting like sr_set_light_field_shadows: it works on a host-only scene, survives sr_set_triangles* /
 * sr_load_3ds, is forwarded to the parts of a multi-device scene, never touches the table, and leaves sr_bake_light_field and every refusal of a
 * light-field frame as they are.  With sr_set_light_field_shadows on, the 16 neighbours are filled through the shadow stage like any cell.  A band
 * lists at most min(16 x its samples, 4 N^4) cells and its scratch has that room (with shadows the bands are 1/16 as large instead): no overflow,
 * no host synchronisation inside a frame.  Statistics as for a light-field frame: [0] = camera samples, [4..7] = the canonical rays of filled cells. */
int  sr_set_light_field_interpolation(sr_scene*, int32_t on);
int32_t sr_get_light_field_interpolation(const sr_scene*);
/* The triangle-index light field, opt-in per scene: rayTraceLightField with LightFieldStoresTriangles = true -> LightFieldTriMethod (Renderer.cs:1590-1611,
 * LightFieldTriMethod.cs:82-231; the reference's own default).  on = 1: the SR_F_LIGHT_FIELD frames of sr_render / sr_render_device and sr_bake_light_field
 * run this method on the TRIANGLE TABLE, a second table of 4 N^4 uint32 beside the colour table (allocated on first use; neither touches the other):
 *   entry 0 = empty, 1 = the cell's canonical ray hit nothing, e >= 2 = triangle e - 2.  The reference's ushort wraps above 65 534 triangles (its own
 *   TODO); the wrap is not reproduced: for n <= 65 534 triangles the low 16 bits of an entry are the reference's .cache value.
 * LightFieldTriMethod is the INNERMOST decorator: it never consults the root geometry it wraps, so the extra geometry has no effect on such a frame.
 * Per camera sample, ray (start, dir) in model space, unmodified:
 *   cell    as for the colour table (same device function); a line that misses the 0.866 sphere is the background;
 *   fill    an empty entry is filled first: the cell's canonical ray (patch centre P(u, v) towards P(s, t), as for the colour table) is traced
 *           through the MODEL ALONE in frame->trace_mode; a hit stores TriangleIndex + 2, a miss (and the NaN ray of N = 1) 1.  The entry depends on
 *           the cell alone: not on the pose, the lights, who fills it or in what order -- a table baked once stays valid while camera, instance
 *           transform and lights move;
 *   e == 1  the background;
 *   stage 1 Triangle.IntersectRay(start, dir) on triangle e - 2 alone -- unclipped start, no root-box clip, no rayFrac offset.  A hit is the result,
 *           even where another triangle is nearer (the reference's artefact, kept);
 *   stage 2 (stage 1 missed) IntersectRayWithLeafNode on the triangle's HandleToLeafNode: the reference tree's leaf that listed the triangle last
 *           (sr_tree_handle_leaf) -- its triangles in the leaf's order against the unclipped ray, nearest hit with strict < whose position lies in the
 *           leaf's box (1e-10 slack), no offset;
 *   stage 3 (stage 2 missed) the full trace of the model, SpatialSubdivision.IntersectRay in SR_MODE_REF_TREE; its answer, hit or miss, is the result.
 * The colour is ShadingMethod's with SR_F_SHADING (position, plane normal, triangle colour), else the triangle's colour; sub-pixel samples, focal blur,
 * row ranges, bands and the resolve are those of any frame.  The reference tree must be built: SR_MODE_REF_TREE is the literal method; SR_MODE_BVH is a
 * library option whose FULL traces (canonical rays, stage 3) take the own BVH with its nearest-hit semantics while stages 1 and 2 still read the
 * reference tree (SR_ERR_NOT_BUILT without it); SR_MODE_BRUTE is SR_ERR_UNSUPPORTED (the method never traces the triangle list).  Every combination a
 * colour light-field frame refuses stays refused, and SR_F_SHADOWS is refused in both forms whatever sr_set_light_field_shadows says (in the reference
 * the secondary rays go through this decorator too: not built).  sr_set_light_field_interpolation is ignored while the switch is on; a multi-device
 * scene renders on devices[0].  A setting like sr_set_light_field_shadows: 0 or 1 (anything else SR_ERR_INVALID_ARG), works on a host-only scene,
 * survives sr_set_triangles* / sr_load_3ds, is forwarded to the parts of a multi-device scene; default 0: nothing changes anywhere.
 * sr_get_light_field_tris / sr_set_light_field_tris: range access like the colour table's (a host-only scene keeps a host copy); an entry that names no
 * triangle of the model reads as 1.  Both tables are dropped by sr_reset_light_field, sr_set_light_field_res, sr_set_triangles*, sr_load_3ds and
 * sr_refit_triangles_device.  A later sr_build with another max_depth / max_per_leaf keeps the triangle table: in SR_MODE_REF_TREE an entry is the
 * triangle the tree's walk returns, which depends on the tree only where two leaves disagree about a hit on their common face (the leaf-face rule of
 * SR_MODE_REF_TREE above).  sr_bake_light_field with the switch on: every empty entry of the range gets TriangleIndex + 2 or 1, *filled counts as
 * before; the frame is needed for trace_mode only but validated as today.
 * Statistics of such a frame: [0] camera samples; [1] triangle tests -- one per sample with e >= 2, the leaf's count per sample that reaches stage 2,
 * what the stage-3 walks count; [2], [3] one node and one leaf per stage-2 call plus the stage-3 walks'; [4] canonical rays traced (one per cell
 * filled; none for NaN rays), [5..7] their walks ([4..7] are 0 with SR_F_PRIMARY_STATS_ONLY in a frame; a bake counts [4] always).  Without
 * SR_F_PRIMARY_STATS_ONLY [20..23] hold the stage census instead of the mirror rays' figures: [20] samples with no candidate triangle (sphere miss or
 * e == 1), [21] resolved by stage 1, [22] by stage 2, [23] that reached stage 3.  [1..3] and [5..7] are pinned in SR_MODE_REF_TREE only; on the own BVH
 * they count what the walks fetch. */
int  sr_set_light_field_triangles(sr_scene*, int32_t on);
int32_t sr_get_light_field_triangles(const sr_scene*);
int  sr_get_light_field_tris(sr_scene*, uint32_t* out, uint64_t first, uint64_t count);
int  sr_set_light_field_tris(sr_scene*, const uint32_t* in, uint64_t first, uint64_t count);
/* LightField4D.RayToFloat4D in batch, at the scene's sr_get_light_field_res: coords[i] = F of the line (starts[i], dirs[i]) (model space, host arrays),
 * inside[i] = 1; a line that misses the sphere: inside[i] = 0 and coords[i] = 0.  Computed on the device by the device function the interpolating
 * frame kernels call, so a caller can reproduce such a frame exactly from these coordinates (the device's atan2 / asin differ from a host's by
 * ulps).  Bad arguments: SR_ERR_INVALID_ARG, before the device is looked at; a host-only scene then returns SR_ERR_NO_DEVICE.  n == 0: SR_OK. */
int  sr_light_field_coords(sr_scene*, int64_t n, const double* starts, const double* dirs, double* coords /* [n][4] */, uint8_t* inside /* [n] */);
/* LightFieldColorMethod.IntersectRay in batch (LightFieldColorMethod.cs:92-217): the colour light field for n lines of the caller's -- a panorama, a
 * cube-map face, a fisheye, the second rays of a pipeline -- where SR_F_LIGHT_FIELD serves the pinhole camera of a frame.  starts[i], dirs[i]: [n][3]
 * in model space, the direction not normalised (sr_trace_rays' and sr_light_field_coords' conventions).  out[i] is the colour a light-field frame
 * gives a camera sample whose ray is (starts[i], dirs[i]): the sphere test, the cell and the entry exactly as SR_F_LIGHT_FIELD defines them; a line
 * with term < 1e-10 gets frame->background_argb | 0xFF000000.  inside[i] (optional) = 1 when the line pierces the sphere, else 0.
 * An empty entry is filled first with what a frame would store for the cell: the canonical ray through `frame`'s root geometry in
 * frame->trace_mode, shaded with SR_F_SHADING, through the dynamic shadow stage when the scene has sr_set_light_field_shadows on and the frame
 * carries SR_F_SHADOWS -- in the scene's table, the one frames and sr_bake_light_field use, so a batch split over several calls equals the one
 * call bit for bit and a batch may follow or precede frames.  *filled = the entries written, as the bake counts them (N = 1: its one cell, whose
 * canonical ray is NaN, stores the background).  With sr_set_light_field_interpolation on, out[i] is the quad-linear blend of the 16 neighbours
 * as an interpolating frame computes it; empty neighbours are filled first.
 * SR_F_LIGHT_FIELD is implied; the camera fields of `frame` are validated as for a frame and otherwise unused.
 * Refused, in this order: n < 0, a NULL starts / dirs / out with n > 0, a NULL frame or scene, options != 0 (reserved): SR_ERR_INVALID_ARG;
 * sr_set_light_field_triangles on (LightFieldTriMethod's three stages per ray are not part of this): SR_ERR_UNSUPPORTED; the switches a light-field
 * frame refuses -- SR_F_AMBIENT_OCCLUSION, SR_F_PATH_TRACING, SR_F_VOXELS, SR_F_SINGLE_KERNEL -- and max_bounces > 0, strip_count > 0:
 * SR_ERR_UNSUPPORTED; then sr_render's validation of the frame (shadows without the scene's switch, static shadows) and of its trace mode
 * (SR_ERR_NOT_BUILT ...); then a host-only scene: SR_ERR_NO_DEVICE.  n == 0 that passes these checks: SR_OK, nothing is touched, *filled = 0.
 * Ordered like a frame (behind a frame of the scene in flight on any stream, the next frame behind it), in passes of at most 2^22 rays (1/16 of
 * that with interpolation and shadows together, as the frame's bands; SR_DBG_BAND_SAMPLES makes them smaller) that follow each other without the
 * host waiting; a later pass reads what an earlier one filled.  A multi-device scene runs it on devices[0].  The host variant blocks and leaves
 * the statistics in sr_last_ray_stats: [0] n, [1..3] 0, [4] canonical rays traced (none for a NaN ray), [5..7] their walks, [4..] also the
 * shadow stage's counts when shadowed; [4..] are 0 with SR_F_PRIMARY_STATS_ONLY.  The device variant takes device arrays, enqueues on `hip_stream`
 * without a host synchronisation and writes *d_filled and d_stats when given. */
int  sr_light_field_rays(sr_scene*, const sr_frame* frame, int64_t n, const double* starts, const double* dirs, uint32_t* out,
                         uint8_t* inside /* or NULL */, uint32_t options, uint64_t* filled /* or NULL */);
int  sr_light_field_rays_device(sr_scene*, const sr_frame* frame, int64_t n, const double* d_starts, const double* d_dirs, uint32_t* d_out,
                                uint8_t* d_inside /* or NULL */, uint32_t options, void* hip_stream, uint64_t* d_filled /* or NULL */,
                                uint64_t* d_stats /* device uint64[SR_STATS_COUNT] or NULL */);
/* Same, but `d_pixels` is DEVICE memory on the scene's device (e.g. a torch tensor's data_ptr) and the
 * work is enqueued on `hip_stream` (a hipStream_t; NULL = the null stream) without host sync. */
/* Ordering: the work is enqueued behind everything already on `hip_stream` and `hip_stream` continues only after it; a
 * shadowed frame is internally forked onto two library-owned streams (event fork / join), see SR_F_NO_SPLIT.  Frames of ONE scene
 * run in submission order whatever streams they are given (the scene's scratch and its per-camera / per-light records belong to one
 * frame at a time: a frame's stream waits for an event the previous frame of the scene left behind); to overlap frames, use scenes. */
int  sr_render_device(sr_scene*, const sr_frame*, void* d_pixels, void* hip_stream, uint64_t* d_stats /* device uint64[SR_STATS_COUNT] (see sr_last_ray_stats) or NULL */);
/* number of int32 pixels sr_render writes for this frame (W*H, or the compact strip size) */
int64_t sr_frame_pixel_count(const sr_frame*);

/* IRayIntersectable.IntersectRay in batch (Raytrace/IRayIntersectable.cs:31-48): the operator interface
 * every primitive, the tree and the decorators implement.  target = SR_MODE_* for the model alone, or
 * SR_TARGET_ROOT = the root geometry of the chain (extra geometry + model in `mode`, Renderer.cs:1536-1549).
 * Host arrays; outputs may be NULL.  counters[n][3] = NumRayTests, NumNodesVisited, NumLeafNodesVisited. */
#define SR_TARGET_ROOT 0x100
/* target = SR_TARGET_VOXELS: VoxelGrid.IntersectRay on the N^3 grid (see SR_F_VOXELS, sr_set_voxel_res): hit, colour and normal; ray_frac and pos are 0, tri_index is -1,
 * counters are {1, 0, 0} (VoxelGrid.NumRayTests == 1).  Builds the grid when there is none. */
#define SR_TARGET_VOXELS 0x200
int  sr_trace_rays(sr_scene*, int32_t target, int64_t n, const double* starts, const double* dirs,
                   uint8_t* hit, double* ray_frac, double* pos, double* normal, uint32_t* color,
                   int32_t* tri_index, int32_t* counters);

/* The same with every array in DEVICE memory on the scene's device, enqueued on `hip_stream` without a host synchronisation: what a
 * throughput measurement of the reference's per-primitive / per-tree micro-benchmarks needs (TriangleTests.cs:100-330,
 * SpatialSubdivisionTests.cs:140-260 time IntersectRay alone, not a transfer).  Outputs may be NULL. */
int  sr_trace_rays_device(sr_scene*, int32_t target, int64_t n, const double* d_starts, const double* d_dirs,
                          uint8_t* d_hit, double* d_ray_frac, double* d_pos, double* d_normal, uint32_t* d_color,
                          int32_t* d_tri_index, int32_t* d_counters, void* hip_stream);

/* A batch of rays that START IN ONE POINT, on the walk a frame's camera rays take: for every i and every non-NULL output the result is bit
 * for bit what sr_trace_rays(scene, target, n, starts, dirs, ...) answers with starts[i] = origin for all i -- same conventions (a miss
 * writes hit 0, zeros and tri_index -1; a hit on extra geometry has tri_index -1 and the primitive's colour; `color` is unshaded), dirs is
 * [n][3] and need not be normalised, every output is optional (all NULL: the call runs for the statistics).  What differs is the speed: in
 * SR_MODE_BVH the per-origin records of a frame are set up for `origin` (facing partition, camera-cone records, fitted boxes, the ordered
 * four-wide copy, with (near, far) planes when the origin is outside the root box's slab on all three axes: sr_debug_counters[5]) and 64
 * rays at a time share one packet walk.  Panoramas, cube-map faces, lens models, foveated sample sets, scans.
 * target: SR_MODE_* (the model alone) or SR_TARGET_ROOT | SR_MODE_*; SR_TARGET_VOXELS is SR_ERR_UNSUPPORTED.  SR_MODE_REF_TREE and
 * SR_MODE_BRUTE trace every ray with a private walk, as sr_trace_rays does, and so does SR_MODE_BVH under SR_DBG_PER_LANE_PRIMARY;
 * SR_DBG_BVH2_PACKETS selects the binary-tree packets, as in a frame.
 * Order: SR_RAYS_COHERENT (options bit 0) is the caller's promise that every run of 64 consecutive rays is a bundle of neighbours (an image
 * in 8x8-tile-major order, say): wave w of a pass takes rays 64 w .. 64 w + 63 as given.  Without it a pass is first ordered by direction
 * (the cell of the unit direction in an octahedral map of 2^12 x 2^12 cells, Morton-interleaved; a stable radix sort).  Results never depend
 * on the option or on the order; speed does.  Other option bits: SR_ERR_INVALID_ARG.
 * A ray is REGULAR when its three components are finite and 2^-40 <= max |d_k| <= 2^40: the fp32 margins of the packet walk's slab tests
 * and cone filter scale with |d| and hold in that range.  Every other ray (the zero vector, NaN, +-inf, 1e300, 1e-300) never enters a
 * packet: it goes to the end of its pass (also with SR_RAYS_COHERENT) and is traced by the function sr_trace_rays calls.
 * origin: HOST memory in both variants; not finite: SR_ERR_INVALID_ARG; any finite point is legal -- inside the root box, outside it, on a
 * triangle's plane.  The camera-cone records are FP64 cross products of (vertex - origin) rounded once to fp32 and evaluated in fp32 against
 * the direction: with the origin further from the root box's centre than 2^20 box diagonals on some axis the FP64 rounding of
 * (vertex - origin) is no longer far below the filter's fp32 margin, and beyond 2^42 a product with a regular direction can overflow
 * fp32.  A frame's camera never stands there (its rays end 10000 |d| from it); such a call runs with private walks (same results).
 * Refusals, in this order: a NULL scene or origin, n < 0, NULL dirs with n > 0, unknown option bits, a non-finite origin:
 * SR_ERR_INVALID_ARG; SR_TARGET_VOXELS: SR_ERR_UNSUPPORTED; sr_trace_rays' own checks (SR_ERR_NO_MODEL, SR_ERR_NOT_BUILT); a host-only
 * scene: SR_ERR_NO_DEVICE.  n == 0 that passes the first three: SR_OK, nothing is touched.
 * State: unlike sr_trace_rays the call REWRITES per-origin state of the scene (the facing partition moves triangle records), so it is
 * ordered like a frame: behind a frame of the scene in flight on any stream, the next frame behind it.  The records stay keyed to `origin`:
 * a following call or frame from the same point reuses them, a frame from elsewhere re-makes them as after any camera move (at 1 M
 * triangles: see profiles/origin_rays) -- alternate origins and every call pays that.  Passes of at most 2^22 rays (SR_DBG_BAND_SAMPLES:
 * fewer) follow each other without the host waiting.  A multi-device scene runs the call on devices[0].  The host variant stages through
 * the scene's device buffers, blocks and fills sr_last_ray_stats; the device variant enqueues on `hip_stream` without a host
 * synchronisation.  Statistics (there is no per-ray counters array: a packet walk counts per wave): [0..3] the primary counters as
 * sr_render_hits defines them -- the reference's notions in SR_MODE_REF_TREE / SR_MODE_BRUTE (the sums of sr_trace_rays' per-ray
 * counters), what a wave fetched on the own BVH -- and [4..] 0. */
#define SR_RAYS_COHERENT 1u
int  sr_trace_origin_rays(sr_scene*, int32_t target, const double origin[3], int64_t n, const double* dirs,
                          uint8_t* hit, double* ray_frac, double* pos, double* normal, uint32_t* color, int32_t* tri_index,
                          uint32_t options, uint64_t stats[4] /* or NULL */);
int  sr_trace_origin_rays_device(sr_scene*, int32_t target, const double origin[3] /* HOST */, int64_t n, const double* d_dirs,
                                 uint8_t* d_hit, double* d_ray_frac, double* d_pos, double* d_normal, uint32_t* d_color,
                                 int32_t* d_tri_index, uint32_t options, void* hip_stream,
                                 uint64_t* d_stats /* device uint64[SR_STATS_COUNT] or NULL */);

/* "Is anything in the way before distance L" for a batch of arbitrary rays: line of sight between two points, a texel's visibility from a
 * light, a form factor, a probe of bounded length -- the question ShadowMethod.cs:169-172 asks (blocked = a hit with rayFrac <= 1.0 on a ray
 * built as end - start) and AmbientOcclusion.cs asks with 2.0.
 * Result: occluded[i] = 1 iff sr_trace_rays(scene, target, ...) answers the ray (starts[i], D_i) with hit == 1 and ray_frac <= limit_i, else
 * 0; nothing else is ever written.  limit_i = limits[i], or 1.0 for every ray when `limits` is NULL.  The comparison is IEEE <=: a NaN limit
 * gives 0, +inf means "any hit", a negative limit gives 0.
 * Direction: D_i = dirs[i], not normalised; with SR_RAYS_ENDPOINTS (options bit 1) dirs[i] is an END POINT and D_i = dirs[i] - starts[i], one
 * FP64 subtraction per component (ShadowMethod.cs:157) -- with the default limit that is "the segment is blocked".
 * target: SR_MODE_* (the model alone) or SR_TARGET_ROOT | SR_MODE_* (extra geometry first, then the model); SR_TARGET_VOXELS is
 * SR_ERR_UNSUPPORTED (a voxel hit has rayFrac 0).
 * Why the walk may stop early: the nearest hit's rayFrac is the minimum over the ray's hits of fl(t + offset) (offset: the clip of the start
 * to the root box; 0 for extra geometry and brute force).  min t <= L holds iff some t <= L does; fl(t + offset) is monotone in t; and
 * Plane.IntersectRay never returns a negative t, so nothing behind the start can be nearer.  Hence "the nearest hit qualifies" iff "some hit
 * qualifies", and on the own BVH (and in brute force) an any-hit walk that stops at the first qualifying hit, and culls every box beyond
 * t = L - offset, gives exactly this answer.  SR_MODE_BVH does that (bvh_intersect<true>(.., limit_i)); SR_MODE_REF_TREE runs the literal walk
 * and compares -- its leaf-face rule (the first leaf with a hit inside its box ends the walk) stays what it is -- and SR_MODE_BRUTE runs the
 * nearest-hit loop and compares.
 * Routing: a ray takes the any-hit walk only when its start is finite (max |s_k| <= 2^100), its limit is neither NaN nor -inf (+inf is
 * allowed) and its direction is REGULAR by sr_trace_origin_rays' definition.  Every other ray -- a zero, NaN, +-inf, 1e300 or 1e-300
 * direction, a non-finite start, a zero-length segment -- goes to the end of its pass and is answered by the function sr_trace_rays calls
 * plus the comparison: equal by construction.
 * Order: without SR_RAYS_COHERENT a pass of SR_MODE_BVH is ordered by the 7-bit Morton cell of the start in the root box, with the
 * direction's octant between the coarse and the fine bits (a stable radix sort); with it the input order is kept, the irregular rays still
 * last.  The other modes walk in input order.  Results never depend on the option or the order; speed does.
 * Refusals, in this order: a NULL scene, n < 0, NULL starts / dirs / occluded with n > 0, unknown option bits: SR_ERR_INVALID_ARG;
 * SR_TARGET_VOXELS: SR_ERR_UNSUPPORTED; sr_trace_rays' own checks (SR_ERR_NO_MODEL, SR_ERR_NOT_BUILT); a host-only scene: SR_ERR_NO_DEVICE.
 * n == 0 that passes all of them: SR_OK, nothing is touched.
 * State: the call rewrites no per-origin or per-light record of the scene, but it reads the triangle records a frame's set-up moves, so it
 * is ordered like a frame: behind a frame of the scene in flight on any stream, the next frame behind it.  Passes of at most 2^22 rays
 * (SR_DBG_BAND_SAMPLES: fewer) follow each other without the host waiting.  A multi-device scene runs the call on devices[0].  The host
 * variant stages through the scene's device buffers, blocks and fills sr_last_ray_stats; the device variant enqueues on `hip_stream`
 * without a host synchronisation.  Statistics: [0] = n; [1..3] in SR_MODE_REF_TREE / SR_MODE_BRUTE the sums of sr_trace_rays' per-ray
 * counters, on the own BVH what the walks fetched (not pinned: an any-hit walk stops where it finds its hit); [4..] 0. */
#define SR_RAYS_ENDPOINTS 2u      /* options bit 1; bit 0 is SR_RAYS_COHERENT */
int  sr_occluded_rays(sr_scene*, int32_t target, int64_t n, const double* starts, const double* dirs,
                      const double* limits /* [n], or NULL: 1.0 for every ray */, uint8_t* occluded,
                      uint32_t options, uint64_t stats[4] /* or NULL */);
int  sr_occluded_rays_device(sr_scene*, int32_t target, int64_t n, const double* d_starts, const double* d_dirs,
                             const double* d_limits /* or NULL */, uint8_t* d_occluded, uint32_t options,
                             void* hip_stream, uint64_t* d_stats /* device uint64[SR_STATS_COUNT] or NULL */);

/* The NEAREST HIT of a batch of arbitrary rays, with a per-ray distance limit, on the walk the library keeps for incoherent rays: what a
 * reflection, a refraction, a gather or the second bounce of a caller's pipeline asks.  More than one bounce and mirror chains are the
 * caller's loop over this call (see sr_render_hits, sr_shade_points, sr_path_points for the other steps).
 * Result: for every ray and every non-NULL output, bit for bit what sr_trace_rays(scene, target, ...) answers for (starts[i], D_i), provided
 * that answer is a hit with ray_frac <= limit_i; otherwise sr_trace_rays' miss (hit 0, zeros, tri_index -1).  limits == NULL: no limit, i.e.
 * sr_trace_rays exactly.  The comparison is IEEE <=: NaN, -inf and negative limits give a miss, +inf any hit.  Every output is optional
 * (all NULL: the call runs for the statistics).  A hit on extra geometry has tri_index -1 and the primitive's colour; `color` is unshaded.
 * Direction: D_i = dirs[i], not normalised; with SR_RAYS_ENDPOINTS dirs[i] is an END POINT and D_i = dirs[i] - starts[i], one FP64
 * subtraction per component as in sr_occluded_rays -- a limit of 1.0 then means "up to the end point".
 * target: SR_MODE_* (the model alone) or SR_TARGET_ROOT | SR_MODE_*; SR_TARGET_VOXELS is SR_ERR_UNSUPPORTED.
 * Why culling at the limit is exact: ray_frac = fl(t + offset) is monotone in t, so if the nearest hit does not qualify no hit does, and "the
 * nearest hit, if it qualifies" is "the nearest qualifying hit".  The walk on the own BVH culls every box beyond t = limit - offset, inflated
 * as bvh_intersect<true> does it (sr_occluded_rays above); whatever it then finds beyond the limit fails the final FP64 test
 * best + offset <= limit.  SR_MODE_REF_TREE and SR_MODE_BRUTE run sr_trace_rays' walk and compare afterwards; the reference tree's leaf-face
 * rule stays what it is.
 * Routing in SR_MODE_BVH: a ray that is REGULAR by sr_occluded_rays' definition (finite start with max |s_k| <= 2^100, regular direction, a
 * limit that is neither NaN nor -inf) takes three kernels: k_nr_prep (FP64 clip to the root box, offset, the fp32 cull bound), k_nr_walk
 * (persistent lanes refilled at 24 busy ones, the four-wide tree with up to eight pending leaves, the first 24 stack levels in LDS, the fp32
 * pre-test, the reference's FP64 triangle test with the lowest-index tie rule) and k_nr_finish (extra geometry from the unclipped start, the
 * limit, the outputs).  Every other ray goes to the end of its pass and is answered by the function sr_trace_rays calls plus the comparison:
 * equal by construction.
 * Order: without SR_RAYS_COHERENT a pass of SR_MODE_BVH is ordered as sr_occluded_rays orders it (start cell, direction octant, a stable radix
 * sort); with it the input order is kept, the irregular rays still last.  Results never depend on the option or the order; speed does.
 * Refusals, in this order: a NULL scene, n < 0, NULL starts / dirs with n > 0, unknown option bits: SR_ERR_INVALID_ARG; SR_TARGET_VOXELS:
 * SR_ERR_UNSUPPORTED; sr_trace_rays' own checks (SR_ERR_NO_MODEL, SR_ERR_NOT_BUILT); a host-only scene: SR_ERR_NO_DEVICE.  n == 0 that passes
 * all of them: SR_OK, nothing is touched.
 * State: as sr_occluded_rays -- no per-origin or per-light record is rewritten, the call is ordered like a frame.  Passes of at most 2^22 rays
 * (SR_DBG_BAND_SAMPLES: fewer) follow each other without the host waiting.  A multi-device scene runs the call on devices[0].  Scratch per
 * pass of p rays in SR_MODE_BVH, from the scene's first scratch set: 64 p bytes of ray records, 16 p of walk results, 16 p + 256 of sort keys
 * and order plus the radix sort's own scratch, and for trees deeper than the LDS levels (max(3 x four-wide depth + 2, depth + 2) - 24 levels)
 * x 8 workgroups per CU x 256 lanes x 4 bytes of stack.  The host variant stages through the scene's device buffers, blocks and fills
 * sr_last_ray_stats; the device variant enqueues on `hip_stream` without a host synchronisation.  Statistics (there is no per-ray counters
 * array): [0] = n; [1..3] in SR_MODE_REF_TREE / SR_MODE_BRUTE the sums of sr_trace_rays' per-ray counters, on the own BVH what the walks
 * fetched (not pinned); [4..] 0. */
int  sr_nearest_rays(sr_scene*, int32_t target, int64_t n, const double* starts, const double* dirs,
                     const double* limits /* [n], or NULL: no limit */,
                     uint8_t* hit, double* ray_frac, double* pos, double* normal, uint32_t* color, int32_t* tri_index,
                     uint32_t options, uint64_t stats[4] /* or NULL */);
int  sr_nearest_rays_device(sr_scene*, int32_t target, int64_t n, const double* d_starts, const double* d_dirs,
                            const double* d_limits /* or NULL */,
                            uint8_t* d_hit, double* d_ray_frac, double* d_pos, double* d_normal, uint32_t* d_color, int32_t* d_tri_index,
                            uint32_t options, void* hip_stream, uint64_t* d_stats /* device uint64[SR_STATS_COUNT] or NULL */);

/* ALL HITS along each ray of a batch, nearest first, with a count: what transparency and X-ray compositing, thickness and path length inside a
 * solid, inside/outside classification, CSG and picking through layers ask -- without peeling (K calls of sr_nearest_rays with an epsilon).
 * Direction and options: as sr_occluded_rays / sr_nearest_rays (SR_RAYS_COHERENT, SR_RAYS_ENDPOINTS; D_i = dirs[i], or dirs[i] - starts[i] with
 * one FP64 subtraction per component).
 * The hit set of ray i.  SR_MODE_BVH: every triangle j whose record passes the per-record test of the own BVH's walk -- the start clipped to
 * the root box (ClipLineSegment), offset = |original - s| / |D|, then Triangle.IntersectRay(rec_j, s, D) with the hit position strictly inside
 * the root box; its ray_frac is the one FP64 sum t + offset.  Equivalently: j is in the set iff a scene that holds triangle j alone, in the
 * same box, answers the ray with a hit, and ray_frac is that answer's.  SR_MODE_BRUTE: the per-record loop of GeometryCollection --
 * Triangle.IntersectRay from the unclipped start, ray_frac = t, no box test.  Triangles are one-sided, as everywhere.  SR_TARGET_ROOT | mode:
 * every element e of the extra geometry adds at most one hit, its own IntersectRay answer from the unclipped start (a rayFrac of DBL_MAX or
 * more does not count), reported with index = -2 - e.  SR_MODE_REF_TREE is SR_ERR_UNSUPPORTED: the literal walk ends in the first leaf that
 * holds a hit inside its box, a triangle lives in several leaves, and "all hits" is not a notion of SpatialSubdivision.  SR_TARGET_VOXELS is
 * SR_ERR_UNSUPPORTED as in the sibling calls.
 * A hit QUALIFIES iff ray_frac <= limit_i (IEEE <=).  A NaN, -inf or negative limit qualifies nothing, +inf every hit whose ray_frac is a number.
 * limits == NULL: no limit -- no comparison is made, as in sr_nearest_rays: an irregular ray whose ray_frac is NaN (offset 0 / 0) still counts, and
 * sorts behind every number.
 * Outputs: count[i] = the number of qualifying hits, NOT capped by max_hits (K).  Row i of index / ray_frac ([n][K]) holds the min(count, K)
 * qualifying hits that come first in the order: ray_frac ascending; at equal ray_frac extra elements before triangles; then element /
 * TriangleIndex ascending.  Every remaining slot of every row is written: index -1, ray_frac 0.0 -- the caller clears nothing.  The order is
 * defined on the reported values.  Relations: count > 0 equals sr_occluded_rays with the same explicit limits; ray_frac[i][0] and count > 0
 * equal sr_nearest_rays' ray_frac and hit; index[i][0] equals its tri_index whenever no other qualifying hit shares that ray_frac
 * (sr_trace_rays breaks ties on t, before the offset is added).
 * NULL arrays: max_hits == 0 is the counting call (index and ray_frac are ignored).  Any of the three arrays may be NULL; all NULL: the call
 * runs for the statistics.  A row the caller does not ask for is kept in the scene's first scratch set (ray_frac is needed for the order), in
 * passes of at most 2^24 / K rays.  With count == NULL and K > 0 the walk culls every box beyond the K-th hit it holds -- a K-nearest query --
 * with count != NULL only beyond limit - offset; the rows are bit for bit the same either way.  The cull bound is bvh_intersect<true>'s,
 * (float)(bound - offset) * (1 + 2^-20) + 1e-30f, with the FP64 room widened by 2^-51 (|bound| + offset) first.
 * Routing in SR_MODE_BVH: a ray that is REGULAR by sr_occluded_rays' definition walks the tree (k_ah_walk) in a pass ordered by start cell and
 * direction octant (SR_RAYS_COHERENT: input order).  Every other ray -- a zero, NaN, +-inf, 1e+-300 direction, a non-finite start, a
 * zero-length segment, a NaN or -inf limit -- goes to the end of its pass and runs the per-record loop (k_ah_loop): the same FP64 predicate over
 * every record, no fp32 stage, O(triangles) per ray.  SR_MODE_BRUTE runs that loop (unclipped) for every ray in input order.
 * Refusals, in this order: a NULL scene, n < 0, NULL starts / dirs with n > 0, max_hits outside 0 .. SR_HITS_MAX, unknown option bits:
 * SR_ERR_INVALID_ARG; SR_TARGET_VOXELS: SR_ERR_UNSUPPORTED; SR_MODE_REF_TREE: SR_ERR_UNSUPPORTED; sr_trace_rays' own checks (SR_ERR_NO_MODEL,
 * SR_ERR_NOT_BUILT); a host-only scene: SR_ERR_NO_DEVICE.  n == 0 that passes all of them: SR_OK, nothing is touched.
 * State: as sr_nearest_rays -- no per-origin or per-light record is rewritten, the call is ordered like a frame.  Passes of at most 2^22 rays
 * (SR_DBG_BAND_SAMPLES: fewer) follow each other without the host waiting.  A multi-device scene runs the call on devices[0].  The host variant
 * stages 24 n + 24 n + 8 n bytes in and 4 n + 12 K n bytes out through the scene's device buffers, blocks and fills sr_last_ray_stats; the
 * device variant enqueues on `hip_stream` without a host synchronisation.  Statistics: [0] = n; [1..3] what the walks fetched (in brute force
 * the sums of the per-record tests); [4..] 0. */
#define SR_HITS_MAX 64
int  sr_all_hits_rays(sr_scene*, int32_t target, int64_t n, const double* starts, const double* dirs,
                      const double* limits /* [n], or NULL: no limit */, int32_t max_hits /* K, 0..SR_HITS_MAX */,
                      uint32_t* count /* [n] or NULL */, int32_t* index /* [n][K] or NULL */, double* ray_frac /* [n][K] or NULL */,
                      uint32_t options, uint64_t stats[4] /* or NULL */);
int  sr_all_hits_rays_device(sr_scene*, int32_t target, int64_t n, const double* d_starts, const double* d_dirs,
                             const double* d_limits /* or NULL */, int32_t max_hits,
                             uint32_t* d_count /* or NULL */, int32_t* d_index /* or NULL */, double* d_ray_frac /* or NULL */,
                             uint32_t options, void* hip_stream, uint64_t* d_stats /* device uint64[SR_STATS_COUNT] or NULL */);

/* THE CLOSEST POINT of the mesh for each point of a batch -- which point of which triangle is nearest, and how far away: what distance
 * fields, proximity and collision tests against a moving mesh (sr_refit_triangles_device), snapping to a surface, attribute transfer and the
 * magnitude of a signed distance ask (its sign: the parity of sr_all_hits_rays counts).  No composition of the ray calls answers it.
 * The distance of point q = points[i] to triangle j.  (a, b, c) = the three vertices of triangle j as the scene holds them (FP64, TriangleIndex
 * order).  closest(q, a, b, c) is the Voronoi-region routine (Ericson, Real-Time Collision Detection 5.1.5; csrc/sr_closest.h, one text for the
 * kernels and the host): with ab = b - a, ac = c - a, ap = q - a, bp = q - b, cp = q - c, d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp,
 * d5 = ab.cp, d6 = ac.cp (every dot product x + y + z, left to right), vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, the first of
 * these that holds decides:  d1 <= 0 && d2 <= 0: vertex a, (v, w) = (0, 0).  d3 >= 0 && d4 <= d3: vertex b, (1, 0).  vc <= 0 && d1 >= 0 && d3 <= 0:
 * edge ab, v = d1 / (d1 - d3), w = 0, the point a + ab v.  d6 >= 0 && d5 <= d6: vertex c, (0, 1).  vb <= 0 && d2 >= 0 && d6 <= 0: edge ac, v = 0,
 * w = d2 / (d2 - d6), a + ac w.  va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0: edge bc, w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w, b + (c - b) w.
 * Otherwise the face: v = vb / (va + vb + vc), w = vc / (va + vb + vc), (a + ab v) + ac w.  Fixed operand order, no contraction, only + - * / and
 * comparisons.  (v, w) are the weights of vertices 2 and 3 -- exactly 0 or 1 where a region pins them -- and in a vertex region the point is the
 * vertex itself, bit for bit.  d2_j = (q - c_j).x^2 + (q - c_j).y^2 + (q - c_j).z^2, summed in that order; dist_j = sqrt(d2_j).
 * The answer for q is the j that minimises (d2_j, j) lexicographically over all triangles whose d2_j is a number: a NaN d2_j (a collinear
 * triangle can divide 0 by 0) never wins, equal d2 goes to the lowest TriangleIndex.  It QUALIFIES iff max_dist is NULL or dist <= max_dist[i]
 * (IEEE <=): a NaN, -inf or negative limit qualifies nothing, +inf every number.  A point with no qualifying answer -- no triangle with a
 * numeric distance, a NaN point, a limit that cuts the answer -- gets tri_index -1 and zeros in dist, pos and uv, as a miss does in the sibling calls.
 * Outputs: tri_index[i] = j, dist[i] = dist_j, pos[i] = c_j, uv[i] = (v, w).  Every output is optional; all four NULL: the call runs for the statistics.
 * Targets: SR_MODE_BVH walks the own BVH, SR_MODE_BRUTE runs the per-record loop over the vertices in index order; both give the same answers bit
 * for bit.  SR_MODE_REF_TREE is SR_ERR_UNSUPPORTED (the reference tree duplicates triangles across leaves and has no distance query), and so are
 * SR_TARGET_ROOT | mode (the extra primitives' closest points are not part of the call) and SR_TARGET_VOXELS.
 * Routing in SR_MODE_BVH: a point is REGULAR when it is finite and no component lies further from the root box's centre than
 * min(2^20 box diagonals, 2^60).  A pass is ordered by the 7-bit Morton cell of the point in the root box (points outside clamp to the edge
 * cells; a stable radix sort; SR_POINTS_COHERENT, options bit 0: the input order is kept), and its regular points walk the tree (k_cp_walk): at a
 * node an fp32 LOWER bound of the squared distance to each child's box, the nearer child first, a box skipped only when its bound strictly
 * exceeds min(best d2, max_dist^2) with every rounding on the way covered -- equality never culls, so an equal-distance triangle
 * with a lower index is always found.  Every other point goes to the end of its pass either way and runs the per-record loop (k_cp_loop): the
 * same FP64 routine over every triangle, no fp32 stage, O(triangles) per point.  SR_MODE_BRUTE runs that loop for every point in input order.
 * Refusals, in this order: a NULL scene, n < 0, NULL points with n > 0, unknown option bits: SR_ERR_INVALID_ARG; SR_TARGET_VOXELS,
 * SR_TARGET_ROOT, SR_MODE_REF_TREE: SR_ERR_UNSUPPORTED; sr_trace_rays' own checks (SR_ERR_NO_MODEL, SR_ERR_NOT_BUILT); a host-only scene:
 * SR_ERR_NO_DEVICE.  A refusal writes nothing.  n == 0 that passes all of them: SR_OK, nothing is touched.
 * State: no per-origin or per-light record is rewritten, the call is ordered like a frame.  Passes of at most 2^22 points
 * (SR_DBG_BAND_SAMPLES: fewer) follow each other without the host waiting.  A multi-device scene runs the call on devices[0].  The host variant
 * stages 24 n + 8 n bytes in and 52 n bytes out through the scene's device buffers, blocks and fills sr_last_ray_stats; the device variant
 * enqueues on `hip_stream` without a host synchronisation.  Statistics: [0] = n; [1..3] = triangles tested, nodes and leaves visited (pinned in
 * brute force only: n x triangles, 0, 0); [4..] 0. */
int  sr_closest_points(sr_scene*, int32_t target, int64_t n, const double* points /* [n][3] */,
                       const double* max_dist /* [n], or NULL: no limit */,
                       int32_t* tri_index /* [n] */, double* dist /* [n] */, double* pos /* [n][3] */, double* uv /* [n][2] */,
                       uint32_t options, uint64_t stats[4] /* or NULL */);
int  sr_closest_points_device(sr_scene*, int32_t target, int64_t n, const double* d_points, const double* d_max_dist /* or NULL */,
                              int32_t* d_tri_index, double* d_dist, double* d_pos, double* d_uv /* each may be NULL */,
                              uint32_t options, void* hip_stream, uint64_t* d_stats /* device uint64[SR_STATS_COUNT] or NULL */);

/* THE TRIANGLES WITHIN REACH of each point of a batch, nearest first, with a count -- the point-side counterpart of sr_all_hits_rays: contact and
 * collision candidates against a moving mesh (sr_refit_triangles_device), k-nearest smoothing and attribute transfer, the surface inside a probe
 * sphere.  sr_closest_points gives one triangle per point, and no second call can exclude the triangle the first one found.
 * Per-triangle values: for point q = points[i] and triangle j, c_j, (v, w), d2_j and dist_j = sqrt(d2_j) are exactly sr_closest_points' values
 * (the routine of csrc/sr_closest.h, nothing new).
 * The SET of q: every j whose d2_j is a number (a NaN never counts) and, where max_dist is given, dist_j <= max_dist[i] (IEEE <=): a NaN, -inf or
 * negative limit admits nothing, +inf every number.  max_dist == NULL: no comparison is made.
 * Outputs: count[i] = the size of the set, NOT capped by max_hits (K).  Row i of index / dist / pos / uv ([n][K], [n][K], [n][K][3], [n][K][2])
 * holds the first min(count, K) members ordered by (d2_j, j) ascending: index = j, dist = dist_j, pos = c_j, uv = (v, w).  Every other slot of
 * every row is written: index -1, zeros elsewhere -- the caller clears nothing.  The order is on d2, not on the rounded distance, so slot 0 is
 * sr_closest_points' answer under the same limit, bit for bit in all four outputs; dist is non-decreasing along a row, and two slots with equal
 * dist may come from distinct d2.
 * NULL arrays: max_hits == 0 is the counting call (the four row arrays are ignored).  Any of the five arrays may be NULL; all NULL: the call runs
 * for the statistics.  An index or dist row the caller does not ask for is kept in the scene's first scratch set (both are needed for the order),
 * in passes of at most 2^24 / K points.  With count == NULL and K > 0 the walk also culls every box beyond the K-th entry it holds -- a K-nearest
 * query; the rows are bit for bit the same as with count.
 * Targets: SR_MODE_BVH and SR_MODE_BRUTE, the same answers bit for bit.  SR_MODE_REF_TREE (a triangle lives in several leaves and would be listed
 * twice), SR_TARGET_ROOT | mode (the extra primitives have no triangle indices) and SR_TARGET_VOXELS are SR_ERR_UNSUPPORTED.
 * Routing in SR_MODE_BVH: sr_closest_points' -- the regular points of a pass, ordered by Morton cell (SR_POINTS_COHERENT: input order), walk the
 * tree (k_nt_walk); a box is skipped only when its fp32 lower bound strictly exceeds min(max_dist^2 inflated, the K-nearest cut) with every
 * rounding covered, the cut being +inf until the row is full and whenever count is wanted, max(worst kept d2, least d2 seen whose
 * closest point lies inside its triangle) otherwise: equality never culls, so the (d2, j) order at the cut is exact.  Every other point runs
 * the per-record loop (k_nt_loop), as every point of SR_MODE_BRUTE does in input order.  The limit per candidate is the exact test
 * fl(sqrt(d2)) <= max_dist, made as d2 <= the largest double whose rounded square root is <= max_dist (found once per point).
 * Refusals, in this order: a NULL scene, n < 0, NULL points with n > 0, max_hits outside 0 .. SR_HITS_MAX, unknown option bits:
 * SR_ERR_INVALID_ARG; SR_TARGET_VOXELS, SR_TARGET_ROOT, SR_MODE_REF_TREE: SR_ERR_UNSUPPORTED; sr_trace_rays' own checks (SR_ERR_NO_MODEL,
 * SR_ERR_NOT_BUILT); a host-only scene: SR_ERR_NO_DEVICE.  A refusal writes nothing.  n == 0 that passes all of them: SR_OK, nothing is touched.
 * State: as sr_closest_points -- the call is ordered like a frame, passes of at most 2^22 points (SR_DBG_BAND_SAMPLES: fewer) follow each other
 * without the host waiting, a multi-device scene runs the call on devices[0].  The host variant stages 24 n + 8 n bytes in and 4 n + 52 K n bytes
 * out through the scene's device buffers, blocks and fills sr_last_ray_stats; the device variant enqueues on `hip_stream` without a host
 * synchronisation.  Statistics: [0] = n; [1..3] = triangles tested, nodes and leaves visited (pinned in brute force only: n x triangles, 0, 0);
 * [4..] 0. */
int  sr_near_triangles(sr_scene*, int32_t target, int64_t n, const double* points /* [n][3] */,
                       const double* max_dist /* [n], or NULL: no limit */, int32_t max_hits /* K, 0..SR_HITS_MAX */,
                       uint32_t* count /* [n] or NULL */, int32_t* index /* [n][K] or NULL */, double* dist /* [n][K] or NULL */,
                       double* pos /* [n][K][3] or NULL */, double* uv /* [n][K][2] or NULL */,
                       uint32_t options, uint64_t stats[4] /* or NULL */);
int  sr_near_triangles_device(sr_scene*, int32_t target, int64_t n, const double* d_points, const double* d_max_dist /* or NULL */,
                              int32_t max_hits, uint32_t* d_count, int32_t* d_index, double* d_dist, double* d_pos, double* d_uv /* each may be NULL */,
                              uint32_t options, void* hip_stream, uint64_t* d_stats /* device uint64[SR_STATS_COUNT] or NULL */);

/* THE TRIANGLES OF THE MODEL THAT CROSS each triangle of a batch, with a count and, per pair, which edges pierce -- mesh against mesh, the
 * fifth question next to the rays' and the points': contact against a mesh that moves (sr_refit_triangles_device), a tool against a surface, "is
 * it colliding at all".  The edges of a query sent through sr_all_hits_rays find where the query pierces the scene; the other half, scene edges
 * that pierce the query, has no other route, and ray hits are one-sided and clipped to the root box.
 * The pair predicate (csrc/sr_tri_overlap.h: one text for the kernels and the host, FP64, only + - * and comparisons in a fixed operand order, no
 * contraction):
 *   vol(a, b, c, d): u = b - a, v = c - a, w = d - a, n = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x); the value n.x w.x + n.y w.y +
 *   n.z w.z, summed left to right.  WHEN ANY TWO OF THE FOUR POINTS ARE EQUAL (== on all three components) vol IS EXACTLY 0.
 *   Edge (p, q) MEETS triangle (a, b, c): sp = vol(a, b, c, p), sq = vol(a, b, c, q); no when sp and sq are both > 0, both < 0, both == 0 (the edge
 *   lies in the plane) or either is NaN; otherwise s1 = vol(p, q, a, b), s2 = vol(p, q, b, c), s3 = vol(p, q, c, a) and the edge meets the triangle
 *   iff all three are >= 0 or all three are <= 0.  Closed: touching counts.  A NaN fails every comparison.
 *   The MASK of the pair (query A = tris[i], scene B = the vertices of triangle j as the scene holds them): bit e (0..2): edge (A[e], A[(e + 1) % 3])
 *   meets B; bit 3 + e: edge (B[e], B[(e + 1) % 3]) meets A.
 *   The pair is REPORTED iff all 18 coordinates are finite, the FP64 bounding boxes of A and B overlap on every axis (closed <= on the coordinates
 *   as given) and the mask is not 0.  The box condition never changes a true answer; it makes the tree's cull conservative by construction.
 * Consequences: coplanar pairs are never reported; a triangle without area can be pierced by nothing, but its edges can pierce; a triangle never
 * crosses itself or an exact copy; two triangles of a mesh that share exactly one vertex are reported (a touch), two that share an edge are
 * reported unless they are coplanar in FP64; swapping the roles swaps the two halves of the mask.
 * Outputs: count[i] = the number of reported triangles, NOT capped by max_hits (K).  Row index[i][0..K): the first min(count, K) of them by
 * ascending TriangleIndex; mask[i][k]: the mask of that pair.  Every other slot of every row is written: index -1, mask 0.  max_hits == 0 is the
 * counting call.  Any of the three arrays may be NULL; all NULL: the call runs for the statistics.  An index row that the masks need and the caller
 * does not ask for is kept in the scene's first scratch set, in passes of at most 2^24 / K queries.
 * Options: SR_POINTS_COHERENT (bit 0): 64 consecutive queries are neighbours, the input order is kept.  SR_OVERLAP_ANY (4u; bit 1 is
 * SR_RAYS_ENDPOINTS elsewhere): count[i] is 1 if any triangle is reported and 0 otherwise, and the query stops at the first one; max_hits must be 0.
 * Targets: SR_MODE_BVH and SR_MODE_BRUTE, the same answers bit for bit.  SR_MODE_REF_TREE (a triangle lives in several leaves), SR_TARGET_ROOT | mode
 * (the extra primitives are not triangles with indices) and SR_TARGET_VOXELS are SR_ERR_UNSUPPORTED.
 * Routing in SR_MODE_BVH: a query is REGULAR when each of its vertices passes sr_closest_points' test (finite, within 2^20 box diagonals of the
 * centre).  The regular queries of a pass, ordered by the Morton cell of the centre of their box (SR_POINTS_COHERENT: input order), walk the own
 * BVH one lane each (k_ot_walk): the query's box relative to the root centre is rounded to fp32 and widened outward, and a child is entered iff it
 * overlaps the child's stored box on all three axes -- every leaf triangle whose FP64 box overlaps the query's is reached whatever the rounding
 * of the build or of a refit.  Every other query runs the per-record loop (k_ot_loop), as every query of SR_MODE_BRUTE does in
 * input order.
 * Refusals, in this order: a NULL scene, n < 0, NULL tris with n > 0, max_hits outside 0 .. SR_HITS_MAX, unknown option bits, SR_OVERLAP_ANY with
 * max_hits > 0: SR_ERR_INVALID_ARG; SR_TARGET_VOXELS, SR_TARGET_ROOT, SR_MODE_REF_TREE: SR_ERR_UNSUPPORTED; sr_trace_rays' own checks
 * (SR_ERR_NO_MODEL, SR_ERR_NOT_BUILT); a host-only scene: SR_ERR_NO_DEVICE.  A refusal writes nothing.  n == 0 that passes all of them: SR_OK,
 * nothing is touched.
 * State: as sr_near_triangles -- the call is ordered like a frame and rewrites no per-origin or per-light record, passes of at most 2^22 queries
 * (SR_DBG_BAND_SAMPLES: fewer) follow each other without the host waiting, a multi-device scene runs the call on devices[0].  The host variant
 * stages 72 n bytes in and 4 n + 5 K n bytes out through the scene's device buffers, blocks and fills sr_last_ray_stats; the device variant
 * enqueues on `hip_stream` without a host synchronisation.  Statistics: [0] = n; [1..3] = pairs on which the predicate ran, nodes and leaves
 * visited (pinned in brute force without SR_OVERLAP_ANY only: n x triangles, 0, 0); [4..] 0.
 * Out of scope: the intersection segment or contact points; penetration depth; excluding the neighbours in a self-query (the caller drops the
 * pairs that share vertices); the four-wide tree and persistent lanes; a split over devices; coplanar overlap. */
#define SR_OVERLAP_ANY 4u
int  sr_overlap_triangles(sr_scene*, int32_t target, int64_t n, const double* tris /* [n][3][3] */, int32_t max_hits /* K, 0..SR_HITS_MAX */,
                          uint32_t* count /* [n] or NULL */, int32_t* index /* [n][K] or NULL */, uint8_t* mask /* [n][K] or NULL */,
                          uint32_t options, uint64_t stats[4] /* or NULL */);
int  sr_overlap_triangles_device(sr_scene*, int32_t target, int64_t n, const double* d_tris, int32_t max_hits,
                                 uint32_t* d_count, int32_t* d_index, uint8_t* d_mask /* each may be NULL */,
                                 uint32_t options, void* hip_stream, uint64_t* d_stats /* device uint64[SR_STATS_COUNT] or NULL */);

/* ShadingMethod.IntersectRay's colour step in batch (ShadingMethod.cs:36-68 -> CalcLighting :110-177): for n recorded
 * intersections out[i] = ModulatePackedColor(color[i], (byte)(255 * intensity)) with the frame's transform and lights (only the
 * matrices, position_z, fov_depth, lights, ambient, shininess and the POINT_LIGHT / SPECULAR flags of `frame` are read).
 * Host arrays.  The decorator's arithmetic on its own -- Math.Pow included -- without a traversal in front of it. */
int  sr_shade_points(sr_scene*, const sr_frame* frame, int64_t n, const double* pos, const double* normal, const uint32_t* color,
                     uint32_t* out);

/* ShadowMethod.IntersectRay's step in batch (ShadowMethod.cs:103-119, 144-179 TraceRaysForSoftShadows): the soft shadow of n caller-given
 * surface points, through the stage a shadowed frame uses (packet shaft walk, per-light penumbra planes, fp32 classification with FP64
 * fallback).  out[i] = ModulatePackedColor(color[i], (byte)(escapes_i / (double)S * 255)), S = frame->shadow_samples (0 => 100), escapes_i =
 * the S sample rays towards pos[i] + normal[i] * 0.001 -- point or directional light, the seed's offset table or area_light_offsets -- that are
 * not blocked (blocked: a hit with rayFrac <= 1.0) by the frame's root geometry: the extra geometry plus the model in trace_mode.  pos and
 * normal are [n][3] in model space; the normal is used as given (not normalised, no facing test; zero is legal).  color == NULL: every point is
 * 0xFFFFFFFF.  out may alias color.  Only the modulated colour is returned, which is what the decorator produces.
 * Read from `frame`: inv_transform, light_pos_view, light_dir_view, SR_F_POINT_LIGHT, shadow_samples, random_seed, area_light_offsets,
 * trace_mode and the library options SR_F_PER_LANE_SHADOWS, SR_F_LITERAL_SECONDARY, SR_F_PRIMARY_STATS_ONLY; SR_F_SHADOWS is implied; the
 * camera fields are validated as for a frame and otherwise unused.
 * Refused, in this order: n < 0, a NULL pos / normal / out with n > 0, a NULL frame or scene, unknown option bits: SR_ERR_INVALID_ARG; what
 * names no step of ShadowMethod on a bare point -- SR_F_STATIC_SHADOWS, SR_F_AMBIENT_OCCLUSION, SR_F_PATH_TRACING, SR_F_VOXELS,
 * SR_F_LIGHT_FIELD, SR_F_SINGLE_KERNEL, max_bounces > 0, strip_count > 0: SR_ERR_UNSUPPORTED; then sr_render's validation of the frame and its
 * trace mode (SR_ERR_NOT_BUILT ...); then a host-only scene: SR_ERR_NO_DEVICE.  n == 0 that passes these checks: SR_OK, nothing is touched.
 * A point never reaches a walk when its probe end E' = pos + normal * 0.001 is not finite: a NaN component of E' -- no geometry answers a
 * ray with a NaN component -- lets all S samples escape; an infinite component does too as far as the model's triangles go, but the extra
 * geometry can block such a ray (the reference's Plane answers an infinite direction with rayFrac 0), so these points' samples are tested
 * against the extra primitives, with the reference's arithmetic, where the points are read.
 * SR_POINTS_COHERENT (options bit 0) is the caller's promise that 64 consecutive points are neighbours (the hit points of a tile, say): the
 * first shaft round takes one packet walk per 64 consecutive points of a pass in the order given.  Without it a pass is first ordered by
 * (cell of the point in the root box, octant of the normal; points outside clamp to the edge cells).  Results never depend on it; speed does.
 * Ordered like a frame (behind a frame of the scene in flight on any stream, the next frame behind it), on the scene's scratch, in passes
 * of at most 2^22 points that follow each other without the host waiting; a multi-device scene runs it on devices[0].  The host variant
 * blocks and leaves the shadow stage's counters in sr_last_ray_stats ([0..3] are 0, [4..] as for a frame, all 0 with
 * SR_F_PRIMARY_STATS_ONLY); the device variant takes device arrays, enqueues on `hip_stream` without a host synchronisation and writes the
 * counters to d_stats when given. */
#define SR_POINTS_COHERENT 1u
int  sr_shadow_points(sr_scene*, const sr_frame* frame, int64_t n, const double* pos, const double* normal, const uint32_t* color /* or NULL */,
                      uint32_t* out, uint32_t options);
int  sr_shadow_points_device(sr_scene*, const sr_frame* frame, int64_t n, const double* d_pos, const double* d_normal,
                             const uint32_t* d_color /* or NULL */, uint32_t* d_out, uint32_t options, void* hip_stream,
                             uint64_t* d_stats /* device uint64[SR_STATS_COUNT] or NULL */);

/* ShadowMethod.IntersectRay's static branch in batch (rayTraceShadowsStatic; ShadowMethod.cs:75-83, 106-112, Texture3DCache.Sample): the n
 * caller-given surface points go, IN INPUT ORDER, through the scene's static shadow cache -- the one static frames fill and read
 * (sr_get_shadow_cache / sr_set_shadow_cache).  Per point: its cell is (int)((p + 0.5) * 127) per axis, clamped to 0 .. 127 (a point outside
 * the unit cube takes the edge cell, where the reference asserts; a NaN coordinate takes index 0), [x][y][z] order.  Point i GENERATES iff its
 * cell is empty when the call starts and no point j < i of the call has the same cell; a generator stores
 * (byte)(escapes / (double)S * 254 + 1), 0 replaced by 1, where S = frame->shadow_samples (0 => 100) and `escapes` is exactly sr_shadow_points'
 * count for that point (E' = pos + normal * 0.001, the normal as given; point or directional light; the seed's offset table or
 * area_light_offsets; blocked = a hit with rayFrac <= 1.0 in the frame's root geometry; a NaN component of E': all S escape, byte 255; an
 * infinite component: only the extra primitives are asked).  There is no canonical point per cell: a cell's byte is the shadow of whichever
 * point and normal asked first, so this call is also how a host bakes the cache ahead of time.
 * amount[i] = the byte of point i's cell, out[i] = ModulatePackedColor(color[i], amount[i]); color == NULL: every point is 0xFFFFFFFF; out may
 * alias color; out and amount are each optional, but not both NULL with n > 0.  *generators (or NULL) receives the number of generators.  A
 * batch split over several calls equals the one call bit for bit: the cache carries the state.
 * Read from `frame`: what sr_shadow_points reads; SR_F_SHADOWS | SR_F_STATIC_SHADOWS are implied; concurrency is not read (a batch is one
 * block); the camera fields are validated as for a frame and otherwise unused; shadow_samples is whatever a static frame accepts (above 128 a
 * static frame leaves the shaft path, and so does this call).  options: SR_POINTS_COHERENT, which here speaks of the generators of a pass in
 * input order.
 * Refused, in this order: n < 0, a NULL pos / normal with n > 0, both outputs NULL with n > 0, a NULL scene or frame, unknown option bits:
 * SR_ERR_INVALID_ARG; SR_F_AMBIENT_OCCLUSION, SR_F_PATH_TRACING, SR_F_VOXELS, SR_F_LIGHT_FIELD, SR_F_SINGLE_KERNEL, max_bounces > 0,
 * strip_count > 0: SR_ERR_UNSUPPORTED; then sr_render's validation of the frame and its trace mode; then a host-only scene: SR_ERR_NO_DEVICE.
 * n == 0 that passes these checks: SR_OK, nothing is touched, *generators = 0.
 * Ordered like a frame (behind a frame of the scene in flight on any stream, the next frame behind it), on the scene's scratch, in passes of
 * at most 2^22 points (SR_DBG_BAND_SAMPLES: fewer) that follow each other without the host waiting: a pass finds the bytes of the passes
 * before it.  A multi-device scene runs it on devices[0], where the cache lives.  The host variant stages, blocks and fills
 * sr_last_ray_stats; the device variant takes device arrays (d_generators too), enqueues on `hip_stream` without a host synchronisation and
 * writes the counters to d_stats when given.  Statistics: [0..3] 0, [4..] what a static frame's shadow stage counts for the generators it is
 * handed (a generator whose E' is not finite, or which a directional light provably reaches -- sr_shadow_points' shortcut -- fires no ray
 * and counts nothing); all 0 with SR_F_PRIMARY_STATS_ONLY. */
int  sr_static_shadow_points(sr_scene*, const sr_frame* frame, int64_t n, const double* pos, const double* normal,
                             const uint32_t* color /* or NULL */, uint32_t* out /* or NULL */, uint8_t* amount /* or NULL */, uint32_t options,
                             uint64_t* generators /* or NULL */);
int  sr_static_shadow_points_device(sr_scene*, const sr_frame* frame, int64_t n, const double* d_pos, const double* d_normal,
                                    const uint32_t* d_color, uint32_t* d_out, uint8_t* d_amount, uint32_t options, void* hip_stream,
                                    uint64_t* d_generators /* or NULL */, uint64_t* d_stats /* device uint64[SR_STATS_COUNT] or NULL */);

/* AmbientOcclusionMethod.IntersectRay's step in batch (AmbientOcclusionMethod.cs:65-99, AmbientOcclusion.cs:101-230): the occlusion byte of n
 * caller-given surface points -- what the decorator leaves when it is applied to the n intersections IN INPUT ORDER by one RenderContext whose
 * Random is Random(frame->random_seed) advanced by 300 * first_generator draws.  Per point: pc = pos clamped per axis to [-0.5, 0.5] (a NaN
 * component becomes 0.5; the reference would throw there), its cell in the 128^3 texture, and -- where the point GENERATES -- 100 probes from
 * pc + normal * 0.001 with directions (2 u0 - 1, 2 u1 - 1, 2 u2 - 1), not normalised, negated when d . n < 0, through the frame's root geometry
 * (the extra geometry plus the model in trace_mode); a probe escapes on no hit or rayFrac > 2.0; the byte is (byte)(escapes / 100.0 * 254 + 1).
 * Generator number g of the call, counted in input order, uses draws 300 (first_generator + g) .. + 299.  The normal is used as given (not
 * normalised, no facing test; zero is legal).
 * Cached (the default; the scene's AO cache, the one AO frames use): point i generates iff its cell is empty when the call starts and no point
 * j < i of the call has the same cell; the byte is stored in the cache and every point's amount is its cell's byte.  SR_F_AO_UNCACHED in
 * frame->flags: every point generates, the cache is neither read nor written.
 * amount[i] = the byte, out[i] = ModulatePackedColor(color[i], amount[i]); color == NULL: every point is 0xFFFFFFFF; out may alias color; out
 * and amount are each optional, but not both NULL with n > 0.  *generators (or NULL) receives the number of generators: a caller that
 * splits a batch passes first_generator + *generators to the next call, and the split calls equal the one call bit for bit.
 * A probe origin that is not finite can only come from the normal and never reaches a walk: a NaN component lets all 100 probes escape; an
 * infinite component does as far as the model goes, and the extra primitives are asked with the reference's arithmetic against the limit
 * 2.0.  Either way the point stays a generator like any other: it consumes its 300 draws and fills its cell.
 * Read from `frame`: random_seed, trace_mode, SR_F_AO_UNCACHED and SR_F_PRIMARY_STATS_ONLY; SR_F_AMBIENT_OCCLUSION is implied; concurrency is
 * not read (a batch is one block); the camera fields are validated as for a frame and otherwise unused.
 * Refused, in this order: n < 0, a NULL pos / normal with n > 0, both outputs NULL with n > 0, a NULL scene or frame, options != 0 (reserved),
 * first_generator + n > 2^40: SR_ERR_INVALID_ARG; SR_F_STATIC_SHADOWS, SR_F_PATH_TRACING, SR_F_VOXELS, SR_F_LIGHT_FIELD, SR_F_SINGLE_KERNEL,
 * max_bounces > 0, strip_count > 0: SR_ERR_UNSUPPORTED; then sr_render's validation of the frame and its trace mode; then a host-only scene:
 * SR_ERR_NO_DEVICE.  n == 0 that passes these checks: SR_OK, nothing is touched, *generators = 0.
 * Ordered like a frame (behind a frame of the scene in flight on any stream, the next frame behind it), on the scene's scratch, in passes of
 * at most 2^17 points (SR_DBG_BAND_SAMPLES: fewer) that follow each other without the host waiting: the 300 draws per generator are made on
 * the device, from jump-ahead states of System.Random (sr_net_random_jump).  A multi-device scene runs it on devices[0], where the cache lives.
 * The host variant stages, blocks and fills sr_last_ray_stats; the device variant takes device arrays (d_generators too), enqueues on
 * `hip_stream` without a host synchronisation and writes the counters to d_stats when given.  Statistics: [0..3] 0, [4] 100 per generator,
 * [5..7] what the probe walks count; all 0 with SR_F_PRIMARY_STATS_ONLY. */
int  sr_ao_points(sr_scene*, const sr_frame* frame, int64_t n, const double* pos, const double* normal, const uint32_t* color /* or NULL */,
                  uint32_t* out /* or NULL */, uint8_t* amount /* or NULL */, uint64_t first_generator, uint32_t options,
                  uint64_t* generators /* or NULL */);
int  sr_ao_points_device(sr_scene*, const sr_frame* frame, int64_t n, const double* d_pos, const double* d_normal, const uint32_t* d_color,
                         uint32_t* d_out, uint8_t* d_amount, uint64_t first_generator, uint32_t options, void* hip_stream,
                         uint64_t* d_generators /* or NULL */, uint64_t* d_stats /* device uint64[SR_STATS_COUNT] or NULL */);
/* diagnostics: the next 55 InternalSample() values of Random(seed) after `skip` draws, computed with the jump-ahead sr_ao_points uses
 * (x^skip mod x^55 + x^21 - 1 over GF(2^31 - 1), applied to the first outputs).  SR_ERR_UNSUPPORTED: one of the seed's first 55 outputs
 * lies outside [0, 2^31 - 2] and the generator is not that recurrence (no such seed is known; sr_ao_points then draws on the host) */
int  sr_net_random_jump(int32_t seed, uint64_t skip, int32_t out[55]);

/* PathTracingMethod.IntersectRay's step in batch (PathTracingMethod.cs:51-76; Renderer.cs:1606-1638 puts it between shading and shadows): the
 * one-bounce diffuse term of n caller-given surface points -- what the decorator leaves when it is applied to the n intersections IN INPUT
 * ORDER by one RenderContext whose Random is Random(frame->random_seed) advanced by 3 * first_sample draws.  Point i uses draws
 * 3 (first_sample + i) .. + 2 (every point is a hit): u = InternalSample * (1.0 / 2147483647.0), d = (2 u0 - 1, 2 u1 - 1, 2 u2 - 1), negated
 * when d . normal[i] < 0.0, then multiplied by 1 / length; dirs[i] = d.  The second ray goes from pos[i] + normal[i] * 0.001 along d through
 * the frame's root geometry (the extra geometry plus the model in trace_mode); incoming[i] = that hit's colour, shaded with the frame's
 * transform and lights when SR_F_SHADING is set, 0 (Color.Black) on a miss; out[i], per channel, = incoming / 255.0 * (normal[i] . d) +
 * color[i] / 255.0, all three scaled by 1 / sqrt(r^2 + g^2 + b^2) when one exceeds 1.0, stored as 0xFF000000 | (byte)(r * 255) << 16 | ...
 * (truncating; NaN gives 0).  FP64 without contraction, in a path-traced frame's operand order.  color[i] is used as given (a caller who
 * wants the frame's result shades it first: sr_shade_points); color == NULL: every point is 0xFFFFFFFF; out may alias color.  The normal is
 * used as given (not normalised, no facing test; zero is legal).  out, incoming and dirs are each optional, but not all NULL with n > 0;
 * with only dirs asked for nothing is traced.  A split batch continues the sequence bit for bit: the next call passes first_sample + n;
 * averaging several rounds is the caller's loop over first_sample.
 * A second-ray origin that is not finite never reaches a walk: a NaN component -- no hit; an infinite component -- no model triangle
 * answers, the extra primitives are asked with the reference's arithmetic.  The colour step then runs on whatever IEEE gives (a NaN normal
 * on a miss: 0xFF000000).
 * Read from `frame`: random_seed, trace_mode, SR_F_SHADING and everything sr_shade_points reads when it is set, SR_F_PRIMARY_STATS_ONLY;
 * SR_F_PATH_TRACING is implied; concurrency is not read (a batch is one block); the camera fields are validated as for a frame and
 * otherwise unused.
 * Refused, in this order: n < 0, a NULL pos / normal with n > 0, all three outputs NULL with n > 0, a NULL scene or frame, options != 0
 * (reserved), first_sample + n > 2^40: SR_ERR_INVALID_ARG; SR_F_SHADOWS (dynamic or static), SR_F_AMBIENT_OCCLUSION, SR_F_VOXELS,
 * SR_F_LIGHT_FIELD, SR_F_SINGLE_KERNEL, max_bounces > 0, strip_count > 0: SR_ERR_UNSUPPORTED; then sr_render's validation of the frame and
 * its trace mode; then a host-only scene: SR_ERR_NO_DEVICE.  n == 0 that passes these checks: SR_OK, nothing is touched.
 * Ordered like a frame (behind a frame of the scene in flight on any stream, the next frame behind it), on the scene's scratch, in passes
 * of at most 2^22 points (SR_DBG_BAND_SAMPLES: fewer) that follow each other without the host waiting: the host knows where every pass
 * starts in the sequence and jumps there (sr_net_random_jump), the draws themselves are made on the device.  (A seed for which
 * sr_net_random_jump answers SR_ERR_UNSUPPORTED -- none is known -- draws on the host, one draw after the other from the seed on, and waits
 * once per pass; first_sample + n > 2^30 is then SR_ERR_UNSUPPORTED.)  A multi-device scene runs it
 * on devices[0].  The host variant stages, blocks and fills sr_last_ray_stats; the device variant takes device arrays, enqueues on
 * `hip_stream` without a host synchronisation and writes the counters to d_stats when given.  Statistics: [0..3] 0, [4..7] (and [20..23]
 * in SR_MODE_BVH) what a path-traced frame counts for the second rays of the same points; all 0 with SR_F_PRIMARY_STATS_ONLY. */
int  sr_path_points(sr_scene*, const sr_frame* frame, int64_t n, const double* pos, const double* normal, const uint32_t* color /* or NULL */,
                    uint32_t* out /* or NULL */, uint32_t* incoming /* or NULL */, double* dirs /* [n][3] or NULL */, uint64_t first_sample,
                    uint32_t options);
int  sr_path_points_device(sr_scene*, const sr_frame* frame, int64_t n, const double* d_pos, const double* d_normal, const uint32_t* d_color,
                           uint32_t* d_out, uint32_t* d_incoming, double* d_dirs, uint64_t first_sample, uint32_t options, void* hip_stream,
                           uint64_t* d_stats /* device uint64[SR_STATS_COUNT] or NULL */);

/* The same step with every array in DEVICE memory on the scene's device (a multi-device scene: devices[0]), enqueued on `hip_stream` without
 * a host synchronisation and without the staging copies.  Validation as sr_shade_points; n == 0: SR_OK. */
int  sr_shade_points_device(sr_scene*, const sr_frame* frame, int64_t n, const double* d_pos, const double* d_normal, const uint32_t* d_color,
                            uint32_t* d_out, void* hip_stream);

/* The frame G-buffer: what the primary stage of a frame answers per camera sample, before any decorator.  Sample i of the frame is
 * ((row - a) * width + col) * n*n + subX * n + subY, a..b the frame's row range clamped to the surface as sr_render clamps it and
 * n = sub_pixel_res: the reference's scan order (Renderer.cs:1717-1790).  sr_frame_sample_count is the number S of samples,
 * rows x width x n^2 (0 for start_row > end_row after clamping or a NULL frame); pure, like sr_frame_pixel_count.  All arrays are SoA
 * with sr_trace_rays' shapes, [S][3] doubles and [S] scalars.
 * starts / dirs: the sample's camera ray in model space, exactly what the frame's primary stage traces (the one-sample fast path, the
 * sub-pixel form, the focal-blur form); the direction is not normalised.  The other arrays: IRayIntersectable.IntersectRay of the frame's root
 * geometry -- the extra geometry plus the model in trace_mode -- for that ray, with sr_trace_rays' conventions: a miss writes hit 0, zeros and
 * tri_index -1; a hit on extra geometry has tri_index -1 and the primitive's colour; color is the unshaded surface colour.  Every output
 * pointer may be NULL and is then neither computed for nor written; all NULL is legal (the call then runs for the statistics).
 * Read from the frame: the surface, the rows, sub_pixel_res, SR_F_FOCAL_BLUR with its fields, the matrices, position_z, fov_depth and
 * trace_mode; the library options SR_F_PRIMARY_STATS_ONLY and SR_F_NO_SPLIT are accepted and have no effect.  The decorator switches are
 * NOT read -- SR_F_SHADING, SR_F_SHADOWS, SR_F_STATIC_SHADOWS, SR_F_AMBIENT_OCCLUSION, SR_F_AO_UNCACHED, SR_F_PATH_TRACING, the lights,
 * max_bounces -- so a frame about to be passed to sr_render can be passed as it is.
 * Refused, in this order: a NULL scene or frame: SR_ERR_INVALID_ARG; what replaces the root geometry or the primary stage -- SR_F_VOXELS,
 * SR_F_LIGHT_FIELD, SR_F_SINGLE_KERNEL, strip_count > 0: SR_ERR_UNSUPPORTED; then sr_render's validation of the frame and its trace mode
 * (SR_ERR_INVALID_ARG, SR_ERR_NO_MODEL, SR_ERR_NOT_BUILT); then a host-only scene: SR_ERR_NO_DEVICE.  An empty row range that passes the
 * first three: SR_OK, nothing is touched (like sr_shadow_points' n == 0, before a device is asked for).
 * The walk is the frame's: in SR_MODE_BVH with a common ray origin the packet walk on the camera-ordered four-wide tree (one traversal per
 * 8x8-pixel tile, camera-cone records, facing partition), per-lane walks with focal blur, in the other modes and under
 * SR_DBG_PER_LANE_PRIMARY / SR_DBG_BVH2_PACKETS (binary-tree packets); row bands as a frame's (SR_DBG_BAND_SAMPLES).
 * Ordered like a frame (behind a frame of the scene in flight on any stream, the next frame behind it); a multi-device scene runs it on
 * devices[0] and sr_last_frame_parts then reads 1.  The device variant enqueues on `hip_stream` without a host synchronisation; the host
 * variant stages through the scene's device buffers, blocks and fills sr_last_ray_stats.  Statistics: [0..3] the primary counters as a frame
 * counts them (SR_MODE_REF_TREE / SR_MODE_BRUTE: those of sr_render of the same frame without decorators; own BVH: what a wave fetched),
 * [4..] 0. */
int64_t sr_frame_sample_count(const sr_frame*);
int  sr_render_hits(sr_scene*, const sr_frame* frame, double* starts, double* dirs, uint8_t* hit, double* ray_frac, double* pos,
                    double* normal, uint32_t* color, int32_t* tri_index, uint64_t stats[4] /* or NULL */);
int  sr_render_hits_device(sr_scene*, const sr_frame* frame, double* d_starts, double* d_dirs, uint8_t* d_hit, double* d_ray_frac,
                           double* d_pos, double* d_normal, uint32_t* d_color, int32_t* d_tri_index, void* hip_stream,
                           uint64_t* d_stats /* device uint64[SR_STATS_COUNT] or NULL */);

/* n NextDouble() of new System.Random(seed) after `skip` samples have been drawn (Next() and NextDouble() consume one each):
 * hosts regenerate the reference's seeded test inputs with it (rays that continue the triangle stream, SpatialSubdivisionTests.cs:141,225) */
void sr_net_random_doubles(int32_t seed, int64_t skip, int64_t n, double* out);

/* Instance.InitRender matrices (Instance.cs:134-135, Matrix.cs:74-169): T = Trans(P)*Roll*Pitch*Yaw,
 * T^-1 = Yaw(-)*Pitch(-)*Roll(-)*Trans(-P); rows 0..2, row-major 3x4. */
void sr_instance_matrices(const double position[3], double yaw, double pitch, double roll,
                          double transform[12], double inv_transform[12]);
/* Renderer.fieldOfViewDepth (Renderer.cs:97-101) */
double sr_default_fov_depth(void);
/* ShadowMethod ctor (ShadowMethod.cs:63-73) with new Random(seed) (Renderer.cs:1624): out[count][3] */
void sr_area_light_offsets(int32_t seed, int32_t count, double* out3);

/* Model.Load3ds + Model.PostProcessGeometry (Model.cs:522-653,750-831; 3dsLoader/ThreeDSFile.cs:132-662):
 * parses a .3DS image and fills the scene's triangles / colours / box (= sr_set_triangles).  The counts
 * and the arrays can be read back with sr_get_triangles. */
int  sr_load_3ds(sr_scene*, const uint8_t* data, size_t len);
int64_t sr_num_triangles(const sr_scene*);
int  sr_get_triangles(const sr_scene*, double* v9, uint32_t* argb, double box_min[3], double box_max[3]);

/* Device time of the library's kernels (opt-in: sr_debug_set(SR_DBG_KERNEL_TIMING, 1)), measured with one HIP event pair per launch on the launch stream and
 * accumulated since sr_reset_kernel_times() (or scene creation): out[i] = {static kernel name, total ms,
 * launches}.  sr_kernel_times waits for the recorded events.  Returns the number of entries (<= cap). */
typedef struct { const char* name; float ms; int32_t launches; } sr_kernel_time;
void sr_reset_kernel_times(sr_scene*);
int  sr_kernel_times(sr_scene*, sr_kernel_time* out, int32_t cap);

/* Ray statistics of the last sr_render(..., stats != NULL): [0..3] primary rays {rays, triangle/primitive tests, nodes
 * visited, leaf nodes visited} -- the reference's notions in SR_MODE_REF_TREE / SR_MODE_BRUTE; on the own BVH the primary walk is one
 * packet walk per 8x8-pixel tile and [1..3] count what a WAVE fetched: [1] 64-byte camera-cone records consulted, [2] 64-byte
 * nodes, [3] 128-byte FP64 triangle records; [4..7] the same for secondary (shadow) rays -- on the shaft path [6],[7] are the shaft
 * walks' nodes / leaves; [8] triangle records staged through LDS by k_shadow_test, [9] hit points it processed,
 * [10] fp32 slab records read by k_shaft, [11] hit points it walked, [12] (sample, triangle) pairs k_shadow_test classified
 * in fp32, [13] pairs it had to decide with the exact FP64 test, [14] / [15] the part of [6] / [10] that came from private per-lane
 * shaft walks (later rounds) rather than from the packet walk; [16..19] the exact fallback's any-hit rays on their own {rays,
 * FP64 triangle records tested, nodes fetched per lane, leaves} (also contained in [4..7]); [20..23] the same for the mirror
 * rays of the bounce pipeline (and for the second rays of a path-traced SR_MODE_BVH frame, which take the same walk; in every mode they
 * are counted in [4..7] unless SR_F_PRIMARY_STATS_ONLY is set; with SR_DBG_KERNEL_SWITCH 94 / 95 [22] and [23] hold the shadow classification's census
 * instead: hit points classified with / without the interior-triangle shortcut; with switch 98 [20..23] hold the umbra hints' census, see there).  These are the counters the roofline's algorithmic bytes are priced from (DESIGN.md "Measurement"). */
int  sr_last_ray_stats(const sr_scene*, uint64_t out[SR_STATS_COUNT]);

/* Seeded synthetic triangle soup = SpatialSubdivisionTests.MakeRandomTriangles
 * (Engine3D-Tests/Raytrace/SpatialSubdivisionTests.cs:397-411) driven by the System.Random port: per triangle
 * v1 = U[0,space)^3 + origin, v2 = v1 + U[0,extent)^3, v3 = v1 + U[0,extent)^3, colour = (uint)Next()
 * (opaque != 0: 0xFF000000 | low 24 bits).  Used by bench.py and the tests so that C#, the CPU checker and
 * the device regenerate identical inputs. */
void sr_make_random_triangles(int32_t seed, int64_t n, double space, double extent, double origin, int32_t opaque,
                              double* v9, uint32_t* argb);

/* ---- the row-strip gather over RCCL / xGMI, native (replaces the TPL fan-out of Renderer.cs:1655-1680 across GPUs) ----
 * The frame's rows are dealt out in interleaved 16-row strips (strip s belongs to rank s % world); every rank renders its strips
 * into a compact buffer and ONE exchange step brings them to rank 0: grouped ncclSend (ranks 1..) / ncclRecv (rank 0) of
 * rows_r x W x 4 bytes each, followed on rank 0 by the row de-interleave (strided device copies) into the full surface.  No
 * reduction, no RNG: the frame does not depend on the split.  librccl is bound with dlopen at first use (a single-GPU host never
 * loads it; a process that already holds an RCCL -- PyTorch's -- keeps using that one); SR_ERR_UNSUPPORTED when it is absent.
 *
 * One process per GPU (no PyTorch needed): rank 0 calls sr_rccl_unique_id and hands the 128 bytes to the other ranks by whatever
 * means the host has (a file, a socket, MPI, a torch store); every rank calls sr_rccl_init(scene, id, world, rank) on its own
 * single-device scene (ncclCommInitRank on the scene's device), then per frame sr_rccl_render(scene, frame, d_full, stream):
 * renders this rank's strips of `frame` (strip_count must be 0: the split is the library's) and gathers; d_full (device memory,
 * W*H int32) is only written on rank 0 and may be NULL elsewhere.  sr_rccl_gather is the exchange step on its own, for a host
 * that rendered its strips itself (sr_frame.strip_rows = 16, strip_count = world, strip_index = rank) into d_strips.  Everything
 * is enqueued on `hip_stream`; consecutive frames of a scene must use the same stream.
 *
 * One process, several devices (sr_create_multi): sr_set_gather(scene, SR_GATHER_RCCL) makes sr_render_device gather the parts'
 * strips with the same grouped send / receive (ncclCommInitAll over the scene's devices, which must be distinct) instead of peer
 * copies -- SR_GATHER_COPY, the default: hipMemcpy2DAsync peer-to-peer where the devices allow it, pinned host staging where not.
 * sr_render (host surface) copies every part's strips over its own PCIe link either way. */
#define SR_RCCL_ID_BYTES 128
enum { SR_GATHER_COPY = 0, SR_GATHER_RCCL = 1 };
int  sr_rccl_unique_id(uint8_t out[SR_RCCL_ID_BYTES]);
int  sr_rccl_init(sr_scene*, const uint8_t id[SR_RCCL_ID_BYTES], int32_t world, int32_t rank);
int  sr_rccl_render(sr_scene*, const sr_frame*, void* d_full, void* hip_stream);
int  sr_rccl_gather(sr_scene*, const sr_frame*, const void* d_strips, void* d_full, void* hip_stream);
int  sr_set_gather(sr_scene* multi_device_scene, int32_t kind);

/* ---- surface passes that Renderer.Render() runs after the raytrace (Engine3D/Renderer.cs:765-767) ----
 * sr_post_process[_device]  = PostProcessImage's per-pixel colour functions (Renderer.cs:819-865, Surface.ApplyColorFunc
 *   Surface.cs:226-233), applied in place to `count` pixels.  `background_color` is Renderer.BackgroundColor (alpha
 *   masked off, Renderer.cs:304-320) and is only read by SR_STYLE_NEGATIVE.  The two depth styles are the reference's
 *   8-bit-alpha-depth twizzles (taken when depthBuffer && !depthBufferHires; the host decides).  Style.Normals reads the
 *   rasteriser's depth buffer and is outside the raytrace path: SR_ERR_UNSUPPORTED.
 * sr_anti_alias[_device]    = AntiAliasImage (Renderer.cs:937-978): src is (dst_width*resolution) x (dst_height*resolution),
 *   every destination pixel is the integer average of its resolution^2 source pixels per channel, alpha 255. */
enum {
    SR_STYLE_STANDARD = 0,       /* Style.Standard: nothing to do */
    SR_STYLE_COLOR_SHUFFLE = 1,  /* ZRGB -> 0GBR */
    SR_STYLE_NEGATIVE = 2,
    SR_STYLE_DEPTH_SMOOTH = 3,   /* ZRGB -> 0ZZZ */
    SR_STYLE_DEPTH_BANDED = 4    /* Z * 111 */
};
int  sr_post_process(sr_scene*, int32_t* pixels, int64_t count, int32_t style, uint32_t background_color);
int  sr_post_process_device(sr_scene*, void* d_pixels, int64_t count, int32_t style, uint32_t background_color, void* hip_stream);
int  sr_anti_alias(sr_scene*, const int32_t* src, int32_t dst_width, int32_t dst_height, int32_t resolution, int32_t* dst);
int  sr_anti_alias_device(sr_scene*, const void* d_src, int32_t dst_width, int32_t dst_height, int32_t resolution, void* d_dst,
                          void* hip_stream);

/* Test / experiment hooks of ONE scene.  The library never reads the process environment: a drop-in must not change its
 * schedule with the host's env.  value < 0 restores the default.  Used by tests/ and scripts/ only. */
enum {
    SR_DBG_BAND_SAMPLES   = 0,   /* samples per row band (default 16 Mi / 32 Mi): small values force several bands; also the cells
                                    per pass of sr_bake_light_field with shadows (default 2^22; whole origin patches, at least one) and the
                                    points per pass of sr_shadow_points and sr_static_shadow_points (default 2^22), of sr_ao_points (default and limit 2^17) and of sr_path_points (default and limit 2^22),
                                    and the rays per pass of sr_trace_origin_rays, of sr_occluded_rays, of sr_nearest_rays and of sr_light_field_rays (default and limit 2^22;
                                    sr_light_field_rays with interpolation and shadows together: 1/16 of the value, as a frame's bands) */
    SR_DBG_ROUND_CAP0     = 1,   /* candidate-list length of shaft round 1 (default 40, <= 64)                                 */
    SR_DBG_ROUND_CAP1     = 2,   /* ... of round 2 (default 64, <= 1024): tiny lists force round 2 and the exact fallback      */
    SR_DBG_SPLIT          = 3,   /* concurrent part-frame pipelines (default 2, <= 4)                                          */
    SR_DBG_FB_RAY_CAP     = 4,   /* capacity of the fallback ray list                                                          */
    SR_DBG_BVH_LEAF       = 5,   /* triangles per leaf of the own BVH, host and device build (default 4, 1..15); read by the next sr_build */
    SR_DBG_KERNEL_SWITCH  = 6,   /* A/B switch of single optimisations, same pixels (0 = production): 31 the bounce pipeline walks its rays in
                                    queue order (no per-level ray sort); 61 the camera-ordered node copy keeps (lo, hi) planes; 71 no facing
                                    partition (the packet walks see every record of a leaf); 72 the camera- / light-ordered node copies keep the base tree's
                                    boxes (not fitted to their live records), 73 / 74 only the camera / light copy is fitted, 75 .. 79 both on the lowest 1 .. 5
                                    levels of the wide tree only; 7 counts umbra decisions of the private shaft walk;
                                    32 a mirror-bounce level as ONE kernel (k_bounce) instead of prepare / walk / finish; 33 the second rays of a path-traced SR_MODE_BVH frame with
                                    private per-lane walks (k_pt_finish) instead of the mirror extension's prepare / walk route; 34 the ambient-occlusion probes of a
                                    SR_MODE_BVH frame as nearest-hit walks instead of any-hit walks with the limit 2.0; 35 sr_bake_light_field on a
                                    SR_MODE_BVH frame with one packet walk per wave of 64 same-origin canonical rays instead of private per-lane
                                    walks (same table; measured slower); 36 the shadow stage of a shadowed light-field frame's lazy fill with the
                                    packet shaft walk instead of private per-lane shaft walks (same table; measured slower); 37 sr_shadow_points queues a pass in input
                                    order whatever the options say (no ray sort); 38 sr_shadow_points runs the first shaft round with private per-lane walks instead of the
                                    packet walk (both: same output); 44 sr_ao_points makes every pass's draw table on the host, one draw after the
                                    other, and waits once per pass (same output; cross-check and baseline); 45 sr_path_points does the same, and then refuses first_sample + n > 2^30 with SR_ERR_UNSUPPORTED: the host draws its way to first_sample; 46 sr_occluded_rays walks a pass in input
                                    order whatever the options say (no ray sort); 47 sr_occluded_rays in SR_MODE_BVH answers every ray with a nearest-hit walk plus the
                                    comparison instead of the any-hit walk (both: same output); 100 + T (T in 0..63) also makes the any-hit launch of sr_occluded_rays run on
                                    persistent lanes that fetch new rays at T busy lanes (same output; faster on incoherent batches, slower on short coherent walks: DESIGN 5.28); 48 sr_nearest_rays walks a pass
                                    in input order whatever the options say (no ray sort); 49 sr_nearest_rays answers every ray with one private walk per lane (k_nr_lane) in input
                                    order, also in SR_MODE_BVH (same output; baseline and cross-check); 100 + T and 200 + K also set the refill threshold and the LDS
                                    stack levels of sr_nearest_rays' walk kernel, as the bounce walk reads them below; 50 sr_all_hits_rays walks a pass in input order whatever the options say
                                    (no ray sort); 51 sr_all_hits_rays answers every ray of SR_MODE_BVH with the per-record loop of its irregular rays (both: same output;
                                    cross-check); 52 sr_closest_points walks a pass in input order whatever the options say (no point sort); 53 sr_closest_points
                                    answers every point of SR_MODE_BVH with the per-record loop of its irregular points (both: same output; cross-check); 54 sr_near_triangles walks a pass in input order whatever the options say (no point sort); 55 sr_near_triangles
                                    answers every point of SR_MODE_BVH with the per-record loop of its irregular points (both: same output; cross-check); 56 sr_overlap_triangles walks a pass in input order whatever the options say (no sort); 57 sr_overlap_triangles
                                    answers every query of SR_MODE_BVH with the per-record loop of its irregular queries (both: same output; cross-check); 39 the apply kernel of an interpolating light-field frame (sr_set_light_field_interpolation) computes base cell and
                                    fractions again instead of taking them from the lookup kernel (same frame; measured slower); 100 + T: the walk kernel
                                    fetches new rays at T busy lanes (default 24); 200 + K: K stack levels per lane in LDS (default 24);
                                    81 the tile kernels with one workgroup per 16x16 tile (no persistent grid); 82 k_primary on the persistent grid
                                    too (its loop form spills registers: opt-in); 84 the persistent shaft walk hands its tiles out in natural order
                                    (no longest-first lists); 830 + n: n resident workgroups per CU for it; 840 + q: a walk is long at q / 4 x the
                                    mean; 63 the packet shaft walk's loop as it was before its scalar diet (the instantiations counted launches run; same frame,
                                    DESIGN 5.8); 630 + n: 830 + n with that loop; 91 the first classification round on k_shadow_cls instead of k_shadow_cls_g; 93 the shadow classification
                                    computes the per-sample box exits for every hit point (no shortcut for candidate lists whose triangles all lie
                                    inside the root box); 94 production path, and a frame rendered with ray statistics leaves the census of that
                                    shortcut in statistics [22] (hit points classified with the shortcut) and [23] (with the per-sample box exits)
                                    instead of the mirror rays' figures; 95 = 93 and 94 together; 96 the packet shaft walk filters its triangles with the
                                    TriSlab records (shaft_touches_wave) instead of the per-light penumbra planes (LightCone); 97 the persistent packet shaft walk without
                                    its umbra hints (no tile tries the leaf runs the previous frame left before it walks, none are left); 98 production path, and
                                    a frame rendered with ray statistics -- which otherwise walks without hints -- uses them and leaves in statistics [20] the walk
                                    length (2 per node step + 1 per triangle filter) of all tiles, [21] that of the tiles that ended with every valid lane in
                                    umbra, [22] the tiles that entered the walk with a lane finished by a hint, [23] the tiles that never took a node step, instead of
                                    the mirror rays' figures; 99 a tile tries its own hint only, not those of the other three tiles of its 16x16 parent; 41 a voxel walk on a grid of at most 64 reads the
                                    colour table instead of the occupancy bits in LDS; 42 a voxel walk on a grid above 64 reads the row-major
                                    occupancy bits in global memory, one level, instead of the two-level walk; 43 a triangle light-field frame
                                    (sr_set_light_field_triangles) lists the samples that need its third stage for a kernel of their own (k_lft_trace) instead of
                                    tracing them inside k_lft_hit (same frame and statistics; measured slower)                                                */
    SR_DBG_KERNEL_TIMING  = 7,   /* > 0: record a HIP event pair around every launch (sr_kernel_times); default off           */
    SR_DBG_EXACT_SHADOW_TESTS = 8, /* > 0: k_shadow_test decides every (sample, triangle) pair with the FP64 arithmetic (no
                                    fp32 classification): an independent schedule of the same result, kept as a cross-check */
    SR_DBG_PER_LANE_SHAFT = 9,   /* bit 0: first shaft round with private per-lane walks (k_shaft) instead of the wave-cooperative
                                    packet walk (k_shaft_pkt); bit 1: later rounds with private walks instead of one wave per hit
                                    point (k_shaft_coop): same lists up to order, same pixels; cross-checks                     */
    SR_DBG_PER_LANE_PRIMARY = 10, /* > 0: primary rays with private per-lane walks instead of the packet walk + camera-cone filter */
    SR_DBG_ROUND2_NODES   = 11,  /* node budget of a private shaft walk of the later rounds (0 = unlimited): walks that exceed it hand
                                    their undecided samples to the exact fallback */
    SR_DBG_BUILD_THREADS  = 12,  /* threads of the host BVH build (default: the host's cores, at most 16); read by the next sr_build    */
    SR_DBG_BVH2_PACKETS   = 13,  /* > 0: the packet walks (k_primary, first shaft round) on the binary tree with a per-step vote instead of
                                    the four-wide tree with per-frame ordered children: same pixels; cross-check and A/B measurement */
    SR_DBG_NO_PEER        = 14,  /* > 0 (multi-device scene): sr_render_device gathers every part's strips through pinned host staging, as it
                                    does for a part whose memory the first device cannot read; test hook for that path                 */
    SR_DBG_LITERAL_SHADOWS = 15, /* > 0: no shortcut for ShadowMethod -- a directional light's samples are traced one by one although all of
                                    them provably escape, and a SR_MODE_REF_TREE frame traces its shadow rays through the reference tree
                                    (as with SR_F_LITERAL_SECONDARY); cross-checks of both shortcuts                                  */
    SR_DBG_AO_TABLE_BYTES = 16,  /* > 0: the limit of an ambient-occlusion frame's draw table in bytes (default 256 MiB): small values let a small frame
                                    reach the refusal                                                                                  */
    SR_DBG_COUNT          = 17
};
int  sr_debug_set(sr_scene*, int32_t key, int64_t value);

/* Diagnostics only: the pipeline's device counters of the last frame, summed over its concurrent part-frame pipelines (last row band of each)
 * {hit-queue entries (on the shaft path: the padded tile-queue slot count, not the hits), per-lane shadow work head, hit points that needed the long (round-2) candidate list,
 *  hit points sent to the exact per-lane fallback, fallback work head,
 *  then host bookkeeping of the last frame: [5] the axes on which the ordered node copies the frame walked hold (near, far) planes
 *  (bits 0-2: the light-ordered copy of the shaft walk, bits 4-6: the camera-ordered copy of the packet primary walk; or-ed over the
 *  parts of a multi-device scene), [6] launches of the shaft walk in its persistent form, [7] those of them that walked the longest-first
 *  tile order an earlier frame's walk lengths made}. */
int  sr_debug_counters(sr_scene*, uint32_t out[8]);

const char* sr_last_error(void);
int32_t     sr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
