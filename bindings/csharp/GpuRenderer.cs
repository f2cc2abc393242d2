// GpuRenderer.cs -- P/Invoke binding of libsoftray_hip.so (include/softray.h) for the reference's C# host.
//
// SOURCE ONLY: the build image has no C# toolchain (no dotnet / mono / csc), so nobody compiles this file here; it is the
// binding a maintainer of voidstar69/softray adds to Engine3D (INTEGRATION.md shows where Renderer.cs calls it).  What WAS
// checked: every member of the reference it touches, against the reference sources --
//   Model.Triangles is ICollection<Triangle> (enumerated, never indexed), Model.Vertices[i].pos, Triangle.vertexIndex1..3,
//   Triangle.diffuseMaterial, Model.Min / Max                                  Engine3D/Model.cs:16,44-46,53,137-138,192-194
//   Surface.PackColorAndAlpha(Color, double)                                    Engine3D/Surface.cs:131
//   Instance.Position, Matrix this[row, col]                                    Engine3D/Instance.cs:47, Matrix.cs:16
//   GeometryCollection.Count / this[int]                                        Engine3D/Raytrace/GeometryCollection.cs:16,24
//   Raytrace.Triangle.Vertex1..3, .Color (uint)                                 Engine3D/Raytrace/Triangle.cs:59-67
//   Plane.Normal, Plane.DistanceToOrigin                                        Engine3D/Raytrace/Plane.cs:40,52
// and the FIVE accessors the reference lacks and INTEGRATION.md adds (private state the native side needs):
//   Sphere.Center, Sphere.Radius, Sphere.PackedColor, Plane.PackedColor, Instance.Transform / Instance.InverseTransform.
// The struct layouts mirror include/softray.h field for field (LayoutKind.Sequential, natural alignment); the byte offsets in
// the comments are the ones the header asserts at compile time (tests/test_abi.py compares them with this file).
//
// There is one entry point per Renderer call site: Upload (PreCalculate), SetExtraGeometry (ExtraGeometryToRaytrace),
// Render (RaytraceGeometry), PostProcess / AntiAlias (the two surface passes of Render()), Dispose.
using System;
using System.Runtime.InteropServices;

namespace Engine3D.Hip
{
    [StructLayout(LayoutKind.Sequential)]
    public struct SrPrim                     // sr_prim, 80 bytes
    {
        /* @0 */ public int kind;            // 0 Sphere {centre, radius}, 2 Triangle {v1, v2, v3}, 3 Plane {unit normal, originDist}
        /* @4 */ public uint argb;
        /* @8 */ [MarshalAs(UnmanagedType.ByValArray, SizeConst = 9)] public double[] p;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SrFrame                    // sr_frame, 368 bytes
    {
        /* @0   */ public int width;
        /* @4   */ public int height;
        /* @8   */ public int start_row;
        /* @12  */ public int end_row;
        /* @16  */ public int sub_pixel_res;
        /* @20  */ public uint background_argb;
        /* @24  */ public uint flags;
        /* @28  */ public int random_seed;
        /* @32  */ public int shadow_samples;
        /* @36  */ public int trace_mode;
        /* @40  */ public int strip_rows;
        /* @44  */ public int strip_count;
        /* @48  */ public int strip_index;
        /* @52  */ public int max_bounces;
        /* @56  */ public int concurrency;
        /* @60  */ public int reserved0;
        /* @64  */ [MarshalAs(UnmanagedType.ByValArray, SizeConst = 12)] public double[] transform;
        /* @160 */ [MarshalAs(UnmanagedType.ByValArray, SizeConst = 12)] public double[] inv_transform;
        /* @256 */ public double position_z;
        /* @264 */ public double fov_depth;
        /* @272 */ public double focal_depth;
        /* @280 */ public double focal_blur_strength;
        /* @288 */ public double ambient;
        /* @296 */ public double shininess;
        /* @304 */ [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public double[] light_dir_view;
        /* @328 */ [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public double[] light_pos_view;
        /* @352 */ public double reflectivity;
        /* @360 */ public IntPtr area_light_offsets;   // double[shadow_samples][3] made with the REAL System.Random, or IntPtr.Zero
    }
    // ByValArray fields of a struct passed by `ref` are marshalled inline (the marshaller copies the managed arrays into the
    // 368-byte native image and back): all five arrays must be non-null and exactly SizeConst long, which Render() guarantees.

    internal static class Native
    {
        const string Lib = "softray_hip";
        [DllImport(Lib)] public static extern int sr_create(int device, out IntPtr scene);
        [DllImport(Lib)] public static extern int sr_create_multi([In] int[] devices, int n, out IntPtr scene);
        [DllImport(Lib)] public static extern int sr_last_frame_parts(IntPtr scene);
        [DllImport(Lib)] public static extern int sr_set_gather(IntPtr scene, int kind);                  // 0 peer copies (default), 1 grouped ncclSend / ncclRecv
        [DllImport(Lib)] public static extern int sr_render_device(IntPtr scene, ref SrFrame frame, IntPtr dPixels, IntPtr hipStream, IntPtr dStats);
        [DllImport(Lib)] public static extern void sr_destroy(IntPtr scene);
        [DllImport(Lib)] public static extern int sr_set_triangles(IntPtr scene, double[] v9, uint[] argb, long n, double[] boxMin, double[] boxMax);
        [DllImport(Lib)] public static extern int sr_set_triangles_device(IntPtr scene, IntPtr dV9, IntPtr dArgb, long n, double[] boxMin, double[] boxMax, IntPtr hipStream);
        [DllImport(Lib)] public static extern int sr_refit_triangles_device(IntPtr scene, IntPtr dV9, IntPtr dArgb, long n, double[] boxMin, double[] boxMax, IntPtr hipStream);
        [DllImport(Lib)] public static extern int sr_set_extra_geometry(IntPtr scene, [In] SrPrim[] prims, int n);
        [DllImport(Lib)] public static extern int sr_build(IntPtr scene, uint modes, int maxDepth, int maxPerLeaf);
        [DllImport(Lib)] public static extern int sr_tree_stats(IntPtr scene, [Out] int[] out4);
        [DllImport(Lib)] public static extern int sr_render(IntPtr scene, ref SrFrame frame, [In, Out] int[] pixels, [Out] ulong[] stats4);
        [DllImport(Lib)] public static extern int sr_reset_shadow_cache(IntPtr scene);
        [DllImport(Lib)] public static extern int sr_reset_ao_cache(IntPtr scene);
        [DllImport(Lib)] public static extern int sr_get_ao_cache(IntPtr scene, [Out] byte[] out128Cubed);
        [DllImport(Lib)] public static extern int sr_set_ao_cache(IntPtr scene, [In] byte[] in128Cubed);
        [DllImport(Lib)] public static extern int sr_set_light_field_res(IntPtr scene, int n);
        [DllImport(Lib)] public static extern int sr_get_light_field_res(IntPtr scene);
        [DllImport(Lib)] public static extern int sr_set_voxel_res(IntPtr scene, int n);
        [DllImport(Lib)] public static extern int sr_get_voxel_res(IntPtr scene);
        [DllImport(Lib)] public static extern int sr_reset_light_field(IntPtr scene);
        [DllImport(Lib)] public static extern int sr_set_light_field_shadows(IntPtr scene, int on);
        [DllImport(Lib)] public static extern int sr_get_light_field_shadows(IntPtr scene);
        [DllImport(Lib)] public static extern int sr_set_light_field_interpolation(IntPtr scene, int on);
        [DllImport(Lib)] public static extern int sr_get_light_field_interpolation(IntPtr scene);
        [DllImport(Lib)] public static extern int sr_set_light_field_triangles(IntPtr scene, int on);
        [DllImport(Lib)] public static extern int sr_get_light_field_triangles(IntPtr scene);
        [DllImport(Lib)] public static extern int sr_get_light_field_tris(IntPtr scene, [Out] uint[] entries, ulong first, ulong count);
        [DllImport(Lib)] public static extern int sr_set_light_field_tris(IntPtr scene, [In] uint[] entries, ulong first, ulong count);
        [DllImport(Lib)] public static extern long sr_tree_handle_leaf(IntPtr scene, long tri, [Out] double[] box, [Out] int[] members, long cap);
        [DllImport(Lib)] public static extern int sr_light_field_coords(IntPtr scene, long n, [In] double[] starts, [In] double[] dirs, [Out] double[] coords, [Out] byte[] inside);
        [DllImport(Lib)] public static extern int sr_get_light_field(IntPtr scene, [Out] uint[] entries, ulong first, ulong count);
        [DllImport(Lib)] public static extern int sr_set_light_field(IntPtr scene, [In] uint[] entries, ulong first, ulong count);
        [DllImport(Lib)] public static extern int sr_light_field_rays(IntPtr scene, ref SrFrame frame, long n, [In] double[] starts, [In] double[] dirs, [Out] uint[] result, [Out] byte[] inside, uint options, out ulong filled);
        [DllImport(Lib)] public static extern int sr_light_field_rays_device(IntPtr scene, ref SrFrame frame, long n, IntPtr dStarts, IntPtr dDirs, IntPtr dOut, IntPtr dInside, uint options, IntPtr hipStream, IntPtr dFilled, IntPtr dStats);
        [DllImport(Lib)] public static extern int sr_bake_light_field(IntPtr scene, ref SrFrame frame, ulong first, ulong count, out ulong filled);
        [DllImport(Lib)] public static extern int sr_shadow_points(IntPtr scene, ref SrFrame frame, long n, [In] double[] pos, [In] double[] normal, [In] uint[] color, [Out] uint[] result, uint options);
        [DllImport(Lib)] public static extern int sr_static_shadow_points(IntPtr scene, ref SrFrame frame, long n, [In] double[] pos, [In] double[] normal, [In] uint[] color, [Out] uint[] result, [Out] byte[] amount, uint options, out ulong generators);
        [DllImport(Lib)] public static extern int sr_static_shadow_points_device(IntPtr scene, ref SrFrame frame, long n, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dOut, IntPtr dAmount, uint options, IntPtr hipStream, IntPtr dGenerators, IntPtr dStats);
        [DllImport(Lib)] public static extern int sr_get_shadow_cache(IntPtr scene, [Out] byte[] out128Cubed);
        [DllImport(Lib)] public static extern int sr_set_shadow_cache(IntPtr scene, [In] byte[] in128Cubed);
        [DllImport(Lib)] public static extern int sr_ao_points(IntPtr scene, ref SrFrame frame, long n, [In] double[] pos, [In] double[] normal, [In] uint[] color, [Out] uint[] result, [Out] byte[] amount, ulong firstGenerator, uint options, out ulong generators);
        [DllImport(Lib)] public static extern int sr_ao_points_device(IntPtr scene, ref SrFrame frame, long n, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dOut, IntPtr dAmount, ulong firstGenerator, uint options, IntPtr hipStream, IntPtr dGenerators, IntPtr dStats);
        [DllImport(Lib)] public static extern int sr_net_random_jump(int seed, ulong skip, [Out] int[] out55);
        [DllImport(Lib)] public static extern int sr_path_points(IntPtr scene, ref SrFrame frame, long n, [In] double[] pos, [In] double[] normal, [In] uint[] color, [Out] uint[] result, [Out] uint[] incoming, [Out] double[] dirs, ulong firstSample, uint options);
        [DllImport(Lib)] public static extern int sr_path_points_device(IntPtr scene, ref SrFrame frame, long n, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dOut, IntPtr dIncoming, IntPtr dDirs, ulong firstSample, uint options, IntPtr hipStream, IntPtr dStats);
        [DllImport(Lib)] public static extern int sr_shadow_points_device(IntPtr scene, ref SrFrame frame, long n, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dOut, uint options, IntPtr hipStream, IntPtr dStats);
        [DllImport(Lib)] public static extern int sr_shade_points_device(IntPtr scene, ref SrFrame frame, long n, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dOut, IntPtr hipStream);
        [DllImport(Lib)] public static extern long sr_frame_sample_count(ref SrFrame frame);
        [DllImport(Lib)] public static extern int sr_render_hits(IntPtr scene, ref SrFrame frame, [Out] double[] starts, [Out] double[] dirs, [Out] byte[] hit, [Out] double[] rayFrac, [Out] double[] pos, [Out] double[] normal, [Out] uint[] color, [Out] int[] triIndex, [Out] ulong[] stats4);
        [DllImport(Lib)] public static extern int sr_render_hits_device(IntPtr scene, ref SrFrame frame, IntPtr dStarts, IntPtr dDirs, IntPtr dHit, IntPtr dRayFrac, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dTriIndex, IntPtr hipStream, IntPtr dStats);
        [DllImport(Lib)] public static extern int sr_trace_origin_rays(IntPtr scene, int target, [In] double[] origin3, long n, [In] double[] dirs, [Out] byte[] hit, [Out] double[] rayFrac, [Out] double[] pos, [Out] double[] normal, [Out] uint[] color, [Out] int[] triIndex, uint options, [Out] ulong[] stats4);
        [DllImport(Lib)] public static extern int sr_trace_origin_rays_device(IntPtr scene, int target, [In] double[] origin3, long n, IntPtr dDirs, IntPtr dHit, IntPtr dRayFrac, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dTriIndex, uint options, IntPtr hipStream, IntPtr dStats);
        [DllImport(Lib)] public static extern int sr_occluded_rays(IntPtr scene, int target, long n, [In] double[] starts, [In] double[] dirs, [In] double[] limits, [Out] byte[] occluded, uint options, [Out] ulong[] stats4);
        [DllImport(Lib)] public static extern int sr_occluded_rays_device(IntPtr scene, int target, long n, IntPtr dStarts, IntPtr dDirs, IntPtr dLimits, IntPtr dOccluded, uint options, IntPtr hipStream, IntPtr dStats);
        [DllImport(Lib)] public static extern int sr_nearest_rays(IntPtr scene, int target, long n, [In] double[] starts, [In] double[] dirs, [In] double[] limits, [Out] byte[] hit, [Out] double[] rayFrac, [Out] double[] pos, [Out] double[] normal, [Out] uint[] color, [Out] int[] triIndex, uint options, [Out] ulong[] stats4);
        [DllImport(Lib)] public static extern int sr_nearest_rays_device(IntPtr scene, int target, long n, IntPtr dStarts, IntPtr dDirs, IntPtr dLimits, IntPtr dHit, IntPtr dRayFrac, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dTriIndex, uint options, IntPtr hipStream, IntPtr dStats);
        [DllImport(Lib)] public static extern int sr_all_hits_rays(IntPtr scene, int target, long n, [In] double[] starts, [In] double[] dirs, [In] double[] limits, int maxHits, [Out] uint[] count, [Out] int[] index, [Out] double[] rayFrac, uint options, [Out] ulong[] stats4);
        [DllImport(Lib)] public static extern int sr_all_hits_rays_device(IntPtr scene, int target, long n, IntPtr dStarts, IntPtr dDirs, IntPtr dLimits, int maxHits, IntPtr dCount, IntPtr dIndex, IntPtr dRayFrac, uint options, IntPtr hipStream, IntPtr dStats);
        [DllImport(Lib)] public static extern int sr_closest_points(IntPtr scene, int target, long n, [In] double[] points, [In] double[] maxDist, [Out] int[] triIndex, [Out] double[] dist, [Out] double[] pos, [Out] double[] uv, uint options, [Out] ulong[] stats4);
        [DllImport(Lib)] public static extern int sr_closest_points_device(IntPtr scene, int target, long n, IntPtr dPoints, IntPtr dMaxDist, IntPtr dTriIndex, IntPtr dDist, IntPtr dPos, IntPtr dUv, uint options, IntPtr hipStream, IntPtr dStats);
        [DllImport(Lib)] public static extern int sr_near_triangles(IntPtr scene, int target, long n, [In] double[] points, [In] double[] maxDist, int maxHits, [Out] uint[] count, [Out] int[] index, [Out] double[] dist, [Out] double[] pos, [Out] double[] uv, uint options, [Out] ulong[] stats4);
        [DllImport(Lib)] public static extern int sr_near_triangles_device(IntPtr scene, int target, long n, IntPtr dPoints, IntPtr dMaxDist, int maxHits, IntPtr dCount, IntPtr dIndex, IntPtr dDist, IntPtr dPos, IntPtr dUv, uint options, IntPtr hipStream, IntPtr dStats);
        [DllImport(Lib)] public static extern int sr_overlap_triangles(IntPtr scene, int target, long n, [In] double[] tris, int maxHits, [Out] uint[] count, [Out] int[] index, [Out] byte[] mask, uint options, [Out] ulong[] stats4);
        [DllImport(Lib)] public static extern int sr_overlap_triangles_device(IntPtr scene, int target, long n, IntPtr dTris, int maxHits, IntPtr dCount, IntPtr dIndex, IntPtr dMask, uint options, IntPtr hipStream, IntPtr dStats);
        [DllImport(Lib)] public static extern int sr_load_3ds(IntPtr scene, byte[] data, UIntPtr len);
        [DllImport(Lib)] public static extern int sr_post_process(IntPtr scene, [In, Out] int[] pixels, long count, int style, uint backgroundColor);
        [DllImport(Lib)] public static extern int sr_anti_alias(IntPtr scene, [In] int[] src, int dstWidth, int dstHeight, int resolution, [In, Out] int[] dst);
        [DllImport(Lib)] public static extern IntPtr sr_last_error();
        [DllImport(Lib)] public static extern int sr_abi_version();
        public static string LastError() { return Marshal.PtrToStringAnsi(sr_last_error()); }

        public const int SR_ERR_INVALID_ARG = -1, SR_ERR_OUT_OF_RANGE = -2, SR_ERR_NO_MODEL = -3, SR_ERR_FORMAT = -8;
        public const int AbiVersion = 5;

        /// <param name="renderCall">true only for sr_render: Render() without a model draws nothing and returns (Renderer.cs:736-739)</param>
        public static void Check(int rc, bool renderCall = false)
        {
            if (rc == 0 || (renderCall && rc == SR_ERR_NO_MODEL)) return;
            string msg = LastError();
            switch (rc)
            {
                case SR_ERR_OUT_OF_RANGE: throw new ArgumentOutOfRangeException("geometry", msg);   // SpatialSubdivision.cs:293
                case SR_ERR_FORMAT: throw new FormatException(msg);                                   // Model.cs:555, ThreeDSFile.cs:168
                case SR_ERR_INVALID_ARG: throw new ArgumentException(msg);
                default: throw new InvalidOperationException(msg);
            }
        }
    }

    /// <summary>What Renderer hands to the device(s) instead of the TPL fan-out over RaytraceBlock (Renderer.cs:1655-1686).</summary>
    public sealed class SoftrayHip : IDisposable
    {
        public const uint F_SHADING = 1, F_SHADOWS = 2, F_FOCAL_BLUR = 4, F_POINT_LIGHT = 8, F_SPECULAR = 16, F_STATIC_SHADOWS = 32;
        /// rayTracePathTracing (Renderer.cs:1613-1618): pass it in `flags` together with rayTraceRandomSeed and rayTraceConcurrency
        /// (the row blocks that each restart the random sequence).  Not together with F_SHADOWS: the library answers
        /// SR_ERR_UNSUPPORTED, which Check turns into InvalidOperationException.
        public const uint F_PATH_TRACING = 1u << 6;
        /// rayTraceVoxels (Renderer.cs:1568-1588) = SR_F_VOXELS: the library walks its own 64^3 grid of the uploaded triangles instead of the
        /// model's tree and the extra geometry; trace_mode is ignored and nothing needs building.  Not together with F_SHADOWS,
        /// F_PATH_TRACING or mirror bounces (SR_ERR_UNSUPPORTED -> InvalidOperationException): keep the CPU chain for those.
        public const uint F_VOXELS = 1u << 7;
        /// rayTraceAmbientOcclusion (Renderer.cs:1631-1638) = SR_F_AMBIENT_OCCLUSION: pass it in `flags` together with rayTraceRandomSeed and
        /// rayTraceConcurrency; F_AO_UNCACHED (with it) = AmbientOcclusionMethod.EnableCache = false.  Not together with F_PATH_TRACING,
        /// F_VOXELS, F_STATIC_SHADOWS or mirror bounces (SR_ERR_UNSUPPORTED -> InvalidOperationException).  The cache lives in the
        /// scene: ResetAmbientOcclusionCache() is what a new Renderer starts with, Get / SetAmbientOcclusionCache move the bytes of
        /// the reference's .ao file (AmbientOcclusion.cs:232-309; the file itself stays the host's business).
        public const uint F_AMBIENT_OCCLUSION = 1u << 13, F_AO_UNCACHED = 1u << 14;
        public const int AoCacheBytes = 128 * 128 * 128;
        /// rayTraceLightField with LightFieldStoresTriangles = false (Renderer.cs:1640-1649) = SR_F_LIGHT_FIELD: pass it in `flags`.  Not together
        /// with F_SHADOWS, F_AMBIENT_OCCLUSION, F_PATH_TRACING, F_VOXELS or mirror bounces (SR_ERR_UNSUPPORTED -> InvalidOperationException);
        /// LightFieldStoresTriangles = true (LightFieldTriMethod) is an opt-in: LightFieldTriangles = true, then the same flag runs it on the triangle table.  The table of 4 N^4 uint entries lives in the scene:
        /// LightFieldResolution is N (default 64 = lightFieldRes), ResetLightField() is what a new Renderer starts with (call it when
        /// LightFieldStoresTriangles changes, Renderer.cs:420-445), Get / SetLightField move ranges of the reference's .cache file.
        public const uint F_LIGHT_FIELD = 1u << 15;
        const uint F_PRIMARY_STATS_ONLY = 1u << 12;     // Num* count primary rays (Renderer.cs:1916-1923): no counting in the shadow stage
        public const int MODE_REF_TREE = 0, MODE_BRUTE = 1, MODE_BVH = 2;
        /// How NumGeometryTests / NumNodeVisits / NumLeafNodeVisits (Renderer.cs:476-504) are answered -- an explicit choice of the
        /// constructor, because they are the literal reference-tree traversal's counters and the fast path does not walk that tree.
        ///   Literal  every model's primary rays walk the reference tree (SR_MODE_REF_TREE): the reference's counters, any model size;
        ///   Auto     (default) models of fewer than OwnBvhThreshold triangles -- the sizes the reference itself handles -- as Literal,
        ///            larger ones as Off;
        ///   Off      every subdivided model on the library's own BVH; Render() then leaves CountersAvailable false and the patched
        ///            Renderer getters throw InvalidOperationException (never a silent zero).
        /// NumRaysFired is exact in every mode; shadow rays take the shaft path on the own BVH in all three (same pixels:
        /// include/softray.h SR_MODE_BVH; obj.3DS at 1024^2: 0.36 ms literal, 0.17 ms on the own BVH).
        public enum TraversalCounters { Auto, Literal, Off }
        public readonly TraversalCounters Counters;
        public int OwnBvhThreshold = 2000;
        /// Did the last Render() produce the three traversal counters?  (false: it ran on the own BVH)
        public bool CountersAvailable { get; private set; } = true;
        IntPtr scene;
        Model uploaded;                  // the model whose triangles the scene holds
        uint builtModes;                 // structures built for `uploaded` (bit 1 << mode)
        SrFrame frame;                   // reused from call to call: its arrays are allocated once
        bool frameReady;
        int offsetsSeed;                 // seed areaLightOffsets was generated with
        double[] areaLightOffsets;       // new Random(rayTraceRandomSeed): ShadowMethod.cs:63-73
        GCHandle offsetsPin;

        /// <summary>One MI355X.</summary>
        public SoftrayHip(int device = 0, TraversalCounters counters = TraversalCounters.Auto)
        {
            Counters = counters;
            if (Native.sr_abi_version() != Native.AbiVersion) throw new InvalidOperationException("libsoftray_hip: ABI version mismatch");
            Native.Check(Native.sr_create(device, out scene));
        }

        /// <summary>A whole node from this one process: the frame's rows are split into interleaved 16-row strips over
        /// `devices` inside the library and copied straight into the caller's pixels (sr_create_multi).</summary>
        /// gatherOverRccl: frames that STAY on the first device (sr_render_device: a host that post-processes or displays from HBM)
        /// are gathered with one grouped ncclSend / ncclRecv over xGMI (sr_set_gather, include/softray.h) instead of peer copies;
        /// Render() into a managed int[] copies every device's strips over its own PCIe link either way.
        public SoftrayHip(int[] devices, TraversalCounters counters = TraversalCounters.Auto, bool gatherOverRccl = false)
        {
            Counters = counters;
            if (Native.sr_abi_version() != Native.AbiVersion) throw new InvalidOperationException("libsoftray_hip: ABI version mismatch");
            Native.Check(Native.sr_create_multi(devices, devices.Length, out scene));
            if (gatherOverRccl) Native.Check(Native.sr_set_gather(scene, 1));
        }

        /// <summary>How many parts (devices) rendered rows of the last frame: 1 when the first device rendered it whole.</summary>
        public int LastFrameParts => Native.sr_last_frame_parts(scene);

        /// PreCalculate() (Renderer.cs:673-699): MakeRayTracableGeometry_simple (:1452-1469) flattened, then the structure for
        /// `mode`.  Like the reference (geometry_* == null guards, :684-696) nothing is rebuilt while the model and the mode
        /// stay the same -- Renderer.Render() calls PreCalculate() every frame.
        /// voxels: the frames will carry F_VOXELS (rayTraceVoxels): only the triangles are needed, no structure is built.
        public void Upload(Model model, int mode, bool voxels = false)
        {
            if (!ReferenceEquals(model, uploaded))
            {
                int n = model.Triangles.Count;
                var v9 = new double[n * 9]; var argb = new uint[n];
                int i = 0;
                foreach (Triangle tri in model.Triangles)                                            // triIndex = enumeration order, :1458-1467
                {
                    Vector v1 = model.Vertices[tri.vertexIndex1].pos, v2 = model.Vertices[tri.vertexIndex2].pos, v3 = model.Vertices[tri.vertexIndex3].pos;
                    v9[9 * i + 0] = v1.x; v9[9 * i + 1] = v1.y; v9[9 * i + 2] = v1.z;
                    v9[9 * i + 3] = v2.x; v9[9 * i + 4] = v2.y; v9[9 * i + 5] = v2.z;
                    v9[9 * i + 6] = v3.x; v9[9 * i + 7] = v3.y; v9[9 * i + 8] = v3.z;
                    argb[i] = Surface.PackColorAndAlpha(tri.diffuseMaterial, 1.0);                   // :1463
                    i++;
                }
                Native.Check(Native.sr_set_triangles(scene, v9, argb, n,
                    new[] { model.Min.x, model.Min.y, model.Min.z }, new[] { model.Max.x, model.Max.y, model.Max.z }));   // :1487
                uploaded = model;
                builtModes = 0;
            }
            if (voxels) return;                                                                      // SR_F_VOXELS ignores trace_mode
            uint bit = 1u << mode;
            if (mode == MODE_REF_TREE && UsesOwnBvh(model)) bit = 1u << MODE_BVH;                    // large model (or Off): only the own BVH is needed
            else if (mode == MODE_REF_TREE && model.Triangles.Count > 0) bit |= 1u << MODE_BVH;      // shadow rays of a tree frame take the shaft path
            if (mode != MODE_BRUTE && (builtModes & bit) != bit)
            {
                Native.Check(Native.sr_build(scene, bit & ~builtModes, 0, 0));                       // SpatialSubdivision defaults 15 / 25
                builtModes |= bit;
            }
        }

        /// The triangles from DEVICE memory (sr_set_triangles_device): v9 = double[n][3][3] and argb = uint[n] on the scene's device
        /// (of a multi-device scene: on its first device), copied and turned into records by kernels on `stream`; argb == IntPtr.Zero
        /// keeps every triangle's colour (same n as before).  A Model is host data in the reference, so this has no counterpart there:
        /// the scene no longer mirrors a Model afterwards (the next Upload sends its model again), and the structure of `mode` is
        /// built by BuildStructure, not by Upload.
        public void SetTrianglesDevice(IntPtr v9, IntPtr argb, long n, double[] min, double[] max, IntPtr stream)
        {
            Native.Check(Native.sr_set_triangles_device(scene, v9, argb, n, min, max, stream));
            uploaded = null;
            builtModes = 0;
        }

        /// New vertices for a mesh that only moves (sr_refit_triangles_device): arguments as SetTrianglesDevice, same n as the model.  The
        /// own BVH that BuildStructure(MODE_BVH) built on the device is REFIT -- no new build; every other structure is dropped as by
        /// SetTrianglesDevice.  The tree keeps the shape of its build: after a large deformation frames get slower, never wrong, and the
        /// caller decides when to BuildStructure again.
        public void RefitTrianglesDevice(IntPtr v9, IntPtr argb, long n, double[] min, double[] max, IntPtr stream)
        {
            Native.Check(Native.sr_refit_triangles_device(scene, v9, argb, n, min, max, stream));
            uploaded = null;
            builtModes &= 1u << 2;                                                                   // SR_MODE_BVH stays built
        }

        /// sr_build for the triangles that SetTrianglesDevice left (MODE_BVH above 64 triangles is built where they are: on the device)
        public void BuildStructure(int mode)
        {
            uint bit = 1u << mode;
            if (mode == MODE_BRUTE || (builtModes & bit) == bit) return;
            Native.Check(Native.sr_build(scene, bit, 0, 0));
            builtModes |= bit;
        }

        bool UsesOwnBvh(Model model)
        {
            if (model.Triangles.Count == 0 || Counters == TraversalCounters.Literal) return false;   // (an empty model: nothing to build a BVH from)
            return Counters == TraversalCounters.Off || model.Triangles.Count >= OwnBvhThreshold;
        }

        /// The trace mode Render() should be given for `rayTraceSubdivision`: the reference tree (literal) or, for large models,
        /// the library's own BVH.
        public int TraceMode(bool rayTraceSubdivision)
        {
            if (!rayTraceSubdivision) return MODE_BRUTE;
            return (uploaded != null && UsesOwnBvh(uploaded)) ? MODE_BVH : MODE_REF_TREE;
        }

        /// ExtraGeometryToRaytrace (Renderer.cs:460, 1545-1549): the collection is scanned first to last BEFORE the model, with
        /// a strict '<' on rayFrac (GeometryCollection.cs:44-69) -- the order is kept.  Call it whenever the collection changes
        /// and before the reference appends the model's root to it (:1547).  Uses the accessors INTEGRATION.md adds.
        public void SetExtraGeometry(GeometryCollection extras)
        {
            int n = extras == null ? 0 : extras.Count;
            var prims = new SrPrim[Math.Max(n, 1)];
            for (int i = 0; i < n; i++)
            {
                var prim = new SrPrim { p = new double[9] };
                IRayIntersectable g = extras[i];
                var sphere = g as Sphere; var plane = g as Plane; var tri = g as Raytrace.Triangle; var box = g as AxisAlignedBox;
                if (sphere != null)
                {
                    prim.kind = 0; prim.argb = sphere.PackedColor;                                    // Color.ToARGB(), Sphere.cs:51-55
                    prim.p[0] = sphere.Center.x; prim.p[1] = sphere.Center.y; prim.p[2] = sphere.Center.z; prim.p[3] = sphere.Radius;
                }
                else if (plane != null)
                {
                    prim.kind = 3; prim.argb = plane.PackedColor;                                     // the stored unit normal and originDist, verbatim
                    prim.p[0] = plane.Normal.x; prim.p[1] = plane.Normal.y; prim.p[2] = plane.Normal.z; prim.p[3] = plane.DistanceToOrigin;
                }
                else if (tri != null)
                {
                    prim.kind = 2; prim.argb = tri.Color;
                    prim.p[0] = tri.Vertex1.x; prim.p[1] = tri.Vertex1.y; prim.p[2] = tri.Vertex1.z;
                    prim.p[3] = tri.Vertex2.x; prim.p[4] = tri.Vertex2.y; prim.p[5] = tri.Vertex2.z;
                    prim.p[6] = tri.Vertex3.x; prim.p[7] = tri.Vertex3.y; prim.p[8] = tri.Vertex3.z;
                }
                else if (box != null)
                {
                    prim.kind = 4; prim.argb = 0xffffffffu;                                           // six Color.White planes (AxisAlignedBox.cs:22-27, Plane.cs:28)
                    prim.p[0] = box.Min.x; prim.p[1] = box.Min.y; prim.p[2] = box.Min.z; prim.p[3] = box.Max.x; prim.p[4] = box.Max.y; prim.p[5] = box.Max.z;
                }
                else throw new NotSupportedException("ExtraGeometryToRaytrace holds a " + g.GetType().Name + ": only Sphere, Plane, Triangle and AxisAlignedBox have a device form");
                prims[i] = prim;
            }
            if (n == 0) prims[0].p = new double[9];
            Native.Check(Native.sr_set_extra_geometry(scene, prims, n));
        }

        /// The frame of a call (Renderer.cs:1510-1528): the arguments copied into the reused sr_frame, the area-light offsets of the seed
        void FillFrame(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform,
                       uint backgroundColor, uint flags, int mode, int startRow, int endRow, int subPixelRes, int randomSeed,
                       double fieldOfViewDepth, double focalDepth, double focalBlurStrength, double ambient, double shininess,
                       Vector lightDirView, Vector lightPosView, int concurrency)
        {
            if (areaLightOffsets == null || offsetsSeed != randomSeed)
            {
                var random = new Random(randomSeed);                                                   // Renderer.cs:1624
                var table = new double[300];
                for (int i = 0; i < 100; i++)                                                          // softShadowQuality, ShadowMethod.cs:9
                {
                    var o = new Vector(random.NextDouble() * 2 - 1, random.NextDouble() * 2 - 1, random.NextDouble() * 2 - 1);
                    o.Normalise(); o *= 0.2;
                    table[3 * i] = o.x; table[3 * i + 1] = o.y; table[3 * i + 2] = o.z;
                }
                if (offsetsPin.IsAllocated) offsetsPin.Free();
                areaLightOffsets = table;
                offsetsPin = GCHandle.Alloc(areaLightOffsets, GCHandleType.Pinned);
                offsetsSeed = randomSeed;
            }
            if (!frameReady)
            {
                frame = new SrFrame { transform = new double[12], inv_transform = new double[12], light_dir_view = new double[3], light_pos_view = new double[3] };
                frameReady = true;
            }
            frame.width = width; frame.height = height; frame.start_row = startRow; frame.end_row = endRow; frame.sub_pixel_res = subPixelRes;
            frame.background_argb = backgroundColor; frame.flags = flags | F_PRIMARY_STATS_ONLY; frame.random_seed = randomSeed; frame.shadow_samples = 0; frame.trace_mode = mode;
            frame.concurrency = concurrency;                                 // rayTraceConcurrency: fill order of the static shadow cache, row blocks of the path tracer
            frame.position_z = instance.Position.z; frame.fov_depth = fieldOfViewDepth; frame.focal_depth = focalDepth;
            frame.focal_blur_strength = focalBlurStrength; frame.ambient = ambient; frame.shininess = shininess;
            frame.light_dir_view[0] = lightDirView.x; frame.light_dir_view[1] = lightDirView.y; frame.light_dir_view[2] = lightDirView.z;
            frame.light_pos_view[0] = lightPosView.x; frame.light_pos_view[1] = lightPosView.y; frame.light_pos_view[2] = lightPosView.z;
            frame.area_light_offsets = offsetsPin.AddrOfPinnedObject();
            for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) { frame.transform[4 * r + c] = transform[r, c]; frame.inv_transform[4 * r + c] = inverseTransform[r, c]; }
        }

        /// Pre-compute the colour light field (sr_bake_light_field): every entry of first .. first + count - 1 that is still empty gets the colour
        /// of its cell's canonical ray, traced and shaded with the frame these arguments describe (the same as Render's; `flags` must hold
        /// F_LIGHT_FIELD; the surface size, rows and sub-pixel samples are validated and otherwise unused).  Frames rendered afterwards look
        /// their colours up and trace nothing.  Blocks; returns the number of entries written.  count = ulong.MaxValue: to the end of the table.
        public ulong BakeLightField(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform,
                                    uint backgroundColor, uint flags, int mode, int subPixelRes, int randomSeed,
                                    double fieldOfViewDepth, double focalDepth, double focalBlurStrength, double ambient, double shininess,
                                    Vector lightDirView, Vector lightPosView, ulong first = 0, ulong count = ulong.MaxValue)
        {
            FillFrame(width, height, instance, transform, inverseTransform, backgroundColor, flags, mode, 0, height - 1, subPixelRes, randomSeed,
                      fieldOfViewDepth, focalDepth, focalBlurStrength, ambient, shininess, lightDirView, lightPosView, 4);
            if (count == ulong.MaxValue)
            {
                ulong n = (ulong)LightFieldResolution, total = 4 * n * n * n * n;
                count = first <= total ? total - first : 1;          // (beyond the table: the library says so)
            }
            ulong filled;
            Native.Check(Native.sr_bake_light_field(scene, ref frame, first, count, out filled));
            return filled;
        }

        /// The colour light field for caller-given lines (sr_light_field_rays; LightFieldColorMethod.IntersectRay): result[i] = the colour a
        /// F_LIGHT_FIELD frame gives a camera sample whose ray is (starts[i], dirs[i]) -- double[n * 3] in model space, the direction not
        /// normalised -- for the frame these arguments describe (the same as Render's; F_LIGHT_FIELD is implied, the surface size is validated and
        /// otherwise unused).  Empty entries of the scene's table are filled first, as a frame fills them: `filled` receives their number.
        /// inside (byte[n] or null): 1 where the line pierces the sphere; a line that misses it gets the background.  The triangle light field
        /// and what a light-field frame refuses: SR_ERR_UNSUPPORTED -> InvalidOperationException.  Blocks.
        public uint[] LightFieldRays(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform, uint backgroundColor, uint flags,
                                     int mode, int randomSeed, double fieldOfViewDepth, double ambient, double shininess, Vector lightDirView,
                                     Vector lightPosView, double[] starts, double[] dirs, out ulong filled, byte[] inside = null)
        {
            if (starts == null || dirs == null || starts.Length != dirs.Length || starts.Length % 3 != 0 || (inside != null && inside.Length != starts.Length / 3))
                throw new ArgumentException("LightFieldRays: starts and dirs are double[n * 3], inside is byte[n] or null");
            FillFrame(width, height, instance, transform, inverseTransform, backgroundColor, flags, mode, 0, height - 1, 1, randomSeed,
                      fieldOfViewDepth, 1.0, 0.0, ambient, shininess, lightDirView, lightPosView, 4);
            var result = new uint[starts.Length / 3];
            Native.Check(Native.sr_light_field_rays(scene, ref frame, result.Length, starts, dirs, result, inside, 0, out filled));
            return result;
        }

        /// The same with every array in DEVICE memory on the scene's device (sr_light_field_rays_device): enqueued on `stream` without a host
        /// synchronisation; dInside and dFilled (a ulong on the device) may be IntPtr.Zero; dStats: ulong[24] on the device, or IntPtr.Zero.
        public void LightFieldRaysDevice(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform, uint backgroundColor, uint flags,
                                         int mode, int randomSeed, double fieldOfViewDepth, double ambient, double shininess, Vector lightDirView,
                                         Vector lightPosView, long n, IntPtr dStarts, IntPtr dDirs, IntPtr dOut, IntPtr dInside, IntPtr stream,
                                         IntPtr dFilled, IntPtr dStats)
        {
            FillFrame(width, height, instance, transform, inverseTransform, backgroundColor, flags, mode, 0, height - 1, 1, randomSeed,
                      fieldOfViewDepth, 1.0, 0.0, ambient, shininess, lightDirView, lightPosView, 4);
            Native.Check(Native.sr_light_field_rays_device(scene, ref frame, n, dStarts, dDirs, dOut, dInside, 0, stream, dFilled, dStats));
        }

        /// sr_shadow_points' option bit 0: 64 consecutive points are neighbours, a pass is queued in the order given (no ray sort)
        public const uint POINTS_COHERENT = 1;

        /// ShadowMethod's soft shadow for caller-given surface points (sr_shadow_points; ShadowMethod.cs:103-119, 144-179): result[i] = color[i]
        /// (color == null: 0xFFFFFFFF) modulated with (byte)(escapes / 100.0 * 255) for the light, the seed's area-light offsets and the root
        /// geometry of the frame these arguments describe (the same as Render's; F_SHADOWS is implied, the surface size is validated and
        /// otherwise unused).  pos / normal: double[n * 3] in model space, the normal as given.  F_STATIC_SHADOWS, F_AMBIENT_OCCLUSION,
        /// F_PATH_TRACING, F_VOXELS and F_LIGHT_FIELD name no step of ShadowMethod on a bare point: SR_ERR_UNSUPPORTED ->
        /// InvalidOperationException.  Blocks.
        public uint[] ShadowPoints(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform, uint flags, int mode, int randomSeed,
                                   Vector lightDirView, Vector lightPosView, double[] pos, double[] normal, uint[] color = null, bool coherent = false)
        {
            if (pos == null || normal == null || pos.Length != normal.Length || pos.Length % 3 != 0 || (color != null && color.Length != pos.Length / 3))
                throw new ArgumentException("ShadowPoints: pos and normal are double[n * 3], color is uint[n] or null");
            FillFrame(width, height, instance, transform, inverseTransform, 0, flags, mode, 0, height - 1, 1, randomSeed,
                      1.0, 1.0, 0.0, 0.0, 0.0, lightDirView, lightPosView, 4);
            frame.flags &= ~F_PRIMARY_STATS_ONLY;                  // the call has no primary rays
            var result = new uint[pos.Length / 3];
            Native.Check(Native.sr_shadow_points(scene, ref frame, result.Length, pos, normal, color, result, coherent ? POINTS_COHERENT : 0));
            return result;
        }

        /// The same with every array in DEVICE memory on the scene's device (sr_shadow_points_device): enqueued on `stream` without a host
        /// synchronisation; dColor may be IntPtr.Zero (every point 0xFFFFFFFF) or dOut itself; dStats: ulong[24] on the device, or IntPtr.Zero.
        public void ShadowPointsDevice(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform, uint flags, int mode, int randomSeed,
                                       Vector lightDirView, Vector lightPosView, long n, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dOut,
                                       bool coherent, IntPtr stream, IntPtr dStats)
        {
            FillFrame(width, height, instance, transform, inverseTransform, 0, flags, mode, 0, height - 1, 1, randomSeed,
                      1.0, 1.0, 0.0, 0.0, 0.0, lightDirView, lightPosView, 4);
            frame.flags &= ~F_PRIMARY_STATS_ONLY;
            Native.Check(Native.sr_shadow_points_device(scene, ref frame, n, dPos, dNormal, dColor, dOut, coherent ? POINTS_COHERENT : 0, stream, dStats));
        }

        /// ShadowMethod's static branch for caller-given surface points, in input order (sr_static_shadow_points; ShadowMethod.cs:106-112,
        /// Texture3DCache.Sample): the first point of an empty cell of the scene's static shadow cache -- the one F_STATIC_SHADOWS frames fill --
        /// generates (byte)(escapes / 100.0 * 254 + 1) for the light, the seed's area-light offsets and the root geometry of the frame these
        /// arguments describe; amount[i] = the byte of point i's cell, result[i] = color[i] (color == null: 0xFFFFFFFF) modulated with it;
        /// `generators` receives the number of generators.  F_SHADOWS | F_STATIC_SHADOWS are implied.  pos / normal: double[n * 3] in model
        /// space, the normal as given.  F_AMBIENT_OCCLUSION, F_PATH_TRACING, F_VOXELS and F_LIGHT_FIELD: SR_ERR_UNSUPPORTED ->
        /// InvalidOperationException.  Blocks.
        public uint[] StaticShadowPoints(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform, uint flags, int mode, int randomSeed,
                                         Vector lightDirView, Vector lightPosView, double[] pos, double[] normal, uint[] color, out byte[] amount,
                                         out ulong generators, bool coherent = false)
        {
            if (pos == null || normal == null || pos.Length != normal.Length || pos.Length % 3 != 0 || (color != null && color.Length != pos.Length / 3))
                throw new ArgumentException("StaticShadowPoints: pos and normal are double[n * 3], color is uint[n] or null");
            FillFrame(width, height, instance, transform, inverseTransform, 0, flags, mode, 0, height - 1, 1, randomSeed,
                      1.0, 1.0, 0.0, 0.0, 0.0, lightDirView, lightPosView, 4);
            frame.flags &= ~F_PRIMARY_STATS_ONLY;                  // the call has no primary rays
            var result = new uint[pos.Length / 3];
            amount = new byte[pos.Length / 3];
            Native.Check(Native.sr_static_shadow_points(scene, ref frame, result.Length, pos, normal, color, result, amount, coherent ? POINTS_COHERENT : 0, out generators));
            return result;
        }

        /// The same with every array in DEVICE memory on the scene's device (sr_static_shadow_points_device): enqueued on `stream` without a host
        /// synchronisation; dColor may be IntPtr.Zero (every point 0xFFFFFFFF) or dOut itself; one of dOut / dAmount may be IntPtr.Zero;
        /// dGenerators: a ulong on the device, or IntPtr.Zero; dStats: ulong[24] on the device, or IntPtr.Zero.
        public void StaticShadowPointsDevice(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform, uint flags, int mode, int randomSeed,
                                             Vector lightDirView, Vector lightPosView, long n, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dOut,
                                             IntPtr dAmount, bool coherent, IntPtr stream, IntPtr dGenerators, IntPtr dStats)
        {
            FillFrame(width, height, instance, transform, inverseTransform, 0, flags, mode, 0, height - 1, 1, randomSeed,
                      1.0, 1.0, 0.0, 0.0, 0.0, lightDirView, lightPosView, 4);
            frame.flags &= ~F_PRIMARY_STATS_ONLY;
            Native.Check(Native.sr_static_shadow_points_device(scene, ref frame, n, dPos, dNormal, dColor, dOut, dAmount, coherent ? POINTS_COHERENT : 0, stream, dGenerators, dStats));
        }

        /// AmbientOcclusionMethod's occlusion byte for caller-given surface points, in input order (sr_ao_points; AmbientOcclusionMethod.cs:65-99,
        /// AmbientOcclusion.cs:101-230): amount[i] = the byte of point i's cell (F_AO_UNCACHED in flags: of the point itself, every point
        /// generates), result[i] = color[i] (color == null: 0xFFFFFFFF) modulated with it.  Generator g of the call uses draws
        /// 300 (firstGenerator + g) .. + 299 of Random(randomSeed); `generators` receives their number, which a caller that splits a batch adds
        /// to firstGenerator of the next call.  F_AMBIENT_OCCLUSION is implied; the cache is the scene's, the one AO frames fill.  pos / normal:
        /// double[n * 3] in model space, the normal as given.  F_STATIC_SHADOWS, F_PATH_TRACING, F_VOXELS and F_LIGHT_FIELD:
        /// SR_ERR_UNSUPPORTED -> InvalidOperationException.  Blocks.
        public uint[] AoPoints(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform, uint flags, int mode, int randomSeed,
                               double[] pos, double[] normal, uint[] color, out byte[] amount, out ulong generators, ulong firstGenerator = 0)
        {
            if (pos == null || normal == null || pos.Length != normal.Length || pos.Length % 3 != 0 || (color != null && color.Length != pos.Length / 3))
                throw new ArgumentException("AoPoints: pos and normal are double[n * 3], color is uint[n] or null");
            FillFrame(width, height, instance, transform, inverseTransform, 0, flags, mode, 0, height - 1, 1, randomSeed,
                      1.0, 1.0, 0.0, 0.0, 0.0, new Vector(0, 0, 1), new Vector(0, 0, 0), 4);
            frame.flags &= ~F_PRIMARY_STATS_ONLY;                  // the call has no primary rays
            var result = new uint[pos.Length / 3];
            amount = new byte[pos.Length / 3];
            Native.Check(Native.sr_ao_points(scene, ref frame, result.Length, pos, normal, color, result, amount, firstGenerator, 0, out generators));
            return result;
        }

        /// The same with every array in DEVICE memory on the scene's device (sr_ao_points_device): enqueued on `stream` without a host
        /// synchronisation; dColor may be IntPtr.Zero (every point 0xFFFFFFFF) or dOut itself; one of dOut / dAmount may be IntPtr.Zero;
        /// dGenerators: a ulong on the device, or IntPtr.Zero; dStats: ulong[24] on the device, or IntPtr.Zero.
        public void AoPointsDevice(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform, uint flags, int mode, int randomSeed,
                                   long n, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dOut, IntPtr dAmount, ulong firstGenerator,
                                   IntPtr stream, IntPtr dGenerators, IntPtr dStats)
        {
            FillFrame(width, height, instance, transform, inverseTransform, 0, flags, mode, 0, height - 1, 1, randomSeed,
                      1.0, 1.0, 0.0, 0.0, 0.0, new Vector(0, 0, 1), new Vector(0, 0, 0), 4);
            frame.flags &= ~F_PRIMARY_STATS_ONLY;
            Native.Check(Native.sr_ao_points_device(scene, ref frame, n, dPos, dNormal, dColor, dOut, dAmount, firstGenerator, 0, stream, dGenerators, dStats));
        }

        /// PathTracingMethod's one-bounce diffuse term for caller-given surface points, in input order (sr_path_points; PathTracingMethod.cs:51-76):
        /// point i fires one second ray from pos[i] + normal[i] * 0.001 in the direction made of draws 3 (firstSample + i) .. + 2 of
        /// Random(randomSeed); incoming[i] = that hit's colour (0 on a miss; with F_SHADING shaded as a frame shades it, with fieldOfViewDepth,
        /// ambient, shininess and the lights given here -- the values Render() and ShadePointsDevice take), result[i] = incoming * (normal . d) +
        /// color[i] (color == null: 0xFFFFFFFF), dirs = the directions (double[n * 3]).  A caller that splits a batch passes firstSample + n to
        /// the next call; averaging several rounds is the caller's loop over firstSample.  F_PATH_TRACING is implied.  pos / normal:
        /// double[n * 3] in model space, the normal as given.  F_SHADOWS, F_AMBIENT_OCCLUSION, F_VOXELS and F_LIGHT_FIELD: SR_ERR_UNSUPPORTED ->
        /// InvalidOperationException.  Blocks.
        public uint[] PathPoints(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform, uint flags, int mode, int randomSeed,
                                 double fieldOfViewDepth, double ambient, double shininess, Vector lightDirView, Vector lightPosView,
                                 double[] pos, double[] normal, uint[] color, out uint[] incoming, out double[] dirs, ulong firstSample = 0)
        {
            if (pos == null || normal == null || pos.Length != normal.Length || pos.Length % 3 != 0 || (color != null && color.Length != pos.Length / 3))
                throw new ArgumentException("PathPoints: pos and normal are double[n * 3], color is uint[n] or null");
            FillFrame(width, height, instance, transform, inverseTransform, 0, flags, mode, 0, height - 1, 1, randomSeed,
                      fieldOfViewDepth, 1.0, 0.0, ambient, shininess, lightDirView, lightPosView, 4);
            frame.flags &= ~F_PRIMARY_STATS_ONLY;                  // the call has no primary rays
            var result = new uint[pos.Length / 3];
            incoming = new uint[pos.Length / 3];
            dirs = new double[pos.Length];
            Native.Check(Native.sr_path_points(scene, ref frame, result.Length, pos, normal, color, result, incoming, dirs, firstSample, 0));
            return result;
        }

        /// The same with every array in DEVICE memory on the scene's device (sr_path_points_device): enqueued on `stream` without a host
        /// synchronisation; dColor may be IntPtr.Zero (every point 0xFFFFFFFF) or dOut itself; dOut, dIncoming and dDirs may each be
        /// IntPtr.Zero, not all three; dStats: ulong[24] on the device, or IntPtr.Zero.
        public void PathPointsDevice(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform, uint flags, int mode, int randomSeed,
                                     double fieldOfViewDepth, double ambient, double shininess, Vector lightDirView, Vector lightPosView,
                                     long n, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dOut, IntPtr dIncoming, IntPtr dDirs, ulong firstSample,
                                     IntPtr stream, IntPtr dStats)
        {
            FillFrame(width, height, instance, transform, inverseTransform, 0, flags, mode, 0, height - 1, 1, randomSeed,
                      fieldOfViewDepth, 1.0, 0.0, ambient, shininess, lightDirView, lightPosView, 4);
            frame.flags &= ~F_PRIMARY_STATS_ONLY;
            Native.Check(Native.sr_path_points_device(scene, ref frame, n, dPos, dNormal, dColor, dOut, dIncoming, dDirs, firstSample, 0, stream, dStats));
        }

        /// The frame G-buffer (sr_render_hits): the arrays a caller wants of one frame's primary hits
        public sealed class FrameHits
        {
            public double[] Starts, Dirs;          // [S * 3] camera rays in model space (null unless asked for)
            public byte[] Hit;                     // [S] 1 hit, 0 miss (zeros and triangle -1)
            public double[] RayFrac, Pos, Normal;  // [S], [S * 3], [S * 3]
            public uint[] Color;                   // [S] unshaded surface colour
            public int[] TriIndex;                 // [S] TriangleIndex, -1 for extra geometry and misses
            public ulong[] Stats4;                 // primary {rays, tests, nodes, leaves}
        }

        /// What the primary stage of the frame these arguments describe answers per camera sample, before any decorator (sr_render_hits), in
        /// scan order ((row - first row) * width + col) * n^2 + subX * n + subY.  The decorator flags are not read; F_VOXELS, F_LIGHT_FIELD and
        /// F_SINGLE_KERNEL are refused: SR_ERR_UNSUPPORTED -> InvalidOperationException.  Blocks.
        public FrameHits RenderHits(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform, uint flags, int mode,
                                    int startRow, int endRow, int subPixelRes, double fieldOfViewDepth, double focalDepth, double focalBlurStrength,
                                    bool rays = false)
        {
            FillFrame(width, height, instance, transform, inverseTransform, 0, flags, mode, startRow, endRow, subPixelRes, 0,
                      fieldOfViewDepth, focalDepth, focalBlurStrength, 0.0, 0.0, new Vector(0, 0, 1), new Vector(0, 0, 0), 4);
            long s = Native.sr_frame_sample_count(ref frame);
            var r = new FrameHits { Hit = new byte[s], RayFrac = new double[s], Pos = new double[s * 3], Normal = new double[s * 3],
                                    Color = new uint[s], TriIndex = new int[s], Stats4 = new ulong[4] };
            if (rays) { r.Starts = new double[s * 3]; r.Dirs = new double[s * 3]; }
            Native.Check(Native.sr_render_hits(scene, ref frame, r.Starts, r.Dirs, r.Hit, r.RayFrac, r.Pos, r.Normal, r.Color, r.TriIndex, r.Stats4));
            return r;
        }

        /// The same with every array in DEVICE memory on the scene's device (sr_render_hits_device), IntPtr.Zero for an array that is not wanted;
        /// enqueued on `stream` without a host synchronisation; dStats: ulong[24] on the device, or IntPtr.Zero.
        public void RenderHitsDevice(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform, uint flags, int mode,
                                     int startRow, int endRow, int subPixelRes, double fieldOfViewDepth, double focalDepth, double focalBlurStrength,
                                     IntPtr dStarts, IntPtr dDirs, IntPtr dHit, IntPtr dRayFrac, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dTriIndex,
                                     IntPtr stream, IntPtr dStats)
        {
            FillFrame(width, height, instance, transform, inverseTransform, 0, flags, mode, startRow, endRow, subPixelRes, 0,
                      fieldOfViewDepth, focalDepth, focalBlurStrength, 0.0, 0.0, new Vector(0, 0, 1), new Vector(0, 0, 0), 4);
            Native.Check(Native.sr_render_hits_device(scene, ref frame, dStarts, dDirs, dHit, dRayFrac, dPos, dNormal, dColor, dTriIndex, stream, dStats));
        }

        /// Nearest hits of a batch of rays that start in one point (sr_trace_origin_rays): bit for bit what IntersectRay answers for
        /// (origin, dirs[i]) on the root geometry (root = true) or the model alone, on the packet walk of a frame's camera rays.  dirs is
        /// double[n * 3], not normalised; coherent: every 64 consecutive rays are neighbours (an image in 8x8-tile-major order).  The call
        /// re-keys the scene's per-origin records to `origin`, as a camera move does.  Blocks.
        public const uint RAYS_COHERENT = 1;
        public FrameHits TraceOriginRays(Vector origin, double[] dirs, int mode, bool root = false, bool coherent = false)
        {
            long n = dirs.Length / 3;
            var r = new FrameHits { Hit = new byte[n], RayFrac = new double[n], Pos = new double[n * 3], Normal = new double[n * 3],
                                    Color = new uint[n], TriIndex = new int[n], Stats4 = new ulong[4] };
            Native.Check(Native.sr_trace_origin_rays(scene, mode | (root ? 0x100 : 0), new[] { origin.x, origin.y, origin.z }, n, dirs, r.Hit, r.RayFrac, r.Pos,
                                                     r.Normal, r.Color, r.TriIndex, coherent ? RAYS_COHERENT : 0, r.Stats4));
            return r;
        }

        /// The same with every array in DEVICE memory on the scene's device (sr_trace_origin_rays_device), IntPtr.Zero for an output that is not
        /// wanted; `origin` stays a host value; enqueued on `stream` without a host synchronisation; dStats: ulong[24] on the device, or IntPtr.Zero.
        public void TraceOriginRaysDevice(Vector origin, long n, IntPtr dDirs, int mode, bool root, bool coherent, IntPtr dHit, IntPtr dRayFrac, IntPtr dPos,
                                          IntPtr dNormal, IntPtr dColor, IntPtr dTriIndex, IntPtr stream, IntPtr dStats)
        {
            Native.Check(Native.sr_trace_origin_rays_device(scene, mode | (root ? 0x100 : 0), new[] { origin.x, origin.y, origin.z }, n, dDirs, dHit, dRayFrac, dPos,
                                                            dNormal, dColor, dTriIndex, coherent ? RAYS_COHERENT : 0, stream, dStats));
        }

        /// "Is anything in the way before distance L" for a batch of rays (sr_occluded_rays): result[i] = 1 iff IntersectRay(starts[i], D_i) hits
        /// with rayFrac &lt;= limits[i] (limits == null: 1.0 for every ray) on the root geometry (root = true) or the model alone -- the test of
        /// ShadowMethod.cs:169-172, with early exit on the own BVH.  starts and dirs are double[n * 3]; D_i = dirs[i], or with endpoints
        /// dirs[i] - starts[i] (dirs holds end points).  coherent: the rays are walked in the order given.  Blocks.
        public const uint RAYS_ENDPOINTS = 2;
        public byte[] OccludedRays(double[] starts, double[] dirs, double[] limits, int mode, bool root = false, bool endpoints = false, bool coherent = false)
        {
            long n = starts.Length / 3;
            var occluded = new byte[n];
            Native.Check(Native.sr_occluded_rays(scene, mode | (root ? 0x100 : 0), n, starts, dirs, limits, occluded,
                                                 (endpoints ? RAYS_ENDPOINTS : 0) | (coherent ? RAYS_COHERENT : 0), null));
            return occluded;
        }

        /// The same with every array in DEVICE memory on the scene's device (sr_occluded_rays_device), dLimits IntPtr.Zero for 1.0 throughout;
        /// enqueued on `stream` without a host synchronisation; dStats: ulong[24] on the device, or IntPtr.Zero.
        public void OccludedRaysDevice(long n, IntPtr dStarts, IntPtr dDirs, IntPtr dLimits, IntPtr dOccluded, int mode, bool root, bool endpoints, bool coherent,
                                       IntPtr stream, IntPtr dStats)
        {
            Native.Check(Native.sr_occluded_rays_device(scene, mode | (root ? 0x100 : 0), n, dStarts, dDirs, dLimits, dOccluded,
                                                        (endpoints ? RAYS_ENDPOINTS : 0) | (coherent ? RAYS_COHERENT : 0), stream, dStats));
        }

        /// The nearest hit of a batch of arbitrary rays within a distance (sr_nearest_rays): bit for bit what IntersectRay answers for
        /// (starts[i], D_i) on the root geometry (root = true) or the model alone where that is a hit with rayFrac &lt;= limits[i] (limits == null:
        /// no limit), a miss otherwise -- on the walk a mirror level's rays take.  starts and dirs are double[n * 3]; D_i = dirs[i], or with
        /// endpoints dirs[i] - starts[i].  coherent: the rays are walked in the order given.  Blocks.
        public FrameHits NearestRays(double[] starts, double[] dirs, double[] limits, int mode, bool root = false, bool endpoints = false, bool coherent = false)
        {
            long n = starts.Length / 3;
            var r = new FrameHits { Hit = new byte[n], RayFrac = new double[n], Pos = new double[n * 3], Normal = new double[n * 3],
                                    Color = new uint[n], TriIndex = new int[n], Stats4 = new ulong[4] };
            Native.Check(Native.sr_nearest_rays(scene, mode | (root ? 0x100 : 0), n, starts, dirs, limits, r.Hit, r.RayFrac, r.Pos, r.Normal, r.Color, r.TriIndex,
                                                (endpoints ? RAYS_ENDPOINTS : 0) | (coherent ? RAYS_COHERENT : 0), r.Stats4));
            return r;
        }

        /// The same with every array in DEVICE memory on the scene's device (sr_nearest_rays_device), dLimits IntPtr.Zero for no limit and
        /// IntPtr.Zero for an output that is not wanted; enqueued on `stream` without a host synchronisation; dStats: ulong[24] on the device, or
        /// IntPtr.Zero.
        public void NearestRaysDevice(long n, IntPtr dStarts, IntPtr dDirs, IntPtr dLimits, int mode, bool root, bool endpoints, bool coherent, IntPtr dHit,
                                      IntPtr dRayFrac, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dTriIndex, IntPtr stream, IntPtr dStats)
        {
            Native.Check(Native.sr_nearest_rays_device(scene, mode | (root ? 0x100 : 0), n, dStarts, dDirs, dLimits, dHit, dRayFrac, dPos, dNormal, dColor,
                                                       dTriIndex, (endpoints ? RAYS_ENDPOINTS : 0) | (coherent ? RAYS_COHERENT : 0), stream, dStats));
        }

        /// Every hit along each ray of a batch, nearest first, with a count (sr_all_hits_rays).  Count[i]: the hits with rayFrac &lt;= limits[i]
        /// (limits == null: no limit), not capped by maxHits; rows i of Index / RayFrac ([n * maxHits]) hold the first min(count, maxHits) of them
        /// by (rayFrac, extra elements first, index) -- TriangleIndex, or -2 - e for extra element e -- and -1 / 0.0 in the unused slots.
        /// mode is MODE_BVH or MODE_BRUTE (the literal reference tree has no notion of all hits).  Blocks.
        public const int HITS_MAX = 64;
        public sealed class RayHitLists { public int MaxHits; public uint[] Count; public int[] Index; public double[] RayFrac; public ulong[] Stats4; }
        public RayHitLists AllHitRays(double[] starts, double[] dirs, double[] limits, int maxHits, int mode, bool root = false, bool endpoints = false,
                                      bool coherent = false)
        {
            long n = starts.Length / 3;
            var r = new RayHitLists { MaxHits = maxHits, Count = new uint[n], Index = new int[n * Math.Max(0, maxHits)],
                                      RayFrac = new double[n * Math.Max(0, maxHits)], Stats4 = new ulong[4] };
            Native.Check(Native.sr_all_hits_rays(scene, mode | (root ? 0x100 : 0), n, starts, dirs, limits, maxHits, r.Count, r.Index, r.RayFrac,
                                                 (endpoints ? RAYS_ENDPOINTS : 0) | (coherent ? RAYS_COHERENT : 0), r.Stats4));
            return r;
        }

        /// The same with every array in DEVICE memory on the scene's device (sr_all_hits_rays_device), dLimits IntPtr.Zero for no limit and
        /// IntPtr.Zero for an output that is not wanted (dCount IntPtr.Zero with maxHits &gt; 0: a K-nearest query); enqueued on `stream` without a
        /// host synchronisation; dStats: ulong[24] on the device, or IntPtr.Zero.
        public void AllHitRaysDevice(long n, IntPtr dStarts, IntPtr dDirs, IntPtr dLimits, int maxHits, int mode, bool root, bool endpoints, bool coherent,
                                     IntPtr dCount, IntPtr dIndex, IntPtr dRayFrac, IntPtr stream, IntPtr dStats)
        {
            Native.Check(Native.sr_all_hits_rays_device(scene, mode | (root ? 0x100 : 0), n, dStarts, dDirs, dLimits, maxHits, dCount, dIndex, dRayFrac,
                                                        (endpoints ? RAYS_ENDPOINTS : 0) | (coherent ? RAYS_COHERENT : 0), stream, dStats));
        }

        /// The closest point of the mesh for each point of a batch (sr_closest_points).  TriIndex[i]: the triangle that minimises (squared
        /// distance, TriangleIndex), Dist[i] its distance, Pos ([n * 3]) the point of it nearest to points[i], Uv ([n * 2]) that point's weights of
        /// vertices 2 and 3 -- where Dist &lt;= maxDist[i] (maxDist == null: no limit); -1 and zeros otherwise.  mode is MODE_BVH or MODE_BRUTE
        /// (the reference tree has no distance query); the model alone, no extra geometry.  Blocks.
        public sealed class ClosestPointResult { public int[] TriIndex; public double[] Dist; public double[] Pos; public double[] Uv; public ulong[] Stats4; }
        public ClosestPointResult ClosestPoints(double[] points, double[] maxDist, int mode, bool coherent = false)
        {
            long n = points.Length / 3;
            var r = new ClosestPointResult { TriIndex = new int[n], Dist = new double[n], Pos = new double[n * 3], Uv = new double[n * 2], Stats4 = new ulong[4] };
            Native.Check(Native.sr_closest_points(scene, mode, n, points, maxDist, r.TriIndex, r.Dist, r.Pos, r.Uv, coherent ? POINTS_COHERENT : 0, r.Stats4));
            return r;
        }

        /// The same with every array in DEVICE memory on the scene's device (sr_closest_points_device), dMaxDist IntPtr.Zero for no limit and
        /// IntPtr.Zero for an output that is not wanted; enqueued on `stream` without a host synchronisation; dStats: ulong[24] on the device, or
        /// IntPtr.Zero.
        public void ClosestPointsDevice(long n, IntPtr dPoints, IntPtr dMaxDist, int mode, bool coherent, IntPtr dTriIndex, IntPtr dDist, IntPtr dPos,
                                        IntPtr dUv, IntPtr stream, IntPtr dStats)
        {
            Native.Check(Native.sr_closest_points_device(scene, mode, n, dPoints, dMaxDist, dTriIndex, dDist, dPos, dUv, coherent ? POINTS_COHERENT : 0, stream,
                                                         dStats));
        }

        /// The triangles within reach of each point of a batch, nearest first, with a count (sr_near_triangles).  Count[i]: the triangles whose
        /// distance is a number &lt;= maxDist[i] (maxDist == null: no limit; not capped by maxHits); rows i of Index / Dist ([n * maxHits]), Pos
        /// ([n * maxHits * 3]) and Uv ([n * maxHits * 2]): the first min(Count, maxHits) of them by (squared distance, TriangleIndex) -- slot 0 is
        /// ClosestPoints' answer -- the rest of a row -1 / zeros.  wantCount false: a K-nearest query (Count is null).  mode is MODE_BVH or
        /// MODE_BRUTE; the model alone, no extra geometry.  Blocks.
        public sealed class NearTriangleLists { public int MaxHits; public uint[] Count; public int[] Index; public double[] Dist; public double[] Pos; public double[] Uv; public ulong[] Stats4; }
        public NearTriangleLists NearTriangles(double[] points, double[] maxDist, int maxHits, int mode, bool wantCount = true, bool coherent = false)
        {
            long n = points.Length / 3;
            long rows = n * Math.Max(0, maxHits);
            var r = new NearTriangleLists { MaxHits = maxHits, Count = wantCount ? new uint[n] : null, Index = new int[rows], Dist = new double[rows],
                                            Pos = new double[rows * 3], Uv = new double[rows * 2], Stats4 = new ulong[4] };
            Native.Check(Native.sr_near_triangles(scene, mode, n, points, maxDist, maxHits, r.Count, r.Index, r.Dist, r.Pos, r.Uv, coherent ? POINTS_COHERENT : 0,
                                                  r.Stats4));
            return r;
        }

        /// The same with every array in DEVICE memory on the scene's device (sr_near_triangles_device), dMaxDist IntPtr.Zero for no limit and
        /// IntPtr.Zero for an output that is not wanted (dCount IntPtr.Zero with maxHits &gt; 0: a K-nearest query); enqueued on `stream` without a
        /// host synchronisation; dStats: ulong[24] on the device, or IntPtr.Zero.
        public void NearTrianglesDevice(long n, IntPtr dPoints, IntPtr dMaxDist, int maxHits, int mode, bool coherent, IntPtr dCount, IntPtr dIndex, IntPtr dDist,
                                        IntPtr dPos, IntPtr dUv, IntPtr stream, IntPtr dStats)
        {
            Native.Check(Native.sr_near_triangles_device(scene, mode, n, dPoints, dMaxDist, maxHits, dCount, dIndex, dDist, dPos, dUv,
                                                         coherent ? POINTS_COHERENT : 0, stream, dStats));
        }

        /// The triangles of the model that cross each triangle of a batch (sr_overlap_triangles; tris: [n * 9]).  Count[i]: the triangles that the
        /// pair predicate of softray.h reports (not capped by maxHits); rows i of Index / Mask ([n * maxHits]): the first min(Count, maxHits) of
        /// them by ascending TriangleIndex with the masks of their pairs (bit e: the query's edge e meets the scene triangle; bit 3 + e: the scene
        /// triangle's edge e meets the query), the rest of a row -1 / 0.  anyHit (SR_OVERLAP_ANY, maxHits must be 0): Count is 0 or 1.  mode is
        /// MODE_BVH or MODE_BRUTE; the model alone, no extra geometry.  Blocks.
        public const uint OVERLAP_ANY = 4;
        public sealed class OverlapTriangleLists { public int MaxHits; public uint[] Count; public int[] Index; public byte[] Mask; public ulong[] Stats4; }
        public OverlapTriangleLists OverlapTriangles(double[] tris, int maxHits, int mode, bool coherent = false, bool anyHit = false)
        {
            long n = tris.Length / 9;
            long rows = n * Math.Max(0, maxHits);
            var r = new OverlapTriangleLists { MaxHits = maxHits, Count = new uint[n], Index = new int[rows], Mask = new byte[rows], Stats4 = new ulong[4] };
            Native.Check(Native.sr_overlap_triangles(scene, mode, n, tris, maxHits, r.Count, r.Index, r.Mask, (coherent ? POINTS_COHERENT : 0) | (anyHit ? OVERLAP_ANY : 0),
                                                     r.Stats4));
            return r;
        }

        /// The same with every array in DEVICE memory on the scene's device (sr_overlap_triangles_device), IntPtr.Zero for an output that is not
        /// wanted; enqueued on `stream` without a host synchronisation; dStats: ulong[24] on the device, or IntPtr.Zero.
        public void OverlapTrianglesDevice(long n, IntPtr dTris, int maxHits, int mode, bool coherent, bool anyHit, IntPtr dCount, IntPtr dIndex, IntPtr dMask,
                                           IntPtr stream, IntPtr dStats)
        {
            Native.Check(Native.sr_overlap_triangles_device(scene, mode, n, dTris, maxHits, dCount, dIndex, dMask,
                                                            (coherent ? POINTS_COHERENT : 0) | (anyHit ? OVERLAP_ANY : 0), stream, dStats));
        }

        /// ShadingMethod's colour step for n recorded intersections in DEVICE memory (sr_shade_points_device): dOut[i] = dColor[i] modulated with
        /// the frame's lighting of (dPos[i], dNormal[i]); enqueued on `stream` without a host synchronisation.
        public void ShadePointsDevice(int width, int height, Instance instance, Matrix transform, Matrix inverseTransform, uint flags,
                                      double fieldOfViewDepth, double ambient, double shininess, Vector lightDirView, Vector lightPosView,
                                      long n, IntPtr dPos, IntPtr dNormal, IntPtr dColor, IntPtr dOut, IntPtr stream)
        {
            FillFrame(width, height, instance, transform, inverseTransform, 0, flags, MODE_BVH, 0, height - 1, 1, 0,
                      fieldOfViewDepth, 1.0, 0.0, ambient, shininess, lightDirView, lightPosView, 4);
            Native.Check(Native.sr_shade_points_device(scene, ref frame, n, dPos, dNormal, dColor, dOut, stream));
        }

        /// The host half of RaytraceGeometry (Renderer.cs:1510-1528, 1652-1653): copy public fields into sr_frame.
        public void Render(int width, int height, int[] pixels, Instance instance, Matrix transform, Matrix inverseTransform,
                           uint backgroundColor, uint flags, int mode, int startRow, int endRow, int subPixelRes, int randomSeed,
                           double fieldOfViewDepth, double focalDepth, double focalBlurStrength, double ambient, double shininess,
                           Vector lightDirView, Vector lightPosView, ulong[] stats4, int concurrency = 4)
        {
            FillFrame(width, height, instance, transform, inverseTransform, backgroundColor, flags, mode, startRow, endRow, subPixelRes, randomSeed,
                      fieldOfViewDepth, focalDepth, focalBlurStrength, ambient, shininess, lightDirView, lightPosView, concurrency);
            // blocking; `pixels` is only touched during the call (the library pins it for the call and copies row bands into it while
            // later bands still render).  The literal tree (and brute force) produce the reference's counters; the own BVH does not:
            // stats4 then gets the rays fired only and CountersAvailable turns false
            CountersAvailable = mode != MODE_BVH;
            ulong[] counters = CountersAvailable ? stats4 : null;
            Native.Check(Native.sr_render(scene, ref frame, pixels, counters), renderCall: true);
            if (!CountersAvailable && stats4 != null)
            {
                int a = Math.Min(Math.Max(0, startRow), height - 1), b = Math.Min(Math.Max(0, endRow), height - 1);   // Renderer.cs:1652-1653
                stats4[0] = b < a ? 0UL : (ulong)(b - a + 1) * (ulong)width * (ulong)(subPixelRes * subPixelRes);       // NumRaysFired (:1916)
                stats4[1] = stats4[2] = stats4[3] = 0;
            }
        }

        /// A new Renderer starts with an empty static shadow cache (ShadowMethod.cs:75-83)
        public void ResetShadowCache() { Native.Check(Native.sr_reset_shadow_cache(scene)); }
        /// The static shadow cache as the reference's softShadow_..._res128.cache file holds it: 128^3 bytes, [x][y][z], 0 = empty cell
        public byte[] GetShadowCache()
        {
            var data = new byte[AoCacheBytes];
            Native.Check(Native.sr_get_shadow_cache(scene, data));
            return data;
        }
        public void SetShadowCache(byte[] data)
        {
            if (data == null || data.Length != AoCacheBytes) throw new ArgumentException("the static shadow cache is 128^3 bytes");
            Native.Check(Native.sr_set_shadow_cache(scene, data));
        }

        /// A new Renderer starts with an empty ambient-occlusion cache (AmbientOcclusion.cs:60-75)
        public void ResetAmbientOcclusionCache() { Native.Check(Native.sr_reset_ao_cache(scene)); }
        /// The cache as the reference's .ao file holds it: 128^3 bytes, [x][y][z], 0 = empty cell
        public byte[] GetAmbientOcclusionCache()
        {
            var data = new byte[AoCacheBytes];
            Native.Check(Native.sr_get_ao_cache(scene, data));
            return data;
        }
        public void SetAmbientOcclusionCache(byte[] data)
        {
            if (data == null || data.Length != AoCacheBytes) throw new ArgumentException("the ambient-occlusion cache is 128^3 bytes");
            Native.Check(Native.sr_set_ao_cache(scene, data));
        }

        /// N of the N^3 voxel grid that F_VOXELS frames walk (VoxelGrid(N, ...), TriMeshToVoxelGrid.Convert(tris, N, grid)), 1..256, default 64 =
        /// voxelGridSize (Renderer.cs:1570); another value drops the grid, which the next voxel frame makes again.  The reference's cache file
        /// name carries it as _res{N}.
        public int VoxelResolution
        {
            get { return Native.sr_get_voxel_res(scene); }
            set { Native.Check(Native.sr_set_voxel_res(scene, value)); }
        }
        /// N of the light field's 4 N^4 entries, 1..128; another value drops the table
        public int LightFieldResolution
        {
            get { return Native.sr_get_light_field_res(scene); }
            set { Native.Check(Native.sr_set_light_field_res(scene, value)); }
        }
        /// Opt-in: SR_F_LIGHT_FIELD together with dynamic SR_F_SHADOWS (rayTraceLightField + rayTraceShadows, RendererTests.cs:240): the canonical
        /// rays go through ShadowMethod and the table stores shadowed colours.  Off (the default): that pair is SR_ERR_UNSUPPORTED.  Static
        /// shadows, AO, path tracing, voxels, mirror bounces, the one-kernel renderer and strips stay refused.  Does not touch the table.
        public bool LightFieldShadows
        {
            get { return Native.sr_get_light_field_shadows(scene) != 0; }
            set { Native.Check(Native.sr_set_light_field_shadows(scene, value ? 1 : 0)); }
        }
        /// Opt-in: LightFieldColorMethod.Interpolate (hard-wired false in the reference).  Light-field frames blend the 16 entries around a sample's
        /// RayToFloat4D coordinate instead of taking the one its line falls into.  Off (the default): nothing changes.  Does not touch the table.
        public bool LightFieldInterpolation
        {
            get { return Native.sr_get_light_field_interpolation(scene) != 0; }
            set { Native.Check(Native.sr_set_light_field_interpolation(scene, value ? 1 : 0)); }
        }
        /// Opt-in: LightFieldStoresTriangles = true (LightFieldTriMethod, Renderer.cs:1590-1611).  SR_F_LIGHT_FIELD frames and BakeLightField then run on the
        /// triangle table (0 empty, 1 nothing, t + 2 triangle t), which depends on the model alone; the reference tree must be built, SR_MODE_BRUTE and
        /// shadows are refused.  Does not touch either table (sr_set_light_field_triangles)
        public bool LightFieldTriangles
        {
            get { return Native.sr_get_light_field_triangles(scene) != 0; }
            set { Native.Check(Native.sr_set_light_field_triangles(scene, value ? 1 : 0)); }
        }
        /// entries.Length entries of the triangle table from index first
        public void GetLightFieldTris(uint[] entries, ulong first)
        {
            Native.Check(Native.sr_get_light_field_tris(scene, entries, first, (ulong)entries.Length));
        }
        public void SetLightFieldTris(uint[] entries, ulong first)
        {
            Native.Check(Native.sr_set_light_field_tris(scene, entries, first, (ulong)entries.Length));
        }
        /// LightField4D.RayToFloat4D in batch, on the device at LightFieldResolution: coords [n * 4], inside [n] (0: the line misses the sphere)
        public void LightFieldCoords(double[] starts, double[] dirs, double[] coords, byte[] inside)
        {
            Native.Check(Native.sr_light_field_coords(scene, inside.Length, starts, dirs, coords, inside));
        }
        /// A new Renderer starts with an empty light field (LightFieldColorMethod.cs:101-115)
        public void ResetLightField() { Native.Check(Native.sr_reset_light_field(scene)); }
        /// Entries first .. first + entries.Length - 1 of the table (0 = empty): ranges, so that the 256 MiB of N = 64 can be streamed
        public void GetLightField(uint[] entries, ulong first)
        {
            if (entries == null) throw new ArgumentNullException("entries");
            Native.Check(Native.sr_get_light_field(scene, entries, first, (ulong)entries.Length));
        }
        public void SetLightField(uint[] entries, ulong first)
        {
            if (entries == null) throw new ArgumentNullException("entries");
            Native.Check(Native.sr_set_light_field(scene, entries, first, (ulong)entries.Length));
        }

        /// PostProcessImage's colour functions (Renderer.cs:819-865): style = (int)Renderer.Style for Standard..DepthBanded.
        public void PostProcess(int[] pixels, int style, uint backgroundColor)
        {
            Native.Check(Native.sr_post_process(scene, pixels, pixels.LongLength, style, backgroundColor));
        }

        /// AntiAliasImage (Renderer.cs:937-978): surface.Pixels (dstWidth*res x dstHeight*res) -> antiAliasedSurface.Pixels.
        public void AntiAlias(int[] src, int dstWidth, int dstHeight, int resolution, int[] dst)
        {
            Native.Check(Native.sr_anti_alias(scene, src, dstWidth, dstHeight, resolution, dst));
        }

        public void Dispose()
        {
            if (offsetsPin.IsAllocated) offsetsPin.Free();
            if (scene != IntPtr.Zero) { Native.sr_destroy(scene); scene = IntPtr.Zero; }
        }
    }
}
