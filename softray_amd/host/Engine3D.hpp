// Engine3D.hpp -- C++17 host-side mirror of the reference's public raytrace API over the C ABI of
// include/softray.h.  The reference is compiled code (C#, .NET Framework 4.0) whose toolchain is absent
// here, so the host layer above the boundary is written in C++ with the reference's names, argument
// meaning and error behaviour:
//
//   Engine3D::Vector / Color                      Engine3D/Vector.cs, Engine3D/Color.cs
//   Engine3D::Raytrace::Sphere / Plane / Triangle / GeometryCollection
//                                                 Engine3D/Raytrace/{Sphere,Plane,Triangle,GeometryCollection}.cs
//   Engine3D::Model / Instance                    Engine3D/Model.cs, Engine3D/Instance.cs
//   Engine3D::Renderer                            Engine3D/Renderer.cs (raytrace half: :35-139, :593, :629, :673, :701)
//
// Header-only; link with -lsoftray_hip.  Nothing is traced on the host: Render() fills an sr_frame the way
// Renderer.RaytraceGeometry does (Renderer.cs:1501-1687) and calls sr_render.  Features outside the hot
// path (rasteriser, static shadows, AO, light field, path tracing, voxels) throw std::logic_error.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <istream>
#include <iterator>
#include <memory>
#include <stdexcept>
#include <string>
#include <variant>
#include <vector>

#include "../../include/softray.h"

namespace Engine3D {

struct ArgumentOutOfRangeException : std::out_of_range { using std::out_of_range::out_of_range; };   // SpatialSubdivision.cs:293
struct FormatException : std::runtime_error { using std::runtime_error::runtime_error; };           // Model.cs:555, ThreeDSFile.cs:168
struct InvalidOperationException : std::runtime_error { using std::runtime_error::runtime_error; };

inline void sr_check(int rc) {
    if (rc == SR_OK) return;
    std::string msg = sr_last_error();
    switch (rc) {
        case SR_ERR_OUT_OF_RANGE: throw ArgumentOutOfRangeException(msg);
        case SR_ERR_FORMAT: throw FormatException(msg);
        case SR_ERR_INVALID_ARG: throw std::invalid_argument(msg);
        default: throw InvalidOperationException(msg);
    }
}

struct Vector {                                            // Vector.cs:9-31
    double x = 0, y = 0, z = 0;
    Vector() = default;
    Vector(double x_, double y_, double z_) : x(x_), y(y_), z(z_) {}
    Vector operator-(const Vector& o) const { return {x - o.x, y - o.y, z - o.z}; }
    Vector operator*(double s) const { return {x * s, y * s, z * s}; }
    void Normalise() {                                     // Vector.cs:177-185
        double inv = 1.0 / std::sqrt(x * x + y * y + z * z);
        x *= inv; y *= inv; z *= inv;
    }
};

inline uint8_t ToByte(double d) {                          // C# unchecked (byte)(double)
    if (!(d > -2147483649.0 && d < 2147483648.0)) return 0;
    return (uint8_t)(int32_t)d;
}

struct Color {                                             // Color.cs:5-36
    double r = 0, g = 0, b = 0;
    uint32_t ToARGB() const {                              // Color.cs:105-111
        return (255u << 24) + ((uint32_t)ToByte(r * 255.0) << 16) + ((uint32_t)ToByte(g * 255.0) << 8) + ToByte(b * 255.0);
    }
    static Color White() { return {1, 1, 1}; }  static Color Red() { return {1, 0, 0}; }
    static Color Green() { return {0, 1, 0}; }  static Color Blue() { return {0, 0, 1}; }
    static Color Yellow() { return {1, 1, 0}; } static Color Cyan() { return {0, 1, 1}; }
};

namespace Raytrace {

struct Sphere {                                            // Sphere.cs:26-33
    Vector center; double radius; Engine3D::Color Color = Engine3D::Color::White();
    Sphere(Vector c, double r) : center(c), radius(r) { if (!(r > 0)) throw std::invalid_argument("radius > 0"); }
};
struct Plane {                                             // Plane.cs:22-29
    Vector point, normal; Engine3D::Color Color = Engine3D::Color::White();
    Plane(Vector p, Vector n) : point(p), normal(n) {}
};
struct Triangle {                                          // Triangle.cs:29-57
    Vector v1, v2, v3; uint32_t color;
    Triangle(Vector a, Vector b, Vector c, uint32_t col) : v1(a), v2(b), v3(c), color(col) {}
};

struct AxisAlignedBox {                                    // AxisAlignedBox.cs:15-28 as an IRayIntersectable (IntersectRay :60-95)
    Vector Min, Max;
    AxisAlignedBox(Vector mn, Vector mx) : Min(mn), Max(mx) {
        if (!(mn.x < mx.x && mn.y < mx.y && mn.z < mx.z)) throw std::invalid_argument("Axis aligned bounding box has bad coordinates");
    }
};

class GeometryCollection {                                 // GeometryCollection.cs:8-31
public:
    using Item = std::variant<Sphere, Plane, Triangle, AxisAlignedBox>;
    void Add(const Item& g) { items_.push_back(g); }
    int Count() const { return (int)items_.size(); }
    std::vector<sr_prim> ToPrims() const {
        std::vector<sr_prim> out;
        for (const Item& it : items_) {
            sr_prim p{};
            if (auto s = std::get_if<Sphere>(&it)) {
                p.kind = 0; p.argb = s->Color.ToARGB();
                p.p[0] = s->center.x; p.p[1] = s->center.y; p.p[2] = s->center.z; p.p[3] = s->radius;
            } else if (auto pl = std::get_if<Plane>(&it)) {
                p.kind = 1; p.argb = pl->Color.ToARGB();
                p.p[0] = pl->point.x; p.p[1] = pl->point.y; p.p[2] = pl->point.z;
                p.p[3] = pl->normal.x; p.p[4] = pl->normal.y; p.p[5] = pl->normal.z;
            } else if (auto b = std::get_if<AxisAlignedBox>(&it)) {
                p.kind = 4; p.argb = 0xffffffffu;          // its six planes are Color.White (Plane.cs:28)
                p.p[0] = b->Min.x; p.p[1] = b->Min.y; p.p[2] = b->Min.z; p.p[3] = b->Max.x; p.p[4] = b->Max.y; p.p[5] = b->Max.z;
            } else {
                const Triangle& t = std::get<Triangle>(it);
                p.kind = 2; p.argb = t.color;
                const Vector* v[3] = {&t.v1, &t.v2, &t.v3};
                for (int k = 0; k < 3; ++k) { p.p[3 * k] = v[k]->x; p.p[3 * k + 1] = v[k]->y; p.p[3 * k + 2] = v[k]->z; }
            }
            out.push_back(p);
        }
        return out;
    }
private:
    std::vector<Item> items_;
};

}  // namespace Raytrace

// Model after Load3ds + PostProcessGeometry (Model.cs:522-653,750-831): triangles scaled into the unit cube.
class Model {
public:
    bool LoadingComplete = false, LoadingError = false;   // Model.cs:199
    std::vector<double> v9;                                // [n][3][3]
    std::vector<uint32_t> argb;                            // PackColorAndAlpha(diffuse, 1.0), Renderer.cs:1463
    Vector Min, Max;

    void Load3dsModelFromStream(std::istream& stream) {
        std::vector<uint8_t> data((std::istreambuf_iterator<char>(stream)), std::istreambuf_iterator<char>());
        sr_scene* tmp = nullptr;
        sr_check(sr_create(-1, &tmp));                     // host-only handle: parsing is host work
        int rc = sr_load_3ds(tmp, data.data(), data.size());
        if (rc != SR_OK) { sr_destroy(tmp); LoadingError = true; sr_check(rc); }
        int64_t n = sr_num_triangles(tmp);
        v9.resize((size_t)n * 9); argb.resize((size_t)n);
        double mn[3], mx[3];
        sr_get_triangles(tmp, v9.data(), argb.data(), mn, mx);
        sr_destroy(tmp);
        Min = {mn[0], mn[1], mn[2]}; Max = {mx[0], mx[1], mx[2]};
        LoadingComplete = true; LoadingError = false;
    }
    int TriangleCount() const { return (int)argb.size(); }
};

class Instance {                                           // Instance.cs:21-51
public:
    explicit Instance(std::shared_ptr<Model> model) : Model_(std::move(model)) {
        if (!Model_) throw std::invalid_argument("model != null");
    }
    std::shared_ptr<Model> Model_;
    Vector Position{0.0, 0.0, 1.5};
    double Yaw = 0, Pitch = 0, Roll = 0;
    double FieldOfViewDepth = 0.5;
};

class Renderer {
public:
    enum class Style { Standard, ColorShuffle, Negative, DepthSmooth, DepthBanded, Normals, Count };   // Renderer.cs:23-33
    // ---- public fields, Renderer.cs:35-139 ----
    Style RenderStyle = Style::Standard;
    bool depthBuffer = false, depthBufferHires = false;    // only steer the two depth styles here (:837-863)
    double ambientLight_intensity = 0.1;
    Vector directionalLight_dir, positionalLight_pos;
    double specularLight_shininess = 100.0;
    bool pointLighting = true, specularLighting = true;
    bool rayTrace = false, rayTraceShading = true, rayTraceShadows = false, rayTraceShadowsStatic = false;
    bool rayTraceAmbientOcclusion = false, rayTraceLightField = false, rayTraceSubdivision = true;
    bool rayTracePathTracing = false, rayTraceVoxels = false, rayTraceFocalBlur = true;
    bool ambientOcclusionEnableCache = true;               // AmbientOcclusionMethod.EnableCache (Renderer.cs:74 TODO, RendererTests.cs:405); false = SR_F_AO_UNCACHED
    double rayTraceFocalDepth = 1.5, rayTraceFocalBlurStrength = 10.0;
    int rayTraceConcurrency = 4, rayTraceSubPixelRes = 1, rayTraceRandomSeed = 1234567890;
    int rayTraceStartRow = 0, rayTraceEndRow = 0;
    // MI355X additions: which structure the device walks (-1: chosen per model, see Mode())
    int gpuTraceMode = -1;
    // How NumGeometryTests / NumNodeVisits / NumLeafNodeVisits (Renderer.cs:476-504) are answered is an explicit choice of the
    // constructor: they are the literal reference-tree traversal's counters, and the fast path does not walk that tree.
    //   Literal  every model's primary rays walk the reference tree (SR_MODE_REF_TREE): the reference's counters, any model size;
    //   Auto     (default) models of fewer than gpuOwnBvhThreshold triangles -- the sizes the reference itself handles -- as Literal,
    //            larger ones as Off;
    //   Off      every subdivided model on the library's own BVH; reading one of the three counters throws InvalidOperationException
    //            (never a silent zero).
    // NumRaysFired is exact in every mode; shadow rays take the shaft path on the own BVH in all three (same pixels).
    enum class TraversalCounters { Auto, Literal, Off };
    const TraversalCounters gpuTraversalCounters;
    int gpuOwnBvhThreshold = 2000;
    int gpuMaxBounces = 0;          // config-5 extension: mirror bounces (0 = the reference's behaviour)
    double gpuReflectivity = 0.0;
    std::vector<std::shared_ptr<Instance>> Instances;
    Raytrace::GeometryCollection ExtraGeometryToRaytrace;

    explicit Renderer(int device = 0, TraversalCounters traversalCounters = TraversalCounters::Auto)   // Renderer.cs:207-230
        : gpuTraversalCounters(traversalCounters) {
        directionalLight_dir = Vector(-1, -1, 1);
        directionalLight_dir.Normalise();
        positionalLight_pos = Vector(0.0, 0.0, 1.5) - directionalLight_dir * 2;
        fieldOfViewDepth_ = sr_default_fov_depth();
        sr_check(sr_create(device, &scene_));
    }
    ~Renderer() { Dispose(); }
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;
    void Dispose() { if (scene_) { sr_destroy(scene_); scene_ = nullptr; } }   // Renderer.cs:236
    void ResetAmbientOcclusionCache() { sr_check(sr_reset_ao_cache(scene_)); }   // what a new Renderer's AmbientOcclusionMethod starts with
    // the static shadow cache (rayTraceShadowsStatic): 128^3 bytes in [x][y][z] order, 0 = empty -- the content of the reference's
    // softShadow_..._res128.cache file (Texture3DCache.SaveCacheToDisk / LoadCacheFromDisk); a new model drops what was set
    static constexpr size_t StaticShadowCacheBytes = (size_t)128 * 128 * 128;
    void GetStaticShadowCache(uint8_t* out) { sr_check(sr_get_shadow_cache(scene_, out)); }
    void SetStaticShadowCache(const uint8_t* in) { sr_check(sr_set_shadow_cache(scene_, in)); }
    // Renderer.cs:420-446: true (the default, as in the reference) = LightFieldTriMethod, which Render() refuses; false = the colour light
    // field, passed on as SR_F_LIGHT_FIELD.  Setting another value disposes of both methods: the light field starts empty again
    bool LightFieldStoresTriangles() const { return lightFieldHasTris_; }
    void LightFieldStoresTriangles(bool value) {
        if (value != lightFieldHasTris_) ResetLightField();
        lightFieldHasTris_ = value;
    }
    // library opt-in (sr_set_light_field_triangles): LightFieldStoresTriangles = true runs LightFieldTriMethod on the library's triangle table
    // instead of being refused.  Off (the default): Render() and BakeLightField() refuse LightFieldStoresTriangles = true, as they always did
    bool LightFieldTriangles() const { return lightFieldTris_; }
    void LightFieldTriangles(bool value) { lightFieldTris_ = value; }
    // ranges of the triangle table (4 N^4 uint32: 0 empty, 1 nothing, t + 2 triangle t), as sr_get_light_field_tris / sr_set_light_field_tris
    void GetLightFieldTris(uint32_t* out, uint64_t first, uint64_t count) { sr_check(sr_get_light_field_tris(scene_, out, first, count)); }
    void SetLightFieldTris(const uint32_t* in, uint64_t first, uint64_t count) { sr_check(sr_set_light_field_tris(scene_, in, first, count)); }
    void ResetLightField() { sr_check(sr_reset_light_field(scene_)); }           // what a new Renderer's light-field method starts with (both tables)
    int LightFieldResolution() const { return (int)sr_get_light_field_res(scene_); }   // lightFieldRes (Renderer.cs:93): 64
    void LightFieldResolution(int n) { sr_check(sr_set_light_field_res(scene_, n)); }
    // library opt-in (sr_set_light_field_shadows): rayTraceLightField together with DYNAMIC rayTraceShadows -- LightFieldColorMethod is the
    // outermost decorator (Renderer.cs:1640-1649), so the table then stores shadowed colours (RendererTests.cs:240).  Off: CheckLightField refuses
    bool LightFieldShadows() const { return sr_get_light_field_shadows(scene_) != 0; }
    void LightFieldShadows(bool value) { sr_check(sr_set_light_field_shadows(scene_, value ? 1 : 0)); }
    // LightFieldColorMethod.Interpolate (LightFieldColorMethod.cs:50, 142-181; hard-wired false in the reference): light-field frames blend the
    // 16 entries around a sample's RayToFloat4D coordinate (sr_set_light_field_interpolation).  Does not touch the table
    bool LightFieldInterpolate() const { return sr_get_light_field_interpolation(scene_) != 0; }
    void LightFieldInterpolate(bool value) { sr_check(sr_set_light_field_interpolation(scene_, value ? 1 : 0)); }
    // library extension: the reference has a constant there (voxelGridSize = 64, Renderer.cs:1570).  1..256; another value drops the grid,
    // which the next voxel frame makes again (sr_set_voxel_res)
    int VoxelGridSize() const { return (int)sr_get_voxel_res(scene_); }
    void VoxelGridSize(int n) { sr_check(sr_set_voxel_res(scene_, n)); }
    int gpuLastFrameParts() const { return scene_ ? sr_last_frame_parts(scene_) : 0; }   // parts (devices) that rendered rows of the last frame

    uint32_t BackgroundColor() const { return backgroundColor_; }
    void BackgroundColor(uint32_t v) { backgroundColor_ = v & 0x00FFFFFFu; }   // Renderer.cs:308-321
    uint32_t BackgroundColorWithAlpha() const { return backgroundColor_ | 0xFF000000u; }

    std::shared_ptr<Engine3D::Model> Model() const { return modelVolatile_; }
    void Model(std::shared_ptr<Engine3D::Model> m) {       // Renderer.cs:349-364
        modelVolatile_ = std::move(m);
        if (modelVolatile_) { modelVolatile_->LoadingComplete = true; modelVolatile_->LoadingError = false; }
    }

    int AntiAliasResolution() const { return antiAliasResolution_; }
    void AntiAliasResolution(int value) {                  // Renderer.cs:366-413
        if (value <= 0) throw std::invalid_argument("AntiAliasResolution must be greater than zero");
        if (value == antiAliasResolution_) return;
        int w = aaPixels_ ? aaWidth_ : width_, h = aaPixels_ ? aaHeight_ : height_;
        int32_t* pixels = aaPixels_ ? aaPixels_ : pixels_;   // restore the original surface
        antiAliasResolution_ = value;
        if (value == 1) {
            aaPixels_ = nullptr;
            hires_.clear();
        } else {
            aaPixels_ = pixels; aaWidth_ = w; aaHeight_ = h;
            w *= value; h *= value;
            hires_.assign((size_t)w * h, 0);               // larger surface for pre-anti-aliased rendering
            pixels = hires_.data();
        }
        SetSurface(w, h, pixels);
    }
    // caller owns `pixels` (int[width*height]); written in place (Renderer.cs:593-626)
    void SetRenderingSurface(int width, int height, int32_t* pixels) {
        const int n = antiAliasResolution_;
        if (width * n == width_ && height * n == height_) {   // unchanged resolution: swap the buffer only
            if (n > 1) aaPixels_ = pixels; else pixels_ = pixels;
            return;
        }
        if (n > 1) {
            aaPixels_ = pixels; aaWidth_ = width; aaHeight_ = height;
            width *= n; height *= n;
            hires_.assign((size_t)width * height, 0);
            pixels = hires_.data();
        }
        SetSurface(width, height, pixels);
    }
    void Load3dsModelFromStream(std::istream& stream) {    // Renderer.cs:629-635
        modelVolatile_ = std::make_shared<Engine3D::Model>();
        modelVolatile_->Load3dsModelFromStream(stream);
    }
    void PreCalculate() {                                  // Renderer.cs:673-699
        if (!PinModel()) throw InvalidOperationException("PreCalculate: no model is loading");
        if (!rayTrace) return;
        if (sceneModel_ != model_.get()) {
            double mn[3] = {model_->Min.x, model_->Min.y, model_->Min.z}, mx[3] = {model_->Max.x, model_->Max.y, model_->Max.z};
            sr_check(sr_set_triangles(scene_, model_->v9.data(), model_->argb.data(), (int64_t)model_->argb.size(), mn, mx));
            sceneModel_ = model_.get();
            built_ = 0;
        }
        int mode = Mode();
        uint32_t want = mode == SR_MODE_BRUTE ? 0u : (1u << mode);
        if (rayTraceVoxels) want = 0u;                     // a voxel frame walks the grid the library makes from the triangles (SR_F_VOXELS)
        if (mode == SR_MODE_REF_TREE && rayTraceShadows && !rayTraceShadowsStatic && !model_->argb.empty())
            want |= 1u << SR_MODE_BVH;                     // a tree frame's shadow rays take the BVH's shaft path
        if (rayTraceLightField && lightFieldHasTris_ && lightFieldTris_ && !rayTraceVoxels)
            want |= 1u << SR_MODE_REF_TREE;                // LightFieldTriMethod's second stage reads the reference tree whatever walks the full rays
        if (want & ~built_) {
            sr_check(sr_build(scene_, want & ~built_, 0, 0));  // SpatialSubdivision defaults 15 / 25
            built_ |= want;
        }
    }
    void Render() {                                        // Renderer.cs:701-778
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!PinModel()) return;                           // silently, :736-739
        if (rayTraceLightField) CheckLightField();         // SR_F_LIGHT_FIELD: the colour light field; what the library refuses, by name
        if (rayTraceAmbientOcclusion) {                    // SR_F_AMBIENT_OCCLUSION: the pairs the library refuses, by name
            if (rayTracePathTracing) throw std::logic_error("rayTraceAmbientOcclusion together with rayTracePathTracing is out of scope (SR_F_AMBIENT_OCCLUSION)");
            if (rayTraceVoxels) throw std::logic_error("rayTraceAmbientOcclusion together with rayTraceVoxels is out of scope (SR_F_AMBIENT_OCCLUSION)");
            if (rayTraceShadows && rayTraceShadowsStatic)
                throw std::logic_error("rayTraceAmbientOcclusion together with rayTraceShadowsStatic is out of scope (SR_F_AMBIENT_OCCLUSION)");
            if (gpuMaxBounces > 0) throw std::logic_error("rayTraceAmbientOcclusion together with gpuMaxBounces is out of scope (SR_F_AMBIENT_OCCLUSION)");
        }
        if (rayTraceVoxels && (rayTraceShadows || rayTracePathTracing || gpuMaxBounces > 0))   // SR_F_VOXELS: the reference's result there is a rayFrac = 0 artefact
            throw std::logic_error("rayTraceVoxels together with rayTraceShadows, rayTracePathTracing or mirror bounces is out of scope (SR_F_VOXELS)");
        if (rayTracePathTracing && rayTraceShadows)
            throw std::logic_error("rayTracePathTracing together with rayTraceShadows is out of scope (SR_F_PATH_TRACING)");
        for (auto& inst : Instances) {
            inst->FieldOfViewDepth = fieldOfViewDepth_;    // :749
            RaytraceGeometry(*inst);
        }
        PostProcessImage();                                // :765
        AntiAliasImage();                                  // :767
    }
    // Pre-compute the colour light field (sr_bake_light_field): every entry that is still empty gets the colour of its cell's canonical ray, with
    // the frame Render() would build for the first instance -- its geometry, shading, pose and lights.  Frames rendered afterwards look their
    // colours up and trace nothing.  The same refusals as Render(); returns the number of entries written (0 without a model)
    uint64_t BakeLightField() {
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!rayTraceLightField) throw std::logic_error("BakeLightField needs rayTraceLightField (with LightFieldStoresTriangles = false)");
        if (!PinModel()) return 0;
        CheckLightField();
        if (Instances.empty()) throw InvalidOperationException("BakeLightField: no instance to take the pose from");
        Instance& inst = *Instances.front();
        inst.FieldOfViewDepth = fieldOfViewDepth_;
        PreCalculate();
        std::vector<sr_prim> prims = ExtraGeometryToRaytrace.ToPrims();
        sr_check(sr_set_extra_geometry(scene_, prims.data(), (int32_t)prims.size()));
        sr_frame f = BuildFrame(inst);
        const uint64_t n = (uint64_t)LightFieldResolution();
        uint64_t filled = 0;
        sr_check(sr_bake_light_field(scene_, &f, 0, 4 * n * n * n * n, &filled));
        return filled;
    }
    // The colour light field for n lines of the caller's (sr_light_field_rays): out[i] = the colour LightFieldColorMethod.IntersectRay gives the ray
    // (starts[i], dirs[i]) -- [n][3] in model space, the direction not normalised -- with the frame Render() would build for the first instance:
    // its geometry, shading, pose and lights; rayTraceLightField is implied.  An empty entry of the renderer's light field -- the one its frames
    // and BakeLightField() fill -- is filled first.  inside (or nullptr): 1 where the line pierces the sphere; a line that misses it gets the
    // background.  Returns the number of entries written (0 without a model or rays).  LightFieldStoresTriangles = true is refused by the
    // library, by name, like everything Render() refuses of a light-field frame
    uint64_t LightFieldRays(int64_t n, const double* starts, const double* dirs, uint32_t* out, uint8_t* inside = nullptr) {
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!PinModel() || n == 0) return 0;
        if (Instances.empty()) throw InvalidOperationException("LightFieldRays: no instance to take the pose from");
        Instance& inst = *Instances.front();
        inst.FieldOfViewDepth = fieldOfViewDepth_;
        PreCalculate();
        std::vector<sr_prim> prims = ExtraGeometryToRaytrace.ToPrims();
        sr_check(sr_set_extra_geometry(scene_, prims.data(), (int32_t)prims.size()));
        sr_frame f = BuildFrame(inst);
        f.flags &= ~(uint32_t)SR_F_PRIMARY_STATS_ONLY;     // (sr_last_ray_stats gets the canonical rays' counters)
        sr_check(sr_set_light_field_triangles(scene_, lightFieldHasTris_ ? 1 : 0));   // (as CheckLightField: true is the library's to refuse)
        uint64_t filled = 0;
        sr_check(sr_light_field_rays(scene_, &f, n, starts, dirs, out, inside, 0u, &filled));
        return filled;
    }
    // ShadowMethod's soft shadow for n surface points of the caller (sr_shadow_points): out[i] = color[i] (nullptr: 0xFFFFFFFF) modulated with the
    // byte of the light, the shadow samples and the root geometry of the frame Render() would build for the first instance; rayTraceShadows is
    // implied.  pos / normal: [n][3] in model space, the normal as given.  coherent: 64 consecutive points are neighbours (SR_POINTS_COHERENT).
    // What names no step of ShadowMethod on a bare point (static shadows, ambient occlusion, path tracing, voxels, light field, mirror
    // bounces) is refused by the library, by name.  Does nothing without a model or points
    void ShadowPoints(int64_t n, const double* pos, const double* normal, const uint32_t* color, uint32_t* out, bool coherent = false) {
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!PinModel() || n == 0) return;
        if (Instances.empty()) throw InvalidOperationException("ShadowPoints: no instance to take the pose from");
        Instance& inst = *Instances.front();
        inst.FieldOfViewDepth = fieldOfViewDepth_;
        PreCalculate();
        if (Mode() == SR_MODE_REF_TREE && !(built_ & (1u << SR_MODE_BVH)) && !model_->argb.empty()) {   // (the shaft path, as for a shadowed tree frame)
            sr_check(sr_build(scene_, 1u << SR_MODE_BVH, 0, 0));
            built_ |= 1u << SR_MODE_BVH;
        }
        std::vector<sr_prim> prims = ExtraGeometryToRaytrace.ToPrims();
        sr_check(sr_set_extra_geometry(scene_, prims.data(), (int32_t)prims.size()));
        sr_frame f = BuildFrame(inst);
        f.flags &= ~(uint32_t)SR_F_PRIMARY_STATS_ONLY;     // (the call has no primary rays: sr_last_ray_stats gets the shadow stage's counters)
        sr_check(sr_shadow_points(scene_, &f, n, pos, normal, color, out, coherent ? SR_POINTS_COHERENT : 0u));
    }
    // ShadowMethod's static branch for n surface points of the caller, in input order (sr_static_shadow_points): the first point of an empty
    // cell of the renderer's static shadow cache -- the one its rayTraceShadowsStatic frames fill -- generates the cell's byte, amount[i] = the
    // byte of point i's cell, out[i] = color[i] (nullptr: 0xFFFFFFFF) modulated with it; either output may be nullptr, not both.  Light, samples
    // and root geometry are those of the frame Render() would build for the first instance; rayTraceShadows and rayTraceShadowsStatic are
    // implied.  coherent: SR_POINTS_COHERENT.  Returns the number of generators (0 without a model or points).  Ambient occlusion, path
    // tracing, voxels, the light field and mirror bounces are refused by the library, by name
    uint64_t StaticShadowPoints(int64_t n, const double* pos, const double* normal, const uint32_t* color, uint32_t* out, uint8_t* amount,
                                bool coherent = false) {
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!PinModel() || n == 0) return 0;
        if (Instances.empty()) throw InvalidOperationException("StaticShadowPoints: no instance to take the pose from");
        Instance& inst = *Instances.front();
        inst.FieldOfViewDepth = fieldOfViewDepth_;
        PreCalculate();
        std::vector<sr_prim> prims = ExtraGeometryToRaytrace.ToPrims();
        sr_check(sr_set_extra_geometry(scene_, prims.data(), (int32_t)prims.size()));
        sr_frame f = BuildFrame(inst);
        f.flags &= ~(uint32_t)SR_F_PRIMARY_STATS_ONLY;     // (the call has no primary rays: sr_last_ray_stats gets the shadow stage's counters)
        uint64_t generators = 0;
        sr_check(sr_static_shadow_points(scene_, &f, n, pos, normal, color, out, amount, coherent ? SR_POINTS_COHERENT : 0u, &generators));
        return generators;
    }
    // AmbientOcclusionMethod's occlusion byte for n surface points of the caller, in input order (sr_ao_points): amount[i] = the byte, out[i] =
    // color[i] (nullptr: 0xFFFFFFFF) modulated with it; either output may be nullptr, not both.  The root geometry, the seed and the cache
    // switch (ambientOcclusionEnableCache) are those of the frame Render() would build for the first instance; rayTraceAmbientOcclusion is
    // implied, the cache is the one the renderer's AO frames fill.  Generator g of the call uses draws 300 (firstGenerator + g) .. + 299 of the
    // frame's Random; returns the number of generators, which a caller that splits a batch adds to firstGenerator of the next call.
    // Static shadows, path tracing, voxels, the light field and mirror bounces are refused by the library, by name.  Returns 0 without a
    // model or points
    uint64_t AmbientOcclusionPoints(int64_t n, const double* pos, const double* normal, const uint32_t* color, uint32_t* out, uint8_t* amount,
                                    uint64_t firstGenerator = 0) {
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!PinModel() || n == 0) return 0;
        if (Instances.empty()) throw InvalidOperationException("AmbientOcclusionPoints: no instance to take the pose from");
        Instance& inst = *Instances.front();
        inst.FieldOfViewDepth = fieldOfViewDepth_;
        PreCalculate();
        std::vector<sr_prim> prims = ExtraGeometryToRaytrace.ToPrims();
        sr_check(sr_set_extra_geometry(scene_, prims.data(), (int32_t)prims.size()));
        sr_frame f = BuildFrame(inst);
        f.flags &= ~(uint32_t)(SR_F_PRIMARY_STATS_ONLY | SR_F_AO_UNCACHED);     // (the call has no primary rays: sr_last_ray_stats gets the probes' counters)
        if (!ambientOcclusionEnableCache) f.flags |= SR_F_AO_UNCACHED;          // (BuildFrame sets it for rayTraceAmbientOcclusion frames only)
        uint64_t generators = 0;
        sr_check(sr_ao_points(scene_, &f, n, pos, normal, color, out, amount, firstGenerator, 0u, &generators));
        return generators;
    }
    // PathTracingMethod's one-bounce diffuse term for n surface points of the caller, in input order (sr_path_points): point i fires one second
    // ray from pos[i] + normal[i] * 0.001 in the direction made of draws 3 (firstSample + i) .. + 2 of the frame's Random; incoming[i] = that
    // hit's colour (shaded when rayTraceShading is on, 0 on a miss), out[i] = incoming * (normal . d) + color[i] (nullptr: 0xFFFFFFFF),
    // dirs[i] = d; each output may be nullptr, not all three.  The root geometry, the seed and the shading switch are those of the frame
    // Render() would build for the first instance; rayTracePathTracing is implied, the shadow and ambient-occlusion switches are not
    // passed on (their steps are ShadowPoints and AmbientOcclusionPoints, which follow this one in the reference's chain).  A caller that
    // splits a batch passes firstSample + n to the next call.  Voxels, the light field and mirror bounces are refused by the library, by
    // name.  Does nothing without a model or points
    void PathTracePoints(int64_t n, const double* pos, const double* normal, const uint32_t* color, uint32_t* out, uint32_t* incoming, double* dirs,
                         uint64_t firstSample = 0) {
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!PinModel() || n == 0) return;
        if (Instances.empty()) throw InvalidOperationException("PathTracePoints: no instance to take the pose from");
        Instance& inst = *Instances.front();
        inst.FieldOfViewDepth = fieldOfViewDepth_;
        PreCalculate();
        std::vector<sr_prim> prims = ExtraGeometryToRaytrace.ToPrims();
        sr_check(sr_set_extra_geometry(scene_, prims.data(), (int32_t)prims.size()));
        sr_frame f = BuildFrame(inst);
        // (the call has no primary rays: sr_last_ray_stats gets the second rays' counters)
        f.flags &= ~(uint32_t)(SR_F_PRIMARY_STATS_ONLY | SR_F_SHADOWS | SR_F_STATIC_SHADOWS | SR_F_AMBIENT_OCCLUSION | SR_F_AO_UNCACHED);
        sr_check(sr_path_points(scene_, &f, n, pos, normal, color, out, incoming, dirs, firstSample, 0u));
    }
    // The frame G-buffer (sr_render_hits): what the primary stage of the frame Render() would build for the first instance answers per camera
    // sample, before any decorator, in scan order ((row - first row) * width + col) * n^2 + subX * n + subY.  Every array has
    // RenderHitsSamples() entries ([S][3] doubles, [S] scalars) and may be nullptr; a miss is hit 0, zeros and triangle -1.  The decorator
    // switches (shading, shadows, ambient occlusion, path tracing, gpuMaxBounces) are not read; voxels and the light field are refused by
    // the library, by name.  Does nothing without a model
    int64_t RenderHitsSamples() const {
        const int a = std::min(std::max(0, rayTraceStartRow), height_ - 1), b = std::min(std::max(0, rayTraceEndRow), height_ - 1);
        return b < a ? 0 : (int64_t)(b - a + 1) * width_ * rayTraceSubPixelRes * rayTraceSubPixelRes;
    }
    void RenderHits(double* starts, double* dirs, uint8_t* hit, double* ray_frac, double* pos, double* normal, uint32_t* color, int32_t* tri_index) {
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!PinModel()) return;
        if (Instances.empty()) throw InvalidOperationException("RenderHits: no instance to take the pose from");
        Instance& inst = *Instances.front();
        inst.FieldOfViewDepth = fieldOfViewDepth_;
        PreCalculate();
        std::vector<sr_prim> prims = ExtraGeometryToRaytrace.ToPrims();
        sr_check(sr_set_extra_geometry(scene_, prims.data(), (int32_t)prims.size()));
        rayTraceStartRow = std::min(std::max(0, rayTraceStartRow), height_ - 1);   // :1652-1653, as Render() does
        rayTraceEndRow = std::min(std::max(0, rayTraceEndRow), height_ - 1);
        sr_frame f = BuildFrame(inst);
        sr_check(sr_render_hits(scene_, &f, starts, dirs, hit, ray_frac, pos, normal, color, tri_index, nullptr));
    }
    // Nearest hits of n rays that start in one model-space point (sr_trace_origin_rays): IntersectRay(origin, dirs[i]) on the root geometry of
    // the chain (extra geometry + the model in the renderer's mode), bit for bit, on the packet walk of a frame's camera rays.  dirs is [n][3],
    // not normalised; every output may be nullptr; coherent: every 64 consecutive rays are neighbours (SR_RAYS_COHERENT).  The scene's
    // per-origin records are re-keyed to `origin`, as by a camera move.  Does nothing without a model
    void TraceOriginRays(const Vector& origin, int64_t n, const double* dirs, uint8_t* hit, double* ray_frac, double* pos, double* normal, uint32_t* color,
                         int32_t* tri_index, bool coherent = false) {
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!PinModel()) return;
        std::vector<sr_prim> prims = ExtraGeometryToRaytrace.ToPrims();
        sr_check(sr_set_extra_geometry(scene_, prims.data(), (int32_t)prims.size()));
        const double o[3] = {origin.x, origin.y, origin.z};
        sr_check(sr_trace_origin_rays(scene_, SR_TARGET_ROOT | Mode(), o, n, dirs, hit, ray_frac, pos, normal, color, tri_index, coherent ? SR_RAYS_COHERENT : 0u, nullptr));
    }
    // "Is anything in the way before distance L" for n rays of the caller's (sr_occluded_rays): occluded[i] = 1 iff IntersectRay(starts[i], D_i) on
    // the root geometry of the chain hits with rayFrac <= limits[i] (limits == nullptr: 1.0 for every ray), else 0 -- the test of ShadowMethod.cs:
    // 169-172, with early exit on the own BVH.  D_i = dirs[i], or with endpoints dirs[i] - starts[i] (dirs holds end points: "the segment is
    // blocked").  coherent: the rays are walked in the order given (SR_RAYS_COHERENT).  Does nothing without a model
    void OccludedRays(int64_t n, const double* starts, const double* dirs, const double* limits, uint8_t* occluded, bool endpoints = false, bool coherent = false) {
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!PinModel()) return;
        PreCalculate();                                    // the model and the tree of Mode() are in the scene
        std::vector<sr_prim> prims = ExtraGeometryToRaytrace.ToPrims();
        sr_check(sr_set_extra_geometry(scene_, prims.data(), (int32_t)prims.size()));
        sr_check(sr_occluded_rays(scene_, SR_TARGET_ROOT | Mode(), n, starts, dirs, limits, occluded,
                                  (endpoints ? SR_RAYS_ENDPOINTS : 0u) | (coherent ? SR_RAYS_COHERENT : 0u), nullptr));
    }
    // The nearest hit of n rays of the caller's within a distance (sr_nearest_rays): IntersectRay(starts[i], D_i) on the root geometry of the
    // chain where it hits with rayFrac <= limits[i] (limits == nullptr: no limit), a miss (hit 0, zeros, tri_index -1) otherwise, bit for bit, on
    // the walk a mirror level's rays take.  D_i = dirs[i], or with endpoints dirs[i] - starts[i]; every output may be nullptr; coherent: the rays
    // are walked in the order given (SR_RAYS_COHERENT).  Reflections, refractions, gathers, a second bounce.  Does nothing without a model
    void NearestRays(int64_t n, const double* starts, const double* dirs, const double* limits, uint8_t* hit, double* ray_frac, double* pos, double* normal,
                     uint32_t* color, int32_t* tri_index, bool endpoints = false, bool coherent = false) {
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!PinModel()) return;
        PreCalculate();                                    // the model and the tree of Mode() are in the scene
        std::vector<sr_prim> prims = ExtraGeometryToRaytrace.ToPrims();
        sr_check(sr_set_extra_geometry(scene_, prims.data(), (int32_t)prims.size()));
        sr_check(sr_nearest_rays(scene_, SR_TARGET_ROOT | Mode(), n, starts, dirs, limits, hit, ray_frac, pos, normal, color, tri_index,
                                 (endpoints ? SR_RAYS_ENDPOINTS : 0u) | (coherent ? SR_RAYS_COHERENT : 0u), nullptr));
    }
    // Every hit of n rays of the caller's, nearest first, with a count (sr_all_hits_rays) on the root geometry of the chain: count[i] = the hits
    // with rayFrac <= limits[i] (limits == nullptr: no limit; not capped by max_hits), rows i of index / ray_frac ([n][max_hits]) the first
    // min(count, max_hits) of them by (rayFrac, extra elements first, index) -- TriangleIndex, or -2 - e for extra element e -- the rest of a row
    // -1 / 0.0.  Any output may be nullptr (count == nullptr: a K-nearest query); max_hits 0 .. SR_HITS_MAX.  Needs the own BVH or brute force:
    // the literal reference tree has no notion of all hits (the library refuses it).  Does nothing without a model
    void AllHitRays(int64_t n, const double* starts, const double* dirs, const double* limits, int32_t max_hits, uint32_t* count, int32_t* index,
                    double* ray_frac, bool endpoints = false, bool coherent = false) {
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!PinModel()) return;
        PreCalculate();                                    // the model and the tree of Mode() are in the scene
        std::vector<sr_prim> prims = ExtraGeometryToRaytrace.ToPrims();
        sr_check(sr_set_extra_geometry(scene_, prims.data(), (int32_t)prims.size()));
        sr_check(sr_all_hits_rays(scene_, SR_TARGET_ROOT | Mode(), n, starts, dirs, limits, max_hits, count, index, ray_frac,
                                  (endpoints ? SR_RAYS_ENDPOINTS : 0u) | (coherent ? SR_RAYS_COHERENT : 0u), nullptr));
    }
    // The closest point of the model for n points of the caller's (sr_closest_points): tri_index[i] = the triangle that minimises (squared
    // distance, TriangleIndex), dist[i] its distance, pos[i] ([n][3]) the point of it nearest to points[i], uv[i] ([n][2]) that point's weights
    // of vertices 2 and 3 -- where dist <= max_dist[i] (max_dist == nullptr: no limit); -1 and zeros otherwise.  Any output may be nullptr.
    // The model alone (no extra geometry); needs the own BVH or brute force: the reference tree has no distance query (the library refuses
    // it).  coherent: SR_POINTS_COHERENT.  Does nothing without a model
    void ClosestPoints(int64_t n, const double* points, const double* max_dist, int32_t* tri_index, double* dist, double* pos, double* uv,
                       bool coherent = false) {
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!PinModel()) return;
        PreCalculate();                                    // the model and the tree of Mode() are in the scene
        sr_check(sr_closest_points(scene_, Mode(), n, points, max_dist, tri_index, dist, pos, uv, coherent ? SR_POINTS_COHERENT : 0u, nullptr));
    }
    // The triangles within reach of n points of the caller's, nearest first, with a count (sr_near_triangles): count[i] = the triangles whose
    // distance is a number <= max_dist[i] (max_dist == nullptr: no limit; not capped by max_hits), rows i of index / dist / pos / uv
    // ([n][max_hits], [n][max_hits], [n][max_hits][3], [n][max_hits][2]) the first min(count, max_hits) of them by (squared distance,
    // TriangleIndex) -- slot 0 is ClosestPoints' answer -- the rest of a row -1 / zeros.  Any output may be nullptr (count == nullptr: a
    // K-nearest query); max_hits 0 .. SR_HITS_MAX.  The model alone; needs the own BVH or brute force (the library refuses the reference
    // tree).  coherent: SR_POINTS_COHERENT.  Does nothing without a model
    void NearTriangles(int64_t n, const double* points, const double* max_dist, int32_t max_hits, uint32_t* count, int32_t* index, double* dist, double* pos,
                       double* uv, bool coherent = false) {
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!PinModel()) return;
        PreCalculate();                                    // the model and the tree of Mode() are in the scene
        sr_check(sr_near_triangles(scene_, Mode(), n, points, max_dist, max_hits, count, index, dist, pos, uv, coherent ? SR_POINTS_COHERENT : 0u, nullptr));
    }
    // The triangles of the model that cross n triangles of the caller's (sr_overlap_triangles; tris [n][3][3]): count[i] = the triangles that
    // the pair predicate of softray.h reports (not capped by max_hits), rows i of index / mask ([n][max_hits]) the first min(count, max_hits)
    // of them by ascending TriangleIndex with the masks of their pairs (bit e: the query's edge e meets the scene triangle; bit 3 + e: the
    // scene triangle's edge e meets the query), the rest of a row -1 / 0.  Any output may be nullptr; max_hits 0 .. SR_HITS_MAX.  any_hit:
    // SR_OVERLAP_ANY (count is 0 or 1; max_hits must be 0).  The model alone; needs the own BVH or brute force (the library refuses the
    // reference tree).  coherent: SR_POINTS_COHERENT.  Does nothing without a model
    void OverlapTriangles(int64_t n, const double* tris, int32_t max_hits, uint32_t* count, int32_t* index, uint8_t* mask, bool coherent = false,
                          bool any_hit = false) {
        if (!rayTrace) throw std::logic_error("the scan-line rasteriser is out of scope of the MI355X hot path");
        if (!PinModel()) return;
        PreCalculate();                                    // the model and the tree of Mode() are in the scene
        sr_check(sr_overlap_triangles(scene_, Mode(), n, tris, max_hits, count, index, mask, (coherent ? SR_POINTS_COHERENT : 0u) | (any_hit ? SR_OVERLAP_ANY : 0u),
                                      nullptr));
    }
    // Renderer.cs:465-504
    int64_t NumRaysFired() const { return (int64_t)stats_[0]; }
    int64_t NumGeometryTests() const { return Counter(1, "NumGeometryTests"); }
    int64_t NumNodeVisits() const { return Counter(2, "NumNodeVisits"); }
    int64_t NumLeafNodeVisits() const { return Counter(3, "NumLeafNodeVisits"); }
    bool TraversalCountersAvailable() const { return haveCounters_; }

    sr_frame BuildFrame(const Instance& instance) const {  // the host half of RaytraceGeometry, :1510-1528,:1652
        sr_frame f{};
        f.width = width_; f.height = height_;
        f.start_row = rayTraceStartRow; f.end_row = rayTraceEndRow;
        f.sub_pixel_res = rayTraceSubPixelRes;
        f.background_argb = backgroundColor_;
        f.flags = (rayTraceShading ? SR_F_SHADING : 0u) | (rayTraceShadows ? SR_F_SHADOWS : 0u) |
                  (rayTraceShadows && rayTraceShadowsStatic ? SR_F_STATIC_SHADOWS : 0u) |      // Renderer.cs:1625; the cache lives in the scene
                  (rayTraceFocalBlur ? SR_F_FOCAL_BLUR : 0u) |
                  (rayTracePathTracing ? SR_F_PATH_TRACING : 0u) |                                 // Renderer.cs:1613-1618; reads random_seed, concurrency
                  (rayTraceAmbientOcclusion ? SR_F_AMBIENT_OCCLUSION : 0u) |                       // Renderer.cs:1631-1638; reads random_seed, concurrency
                  (rayTraceAmbientOcclusion && !ambientOcclusionEnableCache ? SR_F_AO_UNCACHED : 0u) |
                  (rayTraceVoxels ? SR_F_VOXELS : 0u) |                                            // Renderer.cs:1568-1588: the grid replaces tree and extra geometry
                  (rayTraceLightField && (!lightFieldHasTris_ || lightFieldTris_) ? SR_F_LIGHT_FIELD : 0u) |   // Renderer.cs:1590-1611, 1640-1649: the colour or (opt-in) the triangle method
                  (pointLighting ? SR_F_POINT_LIGHT : 0u) | (specularLighting ? SR_F_SPECULAR : 0u) |
                  SR_F_PRIMARY_STATS_ONLY;                 // Num* count primary rays (Renderer.cs:1916-1923)
        f.random_seed = rayTraceRandomSeed;
        f.trace_mode = Mode();
        f.max_bounces = gpuMaxBounces;
        f.concurrency = rayTraceConcurrency;              // the fill order of the static shadow / AO caches, the row blocks of path tracing and AO
        f.reflectivity = gpuReflectivity;
        double pos[3] = {instance.Position.x, instance.Position.y, instance.Position.z};
        sr_instance_matrices(pos, instance.Yaw, instance.Pitch, instance.Roll, f.transform, f.inv_transform);   // Instance.cs:134-135
        f.position_z = instance.Position.z;
        f.fov_depth = instance.FieldOfViewDepth;
        f.focal_depth = rayTraceFocalDepth; f.focal_blur_strength = rayTraceFocalBlurStrength;
        f.ambient = ambientLight_intensity; f.shininess = specularLight_shininess;
        f.light_dir_view[0] = directionalLight_dir.x; f.light_dir_view[1] = directionalLight_dir.y; f.light_dir_view[2] = directionalLight_dir.z;
        f.light_pos_view[0] = positionalLight_pos.x; f.light_pos_view[1] = positionalLight_pos.y; f.light_pos_view[2] = positionalLight_pos.z;
        return f;
    }

private:
    void SetSurface(int width, int height, int32_t* pixels) {   // Renderer.cs:617-626
        pixels_ = pixels; width_ = width; height_ = height;
        rayTraceStartRow = 0; rayTraceEndRow = height - 1;
    }
    void PostProcessImage() {                              // Renderer.cs:819-897
        if ((RenderStyle == Style::DepthSmooth || RenderStyle == Style::DepthBanded) && (depthBufferHires || !depthBuffer)) return;
        if (RenderStyle == Style::Normals) {
            if (depthBuffer || depthBufferHires) throw std::logic_error("Style.Normals reads the rasteriser's depth buffer (out of scope)");
            return;
        }
        if (RenderStyle != Style::Standard)
            sr_check(sr_post_process(scene_, pixels_, (int64_t)width_ * height_, (int32_t)RenderStyle, backgroundColor_));
    }
    void AntiAliasImage() {                                // Renderer.cs:937-978
        if (antiAliasResolution_ < 2) return;
        sr_check(sr_anti_alias(scene_, pixels_, aaWidth_, aaHeight_, antiAliasResolution_, aaPixels_));
    }
    // what the library refuses, by name; then the scene's switch follows LightFieldStoresTriangles (only with the opt-in can it be on)
    void CheckLightField() const {
        if (lightFieldHasTris_ && !lightFieldTris_)
            throw std::logic_error("rayTraceLightField with LightFieldStoresTriangles = true (LightFieldTriMethod) is out of scope: set it to false (SR_F_LIGHT_FIELD), "
                                   "or opt in with LightFieldTriangles(true) (sr_set_light_field_triangles)");
        if (rayTraceShadows && (lightFieldHasTris_ || !(LightFieldShadows() && !rayTraceShadowsStatic)))      // (dynamic shadows only, only with the opt-in, never through LightFieldTriMethod)
            throw std::logic_error("rayTraceLightField together with rayTraceShadows is out of scope (SR_F_LIGHT_FIELD)");
        if (lightFieldHasTris_ && !rayTraceSubdivision)
            throw std::logic_error("rayTraceLightField with LightFieldStoresTriangles = true needs rayTraceSubdivision (LightFieldTriMethod reads the SpatialSubdivision)");
        sr_check(sr_set_light_field_triangles(scene_, lightFieldHasTris_ ? 1 : 0));
        if (rayTraceAmbientOcclusion) throw std::logic_error("rayTraceLightField together with rayTraceAmbientOcclusion is out of scope (SR_F_LIGHT_FIELD)");
        if (rayTracePathTracing) throw std::logic_error("rayTraceLightField together with rayTracePathTracing is out of scope (SR_F_LIGHT_FIELD)");
        if (rayTraceVoxels) throw std::logic_error("rayTraceLightField together with rayTraceVoxels is out of scope (SR_F_LIGHT_FIELD)");
        if (gpuMaxBounces > 0) throw std::logic_error("rayTraceLightField together with gpuMaxBounces is out of scope (SR_F_LIGHT_FIELD)");
    }
    int64_t Counter(int i, const char* name) const {
        if (!haveCounters_)
            throw InvalidOperationException(std::string(name) + ": the last frame ran on the library's own BVH, which does not produce the reference "
                                            "tree's traversal counters; construct the Renderer with TraversalCounters::Literal (or raise gpuOwnBvhThreshold)");
        return (int64_t)stats_[i];
    }
    bool Literal() const {                                 // do the model's primary rays walk the reference tree (and produce its counters)?
        if (model_ && model_->argb.empty()) return true;   // an empty model: nothing to build a BVH from
        if (gpuTraversalCounters == TraversalCounters::Literal) return true;
        if (gpuTraversalCounters == TraversalCounters::Off) return false;
        return !model_ || (int64_t)model_->argb.size() < (int64_t)gpuOwnBvhThreshold;
    }
    int Mode() const {
        if (gpuTraceMode >= 0) return gpuTraceMode;
        if (!rayTraceSubdivision) return SR_MODE_BRUTE;
        return Literal() ? SR_MODE_REF_TREE : SR_MODE_BVH;
    }
    bool PinModel() {                                      // Renderer.cs:791-810
        if (!modelVolatile_) return false;
        if (modelVolatile_->LoadingComplete) { modelVolatile_->LoadingComplete = false; model_ = modelVolatile_; return true; }
        return model_ != nullptr;
    }
    void RaytraceGeometry(Instance& instance) {            // Renderer.cs:1501-1687
        PreCalculate();
        std::vector<sr_prim> prims = ExtraGeometryToRaytrace.ToPrims();
        sr_check(sr_set_extra_geometry(scene_, prims.data(), (int32_t)prims.size()));
        rayTraceStartRow = std::min(std::max(0, rayTraceStartRow), height_ - 1);   // :1652-1653
        rayTraceEndRow = std::min(std::max(0, rayTraceEndRow), height_ - 1);
        sr_frame f = BuildFrame(instance);
        if (!pixels_) throw InvalidOperationException("SetRenderingSurface must be called before Render");
        if (f.trace_mode != SR_MODE_BVH || rayTraceVoxels) {   // the literal tree, brute force or the voxel grid: the reference's counters
            sr_check(sr_render(scene_, &f, pixels_, stats_));
            haveCounters_ = true;
        } else {                                           // the own BVH does not produce them: reading one throws
            sr_check(sr_render(scene_, &f, pixels_, nullptr));
            const int rows = std::max(0, rayTraceEndRow - rayTraceStartRow + 1);
            stats_[0] = (uint64_t)rows * (uint64_t)width_ * (uint64_t)(rayTraceSubPixelRes * rayTraceSubPixelRes);   // NumRaysFired, :1916
            stats_[1] = stats_[2] = stats_[3] = 0;
            haveCounters_ = false;
        }
    }

    sr_scene* scene_ = nullptr;
    uint32_t backgroundColor_ = 0;
    bool lightFieldHasTris_ = true;                        // Renderer.cs:446
    bool lightFieldTris_ = false;                          // LightFieldTriangles(): the library's triangle light field may run
    double fieldOfViewDepth_ = 0;
    int width_ = 1, height_ = 1;
    int32_t* pixels_ = nullptr;
    int antiAliasResolution_ = 1;                          // Renderer.cs:155-156
    int aaWidth_ = 0, aaHeight_ = 0;
    int32_t* aaPixels_ = nullptr;                          // antiAliasedSurface: the caller's buffer while AA > 1
    std::vector<int32_t> hires_;
    std::shared_ptr<Engine3D::Model> modelVolatile_, model_;
    const Engine3D::Model* sceneModel_ = nullptr;
    uint32_t built_ = 0;
    uint64_t stats_[4] = {0, 0, 0, 0};
    bool haveCounters_ = true;                             // before the first frame the reference reads zeros
};

}  // namespace Engine3D
