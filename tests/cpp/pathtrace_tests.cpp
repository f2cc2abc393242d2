// pathtrace_tests.cpp -- the reference's path-tracing golden tests (RendererTests.cs:247-281: PathTracePrimitivesTest,
// PathTraceTrianglesTest) through the C++ host mirror softray_amd/host/Engine3D.hpp with rayTracePathTracing = true.
// usage: pathtrace_tests <golden-dir>        exit 0 = every scenario has 0 differing RGB pixels; 3 = no HIP device
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../softray_amd/host/Engine3D.hpp"

using namespace Engine3D;

static const double kPi = 3.14159265358979323846;
static std::vector<int32_t> pixels(100 * 100);

static bool ReadBmpRgb(const std::string& path, int& w, int& h, std::vector<uint32_t>& rgb) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::vector<unsigned char> d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (d.size() < 54 || d[0] != 'B' || d[1] != 'M') return false;
    uint32_t off; int32_t ww, hh; uint16_t bpp;
    std::memcpy(&off, &d[10], 4); std::memcpy(&ww, &d[18], 4); std::memcpy(&hh, &d[22], 4); std::memcpy(&bpp, &d[28], 2);
    if (bpp != 32 || hh <= 0) return false;
    w = ww; h = hh; rgb.resize((size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            uint32_t px; std::memcpy(&px, &d[off + 4 * ((size_t)(h - 1 - y) * w + x)], 4);
            rgb[(size_t)y * w + x] = px & 0x00FFFFFFu;
        }
    return true;
}

// RendererTests.RaytraceScenario(pathTracing: true, shading: false, ...) (RendererTests.cs:381-459)
static int PathTraceScenario(const std::string& dir, const std::string& model, double objectDepth, bool spheres, bool focalBlur, double focalDepth,
                             int subPixelRes, const std::string& name, bool shadows = false) {
    const int resolution = 100;
    Renderer renderer(0);
    renderer.BackgroundColor(0xff00ff);
    renderer.SetRenderingSurface(resolution, resolution, pixels.data());
    std::ifstream stream(dir + "/" + model, std::ios::binary);
    if (!stream) throw std::runtime_error("cannot open " + model);
    renderer.Load3dsModelFromStream(stream);
    auto inst = std::make_shared<Instance>(renderer.Model());
    inst->Position = Vector(0.0, 0.0, objectDepth);
    inst->Yaw = 135.0 / 180.0 * kPi; inst->Pitch = -22.0 / 180.0 * kPi; inst->Roll = 0.0;
    renderer.Instances.push_back(inst);
    renderer.rayTrace = true;
    renderer.rayTraceSubdivision = true;
    renderer.rayTraceShading = false;
    renderer.rayTracePathTracing = true;
    renderer.rayTraceShadows = shadows;
    renderer.rayTraceFocalBlur = focalBlur;
    renderer.rayTraceFocalDepth = focalDepth;
    renderer.rayTraceSubPixelRes = subPixelRes;
    if (spheres) {                                          // RendererTests.cs:250-257
        Raytrace::Sphere ground(Vector(0, -10000, 0), 9999.5), red(Vector(-0.5, 0, -0.5), 0.5), green(Vector(0.5, 0, 0.5), 0.5),
                         blue(Vector(0.5, 0, -0.5), 0.5), yellow(Vector(-0.5, 0, 0.5), 0.5);
        red.Color = Color::Red(); green.Color = Color::Green(); blue.Color = Color::Blue(); yellow.Color = Color::Yellow();
        for (const Raytrace::Sphere& s : {ground, red, green, blue, yellow}) renderer.ExtraGeometryToRaytrace.Add(s);
    }
    renderer.Render();
    int w = 0, h = 0; std::vector<uint32_t> base;
    if (!ReadBmpRgb(dir + "/raytrace/100x100/" + name + ".bmp", w, h, base) || w != resolution || h != resolution) { std::printf("%-48s MISSING BASELINE\n", name.c_str()); return 1; }
    int diff = 0;
    for (int i = 0; i < w * h; ++i) if (((uint32_t)pixels[i] & 0x00FFFFFFu) != base[i] || ((uint32_t)pixels[i] >> 24) != 0xFFu) ++diff;
    const bool rays_ok = renderer.NumRaysFired() == (int64_t)resolution * resolution * subPixelRes * subPixelRes;
    std::printf("%-48s diff=%d rays=%lld%s\n", name.c_str(), diff, (long long)renderer.NumRaysFired(), (diff || !rays_ok) ? "  <-- FAILED" : "");
    return (diff || !rays_ok) ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <golden-dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    try {
        int bad = 0;
        // PathTraceTrianglesTest (RendererTests.cs:268-281): obj2.3DS, depth 1, focal depth 1
        bad += PathTraceScenario(dir, "obj2.3DS", 1.0, false, false, 1.5, 1, "pathTracing_noShading");
        bad += PathTraceScenario(dir, "obj2.3DS", 1.0, false, false, 1.5, 2, "pathTracing_noShading_2xAA");
        bad += PathTraceScenario(dir, "obj2.3DS", 1.0, false, false, 1.5, 4, "pathTracing_noShading_4xAA");
        bad += PathTraceScenario(dir, "obj2.3DS", 1.0, false, false, 1.5, 8, "pathTracing_noShading_8xAA");
        bad += PathTraceScenario(dir, "obj2.3DS", 1.0, false, true, 1.0, 2, "pathTracing_noShading_focalBlurx2");
        bad += PathTraceScenario(dir, "obj2.3DS", 1.0, false, true, 1.0, 4, "pathTracing_noShading_focalBlurx4");
        bad += PathTraceScenario(dir, "obj2.3DS", 1.0, false, true, 1.0, 8, "pathTracing_noShading_focalBlurx8");
        // PathTracePrimitivesTest (:247-266): obj.3ds at depth 3 with the five spheres, focal depth 2.5
        bad += PathTraceScenario(dir, "obj.3ds", 3.0, true, false, 3.5, 1, "pathTracing_noShading_6_geometry");
        bad += PathTraceScenario(dir, "obj.3ds", 3.0, true, true, 2.5, 4, "pathTracing_noShading_focalBlurx4_7_geometry");
        bad += PathTraceScenario(dir, "obj.3ds", 3.0, true, true, 2.5, 8, "pathTracing_noShading_focalBlurx8_8_geometry");
        // path tracing together with shadows is refused, naming the combination
        try { PathTraceScenario(dir, "obj2.3DS", 1.0, false, false, 1.5, 1, "pathTracing_noShading", true); ++bad; std::printf("expected a refusal of path tracing + shadows\n"); }
        catch (const std::logic_error& e) {
            if (std::string(e.what()).find("rayTracePathTracing together with rayTraceShadows") == std::string::npos) ++bad;
            else std::printf("path tracing + shadows refused ok\n");
        }
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
}
