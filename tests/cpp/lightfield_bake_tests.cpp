// lightfield_bake_tests.cpp -- Renderer::BakeLightField() of the C++ host mirror softray_amd/host/Engine3D.hpp: the whole colour light field
// pre-computed with the frame Render() would build, then two of the reference's goldens (RendererTests.cs:234-241) rendered from it.
// usage: lightfield_bake_tests <golden-dir>     exit 0 = every scenario has 0 differing RGB pixels and every count is right; 3 = no HIP device
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../softray_amd/host/Engine3D.hpp"

using namespace Engine3D;

static const double kPi = 3.14159265358979323846;
static const int kRes = 100;
static std::vector<int32_t> pixels(kRes* kRes);

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

// RendererTests.RaytraceScenario(lightField: true, lightFieldWithTris: false, ...) (RendererTests.cs:381-459): obj.3ds at depth 1
static void Setup(Renderer& renderer, const std::string& dir, bool shading, int subPixelRes) {
    renderer.BackgroundColor(0xff00ff);
    renderer.SetRenderingSurface(kRes, kRes, pixels.data());
    std::ifstream stream(dir + "/obj.3ds", std::ios::binary);
    if (!stream) throw std::runtime_error("cannot open obj.3ds");
    renderer.Load3dsModelFromStream(stream);
    auto inst = std::make_shared<Instance>(renderer.Model());
    inst->Position = Vector(0.0, 0.0, 1.0);
    inst->Yaw = 135.0 / 180.0 * kPi; inst->Pitch = -22.0 / 180.0 * kPi; inst->Roll = 0.0;
    renderer.Instances.push_back(inst);
    renderer.rayTrace = true;
    renderer.rayTraceSubdivision = true;
    renderer.rayTraceShading = shading;
    renderer.rayTraceFocalBlur = false;
    renderer.rayTraceSubPixelRes = subPixelRes;
    renderer.rayTraceLightField = true;
}

static int Compare(const std::string& dir, const std::string& name) {
    int w = 0, h = 0; std::vector<uint32_t> base;
    if (!ReadBmpRgb(dir + "/raytrace/100x100/" + name + ".bmp", w, h, base) || w != kRes || h != kRes) { std::printf("%-40s MISSING BASELINE\n", name.c_str()); return 1; }
    int diff = 0;
    for (int i = 0; i < w * h; ++i) if (((uint32_t)pixels[i] & 0x00FFFFFFu) != base[i]) ++diff;
    std::printf("%-40s diff=%d%s\n", name.c_str(), diff, diff ? "  <-- FAILED" : "");
    return diff ? 1 : 0;
}

// bake the whole table, render the golden from it, and bake again: nothing may be left to fill
static int Scenario(const std::string& dir, bool shading, int subPixelRes, const std::string& golden) {
    int bad = 0;
    Renderer renderer(0);
    Setup(renderer, dir, shading, subPixelRes);
    try { renderer.BakeLightField(); ++bad; std::printf("expected a refusal with LightFieldStoresTriangles = true\n"); }
    catch (const std::logic_error& e) {
        if (std::string(e.what()).find("LightFieldStoresTriangles = true") == std::string::npos) { ++bad; std::printf("refusal does not name the switch: %s\n", e.what()); }
    }
    renderer.LightFieldStoresTriangles(false);
    const uint64_t n = (uint64_t)renderer.LightFieldResolution(), total = 4 * n * n * n * n;
    const uint64_t filled = renderer.BakeLightField();
    if (filled != total) { ++bad; std::printf("BakeLightField filled %llu of %llu entries\n", (unsigned long long)filled, (unsigned long long)total); }
    renderer.Render();
    bad += Compare(dir, golden);
    if (renderer.NumRaysFired() != (int64_t)kRes * kRes * subPixelRes * subPixelRes) { ++bad; std::printf("NumRaysFired must count the camera samples\n"); }
    const uint64_t again = renderer.BakeLightField();
    if (again != 0) { ++bad; std::printf("a second bake filled %llu entries\n", (unsigned long long)again); }
    else std::printf("second bake fills 0 ok\n");
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <golden-dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    try {
        int bad = 0;
        bad += Scenario(dir, false, 1, "noShading_lightFieldColor");
        bad += Scenario(dir, true, 4, "shading_lightFieldColor_4xAA");
        {
            Renderer renderer(0);
            Setup(renderer, dir, true, 1);
            renderer.LightFieldStoresTriangles(false);
            renderer.rayTraceShadows = true;
            try { renderer.BakeLightField(); ++bad; std::printf("expected a refusal with rayTraceShadows\n"); }
            catch (const std::logic_error& e) {
                if (std::string(e.what()).find("rayTraceLightField together with rayTraceShadows") == std::string::npos) { ++bad; std::printf("refusal does not name the pair: %s\n", e.what()); }
                else std::printf("rayTraceLightField together with rayTraceShadows refused ok\n");
            }
        }
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
}
