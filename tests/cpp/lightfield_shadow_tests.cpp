// lightfield_shadow_tests.cpp -- Renderer::LightFieldShadows() of the C++ host mirror softray_amd/host/Engine3D.hpp: rayTraceLightField together
// with dynamic rayTraceShadows.  The golden of the reference's active test RaytraceLightField_Colors (RendererTests.cs:240: light field, focal
// blur, shadows, 4 x 4 samples) from an empty table and from a table baked with shadows; the refusals with the switch off and with static shadows.
// usage: lightfield_shadow_tests <golden-dir>     exit 0 = 0 differing RGB pixels and every count is right; 3 = no HIP device
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

// RendererTests.RaytraceScenario(lightField: true, lightFieldWithTris: false, shadows: true, focalBlur: true, subPixelRes: 4) (RendererTests.cs:240, 381-459)
static void Setup(Renderer& renderer, const std::string& dir) {
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
    renderer.rayTraceShading = true;
    renderer.rayTraceShadows = true;
    renderer.rayTraceFocalBlur = true;
    renderer.rayTraceSubPixelRes = 4;
    renderer.rayTraceLightField = true;
    renderer.LightFieldStoresTriangles(false);
}

static int Compare(const std::string& dir, const std::string& name, const char* what) {
    int w = 0, h = 0; std::vector<uint32_t> base;
    if (!ReadBmpRgb(dir + "/raytrace/100x100/" + name + ".bmp", w, h, base) || w != kRes || h != kRes) { std::printf("%-40s MISSING BASELINE\n", name.c_str()); return 1; }
    int diff = 0;
    for (int i = 0; i < w * h; ++i) if (((uint32_t)pixels[i] & 0x00FFFFFFu) != base[i]) ++diff;
    std::printf("%s: %s diff=%d%s\n", what, name.c_str(), diff, diff ? "  <-- FAILED" : "");
    return diff ? 1 : 0;
}

static int Refused(Renderer& renderer, bool bake, const char* what) {
    try { if (bake) renderer.BakeLightField(); else renderer.Render(); }
    catch (const std::logic_error& e) {
        if (std::string(e.what()).find("rayTraceLightField together with rayTraceShadows") != std::string::npos) { std::printf("%s refused ok\n", what); return 0; }
        std::printf("%s: the refusal does not name the pair: %s\n", what, e.what());
        return 1;
    }
    std::printf("%s: expected a refusal\n", what);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <golden-dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const std::string golden = "shading_shadows_lightFieldColor_focalBlurx4";
    try {
        int bad = 0;
        Renderer renderer(0);
        Setup(renderer, dir);
        // ---- the default: the pair is refused, by Render() and by BakeLightField() ----
        if (renderer.LightFieldShadows()) { ++bad; std::printf("LightFieldShadows must default to false\n"); }
        bad += Refused(renderer, false, "switch off, Render");
        bad += Refused(renderer, true, "switch off, BakeLightField");
        // ---- switch on: the golden from an empty table ----
        renderer.LightFieldShadows(true);
        if (!renderer.LightFieldShadows()) { ++bad; std::printf("LightFieldShadows(true) did not stick\n"); }
        renderer.Render();
        bad += Compare(dir, golden, "empty table");
        if (renderer.NumRaysFired() != (int64_t)kRes * kRes * 16) { ++bad; std::printf("NumRaysFired must count the camera samples\n"); }
        // ---- ... and from a table baked with shadows: no cell is left for the frame ----
        renderer.ResetLightField();
        const uint64_t n = (uint64_t)renderer.LightFieldResolution(), total = 4 * n * n * n * n;
        const uint64_t filled = renderer.BakeLightField();
        if (filled != total) { ++bad; std::printf("BakeLightField filled %llu of %llu entries\n", (unsigned long long)filled, (unsigned long long)total); }
        std::fill(pixels.begin(), pixels.end(), 0);
        renderer.Render();
        bad += Compare(dir, golden, "baked table");
        const uint64_t again = renderer.BakeLightField();
        if (again != 0) { ++bad; std::printf("a second bake filled %llu entries\n", (unsigned long long)again); }
        else std::printf("second bake fills 0 ok\n");
        // ---- static shadows stay refused with the switch on; the switch off refuses again ----
        renderer.rayTraceShadowsStatic = true;
        bad += Refused(renderer, false, "switch on, static shadows");
        renderer.rayTraceShadowsStatic = false;
        renderer.LightFieldShadows(false);
        bad += Refused(renderer, false, "switch off again");
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
}
