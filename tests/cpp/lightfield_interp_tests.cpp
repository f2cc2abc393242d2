// lightfield_interp_tests.cpp -- Renderer::LightFieldInterpolate() of the C++ host mirror softray_amd/host/Engine3D.hpp: the colour light field with
// quad-linear interpolation (LightFieldColorMethod.Interpolate; sr_set_light_field_interpolation).  The reference has no golden for it (its test
// file carries "TODO: add render with quad-filtering on color lightfield"), so the mirror's frame is compared with sr_render on a scene of the
// plain C ABI that has the switch on and gets the frame the mirror builds: the mirror passes the switch on, and nothing else.
// usage: lightfield_interp_tests <golden-dir>     exit 0 = every check holds; 3 = no HIP device
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../softray_amd/host/Engine3D.hpp"

using namespace Engine3D;

static const double kPi = 3.14159265358979323846;
static const int kRes = 100;
static std::vector<int32_t> pixels(kRes* kRes);

// RendererTests.RaytraceScenario(lightField: true, lightFieldWithTris: false, subPixelRes: 2) (RendererTests.cs:234-241, 381-459)
static void Setup(Renderer& renderer, const std::vector<unsigned char>& model) {
    renderer.BackgroundColor(0xff00ff);
    renderer.SetRenderingSurface(kRes, kRes, pixels.data());
    std::string bytes(model.begin(), model.end());
    std::istringstream stream(bytes, std::ios::binary);
    renderer.Load3dsModelFromStream(stream);
    auto inst = std::make_shared<Instance>(renderer.Model());
    inst->Position = Vector(0.0, 0.0, 1.0);
    inst->Yaw = 135.0 / 180.0 * kPi; inst->Pitch = -22.0 / 180.0 * kPi; inst->Roll = 0.0;
    renderer.Instances.push_back(inst);
    renderer.rayTrace = true;
    renderer.rayTraceSubdivision = true;
    renderer.rayTraceShading = true;
    renderer.rayTraceSubPixelRes = 2;
    renderer.rayTraceLightField = true;
    renderer.LightFieldStoresTriangles(false);
    renderer.LightFieldResolution(16);
}

static int Differing(const std::vector<int32_t>& a, const std::vector<int32_t>& b) {
    int diff = 0;
    for (size_t i = 0; i < a.size(); ++i) if (a[i] != b[i]) ++diff;
    return diff;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <golden-dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    try {
        int bad = 0;
        std::ifstream file(dir + "/obj.3ds", std::ios::binary);
        if (!file) throw std::runtime_error("cannot open obj.3ds");
        const std::vector<unsigned char> model((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
        Renderer renderer(0);
        Setup(renderer, model);
        // ---- the default: off, the nearest lookup ----
        if (renderer.LightFieldInterpolate()) { ++bad; std::printf("LightFieldInterpolate must default to false\n"); }
        else std::printf("switch defaults to off ok\n");
        renderer.Render();
        const std::vector<int32_t> nearest = pixels;
        // ---- on: another frame ----
        renderer.LightFieldInterpolate(true);
        if (!renderer.LightFieldInterpolate()) { ++bad; std::printf("LightFieldInterpolate(true) did not stick\n"); }
        renderer.ResetLightField();
        std::fill(pixels.begin(), pixels.end(), 0);
        renderer.Render();
        const std::vector<int32_t> blended = pixels;
        if (Differing(nearest, blended) > 0) std::printf("interpolated frame differs from the nearest lookup ok\n");
        else { ++bad; std::printf("the interpolated frame equals the nearest lookup\n"); }
        if (renderer.NumRaysFired() != (int64_t)kRes * kRes * 4) { ++bad; std::printf("NumRaysFired must count the camera samples\n"); }
        // ---- the same frame through the C ABI ----
        sr_scene* raw = nullptr;
        sr_check(sr_create(0, &raw));
        sr_check(sr_load_3ds(raw, model.data(), model.size()));
        sr_frame f = renderer.BuildFrame(*renderer.Instances.front());
        sr_check(sr_build(raw, 1u << f.trace_mode, 0, 0));
        sr_check(sr_set_light_field_res(raw, 16));
        sr_check(sr_set_light_field_interpolation(raw, 1));
        std::vector<int32_t> direct(kRes * kRes, 0);
        sr_check(sr_render(raw, &f, direct.data(), nullptr));
        const int diff = Differing(blended, direct);
        std::printf("interpolated frame equals sr_render with the switch on: diff=%d%s\n", diff, diff ? "  <-- FAILED" : "");
        bad += diff ? 1 : 0;
        sr_destroy(raw);
        // ---- a warm table, and the switch off again ----
        std::fill(pixels.begin(), pixels.end(), 0);
        renderer.Render();
        if (Differing(blended, pixels) == 0) std::printf("warm frame identical ok\n");
        else { ++bad; std::printf("the warm frame differs\n"); }
        renderer.LightFieldInterpolate(false);
        renderer.ResetLightField();
        std::fill(pixels.begin(), pixels.end(), 0);
        renderer.Render();
        if (Differing(nearest, pixels) == 0) std::printf("switch off: the nearest lookup again ok\n");
        else { ++bad; std::printf("switch off: the frame is not the nearest lookup\n"); }
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
}
