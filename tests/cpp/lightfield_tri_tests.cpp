// lightfield_tri_tests.cpp -- Renderer::LightFieldTriangles() of the C++ host mirror softray_amd/host/Engine3D.hpp: the opt-in that lets
// LightFieldStoresTriangles = true (the reference's default, LightFieldTriMethod) run on the library's triangle table
// (sr_set_light_field_triangles).  Without the opt-in Render() and BakeLightField() refuse as they always did, naming the switch.  The reference
// ignores its own test of this method, so the mirror's frame is compared with sr_render on a scene of the plain C ABI that has the switch on and
// gets the frame the mirror builds: the mirror passes the switch on, and nothing else.
// usage: lightfield_tri_tests <golden-dir>     exit 0 = every check holds; 3 = no HIP device
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../softray_amd/host/Engine3D.hpp"

using namespace Engine3D;

static const double kPi = 3.14159265358979323846;
static const int kRes = 100, kN = 8;
static std::vector<int32_t> pixels(kRes* kRes);

// RendererTests.RaytraceScenario(lightField: true, lightFieldWithTris: true) (RendererTests.cs:217-220, 381-459), at a coarse resolution so that
// all three stages work
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
    renderer.rayTraceLightField = true;
    renderer.LightFieldResolution(kN);
}

static int Differing(const std::vector<int32_t>& a, const std::vector<int32_t>& b) {
    int diff = 0;
    for (size_t i = 0; i < a.size(); ++i) if (a[i] != b[i]) ++diff;
    return diff;
}

template <class F>
static bool RefusesByName(F call) {
    try { call(); } catch (const std::logic_error& e) { return std::strstr(e.what(), "LightFieldStoresTriangles = true") != nullptr; }
    return false;
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
        const uint64_t total = 4ull * kN * kN * kN * kN;
        // ---- the default: LightFieldStoresTriangles = true is refused, by name ----
        if (!renderer.LightFieldStoresTriangles() || renderer.LightFieldTriangles()) { ++bad; std::printf("defaults: LightFieldStoresTriangles true, LightFieldTriangles false\n"); }
        if (RefusesByName([&] { renderer.Render(); })) std::printf("without the opt-in Render() names the switch ok\n");
        else { ++bad; std::printf("without the opt-in Render() must refuse LightFieldStoresTriangles = true by name\n"); }
        if (RefusesByName([&] { renderer.BakeLightField(); })) std::printf("without the opt-in BakeLightField() names the switch ok\n");
        else { ++bad; std::printf("without the opt-in BakeLightField() must refuse LightFieldStoresTriangles = true by name\n"); }
        // ---- the opt-in: the frame is the one the C ABI renders with the switch on ----
        renderer.LightFieldTriangles(true);
        std::fill(pixels.begin(), pixels.end(), 0);
        renderer.Render();
        const std::vector<int32_t> lazy = pixels;
        if (renderer.NumRaysFired() != (int64_t)kRes * kRes) { ++bad; std::printf("NumRaysFired must count the camera samples\n"); }
        sr_scene* raw = nullptr;
        sr_check(sr_create(0, &raw));
        sr_check(sr_load_3ds(raw, model.data(), model.size()));
        sr_frame f = renderer.BuildFrame(*renderer.Instances.front());
        sr_check(sr_build(raw, (1u << f.trace_mode) | (1u << SR_MODE_REF_TREE), 0, 0));
        sr_check(sr_set_light_field_res(raw, kN));
        sr_check(sr_set_light_field_triangles(raw, 1));
        std::vector<int32_t> direct(kRes * kRes, 0);
        sr_check(sr_render(raw, &f, direct.data(), nullptr));
        const int diff = Differing(lazy, direct);
        std::printf("triangle frame equals sr_render with the switch on: diff=%d%s\n", diff, diff ? "  <-- FAILED" : "");
        bad += diff ? 1 : 0;
        int background = 0;
        for (int32_t p : lazy) background += ((uint32_t)p & 0xffffffu) == 0xff00ffu;
        if (background == 0 || background == kRes * kRes) { ++bad; std::printf("the frame must show the model on the background\n"); }
        // ---- the bake ----
        renderer.ResetLightField();
        sr_check(sr_reset_light_field(raw));
        const uint64_t filled = renderer.BakeLightField();
        uint64_t filled_direct = 0;
        sr_check(sr_bake_light_field(raw, &f, 0, total, &filled_direct));
        std::vector<uint32_t> a(total), b(total);
        sr_check(sr_get_light_field_tris(raw, b.data(), 0, total));
        renderer.GetLightFieldTris(a.data(), 0, total);
        if (filled == total && filled_direct == total && a == b && a[0] != 0) std::printf("BakeLightField() equals sr_bake_light_field: filled equal, tables equal ok\n");
        else { ++bad; std::printf("BakeLightField(): filled %llu / %llu of %llu, tables %s\n", (unsigned long long)filled, (unsigned long long)filled_direct, (unsigned long long)total, a == b ? "equal" : "differ"); }
        std::fill(pixels.begin(), pixels.end(), 0);
        renderer.Render();
        if (Differing(lazy, pixels) == 0) std::printf("frame from the baked table identical ok\n");
        else { ++bad; std::printf("the frame from the baked table differs from the lazy frame\n"); }
        sr_destroy(raw);
        // ---- LightFieldStoresTriangles = false: the colour method, whatever the opt-in says ----
        renderer.LightFieldStoresTriangles(false);
        std::fill(pixels.begin(), pixels.end(), 0);
        renderer.Render();
        renderer.GetLightFieldTris(a.data(), 0, total);
        bool empty = true;
        for (uint32_t e : a) empty = empty && e == 0;       // (the change of LightFieldStoresTriangles emptied both tables, and a colour frame fills only its own)
        if (empty && Differing(lazy, pixels) > 0) std::printf("LightFieldStoresTriangles = false: the colour light field ok\n");
        else { ++bad; std::printf("LightFieldStoresTriangles = false must run the colour light field\n"); }
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
}
