// ao_tests.cpp -- ambient occlusion (rayTraceAmbientOcclusion, SR_F_AMBIENT_OCCLUSION) through the C++ host mirror
// softray_amd/host/Engine3D.hpp.  The reference has no golden for it (RendererTests.cs:402-405 switches AO off), so the expected frames
// come from the CPU model (tests/ao_model.py): the caller writes them to a file of 2 x 100 x 100 ARGB words -- the uncached frame, then
// the first cached frame -- of obj2.3DS in the RendererTests pose.
// usage: ao_tests <golden-dir> <expected-file>        exit 0 = 0 differing pixels and every refused pair refused by name; 3 = no HIP device
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

static void Setup(Renderer& renderer, const std::string& dir) {
    renderer.BackgroundColor(0xff00ff);
    renderer.SetRenderingSurface(kRes, kRes, pixels.data());
    std::ifstream stream(dir + "/obj2.3DS", std::ios::binary);
    if (!stream) throw std::runtime_error("cannot open obj2.3DS");
    renderer.Load3dsModelFromStream(stream);
    auto inst = std::make_shared<Instance>(renderer.Model());
    inst->Position = Vector(0.0, 0.0, 1.0);
    inst->Yaw = 135.0 / 180.0 * kPi; inst->Pitch = -22.0 / 180.0 * kPi; inst->Roll = 0.0;
    renderer.Instances.push_back(inst);
    renderer.rayTrace = true;
    renderer.rayTraceSubdivision = true;
    renderer.rayTraceShading = true;
    renderer.rayTraceFocalBlur = false;
    renderer.rayTraceAmbientOcclusion = true;
}

static int Compare(const char* name, const uint32_t* want) {
    int diff = 0;
    for (int i = 0; i < kRes * kRes; ++i) if ((uint32_t)pixels[i] != want[i]) ++diff;
    std::printf("%-24s diff=%d%s\n", name, diff, diff ? "  <-- FAILED" : "");
    return diff ? 1 : 0;
}

template <class F>
static int Refused(const std::string& dir, const char* other, F set) {
    Renderer renderer(0);
    Setup(renderer, dir);
    set(renderer);
    try { renderer.Render(); }
    catch (const std::logic_error& e) {
        const std::string want = std::string("rayTraceAmbientOcclusion together with ") + other;
        if (std::string(e.what()).find(want) != std::string::npos) { std::printf("%s refused ok\n", want.c_str()); return 0; }
        std::printf("refusal does not name the pair: %s\n", e.what());
        return 1;
    }
    std::printf("expected a refusal of rayTraceAmbientOcclusion + %s\n", other);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s <golden-dir> <expected-file>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    try {
        std::vector<uint32_t> want(2 * kRes * kRes);
        {
            std::ifstream f(argv[2], std::ios::binary);
            if (!f.read(reinterpret_cast<char*>(want.data()), (std::streamsize)(want.size() * 4))) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
        }
        int bad = 0;
        {
            Renderer renderer(0);
            Setup(renderer, dir);
            renderer.ambientOcclusionEnableCache = false;
            renderer.Render();
            bad += Compare("ao_uncached", want.data());
            if (renderer.NumRaysFired() != (int64_t)kRes * kRes) { ++bad; std::printf("NumRaysFired counts the probes\n"); }   // Num* count primary rays
            // the same renderer with the cache on: cold, warm (same pixels), and cold again after the reset
            renderer.ambientOcclusionEnableCache = true;
            renderer.Render();
            bad += Compare("ao_cached", want.data() + kRes * kRes);
            renderer.Render();
            bad += Compare("ao_cached_warm", want.data() + kRes * kRes);
            renderer.ResetAmbientOcclusionCache();
            renderer.Render();
            bad += Compare("ao_cached_after_reset", want.data() + kRes * kRes);
        }
        bad += Refused(dir, "rayTracePathTracing", [](Renderer& r) { r.rayTracePathTracing = true; });
        bad += Refused(dir, "rayTraceVoxels", [](Renderer& r) { r.rayTraceVoxels = true; });
        bad += Refused(dir, "rayTraceShadowsStatic", [](Renderer& r) { r.rayTraceShadows = true; r.rayTraceShadowsStatic = true; });
        bad += Refused(dir, "gpuMaxBounces", [](Renderer& r) { r.gpuMaxBounces = 1; });
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
}
