// voxel_tests.cpp -- the reference's voxel-grid golden tests (RendererTests.cs:285-306: RaytraceVoxelGrid,
// RaytraceVoxelGridWithOtherObject) through the C++ host mirror softray_amd/host/Engine3D.hpp with rayTraceVoxels = true.
// usage: voxel_tests <golden-dir>        exit 0 = every scenario has 0 differing RGB pixels; 3 = no HIP device
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

// RendererTests.RaytraceScenario(voxels: true, ...) (RendererTests.cs:381-459)
static int VoxelScenario(const std::string& dir, const std::string& model, double objectDepth, double yawDeg, double pitchDeg, bool shading,
                         const std::string& name, bool shadows = false, bool otherObject = false) {
    const int resolution = 100;
    Renderer renderer(0);
    renderer.BackgroundColor(0xff00ff);
    renderer.SetRenderingSurface(resolution, resolution, pixels.data());
    std::ifstream stream(dir + "/" + model, std::ios::binary);
    if (!stream) throw std::runtime_error("cannot open " + model);
    renderer.Load3dsModelFromStream(stream);
    auto inst = std::make_shared<Instance>(renderer.Model());
    inst->Position = Vector(0.0, 0.0, objectDepth);
    inst->Yaw = yawDeg / 180.0 * kPi; inst->Pitch = pitchDeg / 180.0 * kPi; inst->Roll = 0.0;
    renderer.Instances.push_back(inst);
    renderer.rayTrace = true;
    renderer.rayTraceSubdivision = true;
    renderer.rayTraceShading = shading;
    renderer.rayTraceVoxels = true;
    renderer.rayTraceShadows = shadows;
    if (otherObject) {                                      // extra geometry is ignored by a voxel frame (RendererTests.cs:308)
        Raytrace::Sphere red(Vector(-0.5, 0, -0.5), 0.5);
        red.Color = Color::Red();
        renderer.ExtraGeometryToRaytrace.Add(red);
    }
    renderer.Render();
    int w = 0, h = 0; std::vector<uint32_t> base;
    if (!ReadBmpRgb(dir + "/raytrace/100x100/" + name + ".bmp", w, h, base) || w != resolution || h != resolution) { std::printf("%-32s MISSING BASELINE\n", name.c_str()); return 1; }
    int diff = 0;
    for (int i = 0; i < w * h; ++i) if (((uint32_t)pixels[i] & 0x00FFFFFFu) != base[i] || ((uint32_t)pixels[i] >> 24) != 0xFFu) ++diff;
    // every camera ray counts once in NumRaysFired and once in NumGeometryTests (VoxelGrid.NumRayTests == 1); no nodes, no leaves
    const int64_t rays = (int64_t)resolution * resolution;
    const bool stats_ok = renderer.NumRaysFired() == rays && renderer.NumGeometryTests() == rays && renderer.NumNodeVisits() == 0 && renderer.NumLeafNodeVisits() == 0;
    std::printf("%-32s diff=%d rays=%lld%s\n", name.c_str(), diff, (long long)renderer.NumRaysFired(), (diff || !stats_ok) ? "  <-- FAILED" : "");
    return (diff || !stats_ok) ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <golden-dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    try {
        int bad = 0;
        bad += VoxelScenario(dir, "obj.3ds", 4.0, 135.0, -22.0, true, "voxels_shading");                       // RaytraceVoxelGrid
        bad += VoxelScenario(dir, "obj2.3DS", 3.0, 170.0, 0.0, false, "voxels_noShading");                     // RaytraceVoxelGridWithOtherObject
        bad += VoxelScenario(dir, "obj.3ds", 4.0, 135.0, -22.0, true, "voxels_shading", false, true);          // ... extra geometry changes nothing
        // voxels together with shadows are refused, naming the combination
        try { VoxelScenario(dir, "obj.3ds", 4.0, 135.0, -22.0, true, "voxels_shading", true); ++bad; std::printf("expected a refusal of voxels + shadows\n"); }
        catch (const std::logic_error& e) {
            if (std::string(e.what()).find("rayTraceVoxels together with rayTraceShadows") == std::string::npos) ++bad;
            else std::printf("voxels + shadows refused ok\n");
        }
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
}
