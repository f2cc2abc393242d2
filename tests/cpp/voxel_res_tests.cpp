// voxel_res_tests.cpp -- voxel grids of another size than the reference's constant 64 through the C++ host mirror
// softray_amd/host/Engine3D.hpp: Renderer::VoxelGridSize(n) (a library extension, sr_set_voxel_res) with rayTraceVoxels = true.
//   1. the reference's single-triangle grid (TriangleTests.cs:368-393) at 32^3;
//   2. obj.3ds at 98^3.
// Both 64 x 48, depth 3, the goldens' pose, shading on.  The expected pixels are the CRC-32 of the frames tests/voxel_model_n.py renders
// (little-endian ARGB, row-major); tests/test_gpu_voxel_res.py checks the constants below against the model.
// usage: voxel_res_tests <golden-dir>        exit 0 = both frames have the model's CRC; 3 = no HIP device
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../softray_amd/host/Engine3D.hpp"

using namespace Engine3D;

static const uint32_t kCrcKat32 = 0xebb7e226u;
static const uint32_t kCrcObj98 = 0x87aadbe0u;

static const double kPi = 3.14159265358979323846;
static const int kWidth = 64, kHeight = 48;
static std::vector<int32_t> pixels(kWidth * kHeight);

static uint32_t Crc32(const void* data, size_t n) {
    const unsigned char* p = (const unsigned char*)data;
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

static int Scenario(const char* name, std::shared_ptr<Model> model, const std::string& file, int gridSize, uint32_t want) {
    Renderer renderer(0);
    renderer.BackgroundColor(0xff00ff);
    renderer.SetRenderingSurface(kWidth, kHeight, pixels.data());
    if (model) renderer.Model(model);
    else {
        std::ifstream stream(file, std::ios::binary);
        if (!stream) throw std::runtime_error("cannot open " + file);
        renderer.Load3dsModelFromStream(stream);
    }
    auto inst = std::make_shared<Instance>(renderer.Model());
    inst->Position = Vector(0.0, 0.0, 3.0);
    inst->Yaw = 135.0 / 180.0 * kPi; inst->Pitch = -22.0 / 180.0 * kPi; inst->Roll = 0.0;
    renderer.Instances.push_back(inst);
    renderer.rayTrace = true;
    renderer.rayTraceShading = true;
    renderer.rayTraceVoxels = true;
    int bad = 0;
    if (renderer.VoxelGridSize() != 64) { std::printf("%-8s the default grid size is %d, not 64\n", name, renderer.VoxelGridSize()); ++bad; }
    renderer.VoxelGridSize(gridSize);
    if (renderer.VoxelGridSize() != gridSize) ++bad;
    std::fill(pixels.begin(), pixels.end(), 0);
    renderer.Render();
    const uint32_t got = Crc32(pixels.data(), pixels.size() * sizeof(int32_t));
    const int64_t rays = (int64_t)kWidth * kHeight;
    const bool stats_ok = renderer.NumRaysFired() == rays && renderer.NumGeometryTests() == rays && renderer.NumNodeVisits() == 0 && renderer.NumLeafNodeVisits() == 0;
    if (got != want || !stats_ok) ++bad;
    std::printf("%-8s grid %d crc %08x want %08x rays %lld%s\n", name, gridSize, got, want, (long long)renderer.NumRaysFired(), bad ? "  <-- FAILED" : "  crc ok");
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <golden-dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    try {
        int bad = 0;
        auto kat = std::make_shared<Model>();                  // one triangle at z = 0.001: 32 * 32 filled cells at 32^3
        kat->v9 = {-0.5, -0.5, 0.001, 0.5, 0.5, 0.001, -0.5, 0.5, 0.001};
        kat->argb = {0xFF40C080u};
        kat->Min = Vector(-0.5, -0.5, -0.5); kat->Max = Vector(0.5, 0.5, 0.5);
        bad += Scenario("kat32", kat, "", 32, kCrcKat32);
        bad += Scenario("obj98", nullptr, dir + "/obj.3ds", 98, kCrcObj98);
        {                                                       // outside 1..256: the library refuses, the size stays
            Renderer renderer(0);
            try { renderer.VoxelGridSize(257); ++bad; std::printf("expected a refusal of grid size 257\n"); }
            catch (const std::exception& e) {
                if (std::string(e.what()).find("1..256") == std::string::npos || renderer.VoxelGridSize() != 64) ++bad;
                else std::printf("range refused ok\n");
            }
        }
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
}
