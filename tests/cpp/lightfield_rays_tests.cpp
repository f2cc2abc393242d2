// lightfield_rays_tests.cpp -- Renderer::LightFieldRays() of the C++ host mirror softray_amd/host/Engine3D.hpp (sr_light_field_rays): the colour
// light field for lines of the caller's, on a model of one triangle in the plane z = 0.001 (TriangleTests.cs:368-393's) with shading off, where
// every answer is known:
//   a line that misses the sphere of radius 0.866 gets the background and inside = 0, and fills nothing;
//   every other colour is the triangle's or the background's, and lines through the middle of the triangle from its front see the triangle;
//   a cold call and the same call on the warm table give the same colours, the second fills nothing;
//   a batch split in two equals the whole, colours and fill counts;
//   LightFieldStoresTriangles = true (the mirror's default) is refused by the library, by name.
// usage: lightfield_rays_tests        exit 0 = every answer as stated; 3 = no HIP device
#include <cstdio>
#include <string>
#include <vector>

#include "../../softray_amd/host/Engine3D.hpp"

using namespace Engine3D;

static int Check(const char* what, bool ok) {
    std::printf("%-58s%s\n", what, ok ? "  ok" : "  <-- FAILED");
    return ok ? 0 : 1;
}

int main() {
    try {
        const uint32_t kTriangle = 0xFF40C080u, kBackground = 0xFF123456u;
        auto kat = std::make_shared<Model>();
        kat->v9 = {-0.5, -0.5, 0.001, 0.5, 0.5, 0.001, -0.5, 0.5, 0.001};
        kat->argb = {kTriangle};
        kat->Min = Vector(-0.5, -0.5, -0.5); kat->Max = Vector(0.5, 0.5, 0.5);
        Renderer renderer(0);
        static std::vector<int32_t> pixels(16 * 16);
        renderer.BackgroundColor(kBackground & 0xFFFFFFu);
        renderer.SetRenderingSurface(16, 16, pixels.data());
        renderer.Model(kat);
        auto inst = std::make_shared<Instance>(renderer.Model());
        inst->Position = Vector(0.0, 0.0, 1.0);
        renderer.Instances.push_back(inst);
        renderer.rayTrace = true;
        renderer.rayTraceShading = false;
        renderer.rayTraceLightField = true;
        renderer.LightFieldResolution(8);
        int bad = 0;
        // a fan of lines: from points on two rings at z = +-0.8 through points of a 5 x 5 grid inside the triangle's outline and beside it
        std::vector<double> starts, dirs;
        for (int side = 0; side < 2; ++side)
            for (int i = 0; i < 5; ++i)
                for (int j = 0; j < 5; ++j) {
                    const double z = side ? -0.8 : 0.8;
                    const double sx = 0.1 * (i - 2), sy = 0.07 * (j - 2), tx = -0.45 + 0.2 * i + 0.013, ty = -0.45 + 0.2 * j + 0.017;
                    const double s[3] = {sx, sy, z}, d[3] = {tx - sx, ty - sy, -z};
                    starts.insert(starts.end(), s, s + 3); dirs.insert(dirs.end(), d, d + 3);
                }
        const int64_t through = (int64_t)starts.size() / 3;
        // ... and lines that pass the sphere by
        for (int i = 0; i < 6; ++i) {
            const double s[3] = {2.0 + 0.1 * i, -3.0, 0.3}, d[3] = {0.0, 1.0, 0.01 * i};
            starts.insert(starts.end(), s, s + 3); dirs.insert(dirs.end(), d, d + 3);
        }
        const int64_t n = (int64_t)starts.size() / 3;
        std::vector<uint32_t> cold(n, 7u), warm(n, 7u), parts(n, 7u);
        std::vector<uint8_t> inside(n, 9), inside2(n, 9);
        try {
            renderer.LightFieldRays(n, starts.data(), dirs.data(), cold.data(), inside.data());
            bad += Check("LightFieldStoresTriangles = true is refused", false);
        } catch (const std::exception& e) {
            bad += Check("LightFieldStoresTriangles = true is refused, by name", std::string(e.what()).find("sr_set_light_field_triangles") != std::string::npos);
        }
        renderer.LightFieldStoresTriangles(false);
        const uint64_t filled = renderer.LightFieldRays(n, starts.data(), dirs.data(), cold.data(), inside.data());
        bool miss_ok = true, colours_ok = true, inside_ok = true;
        int triangle = 0, background = 0;
        for (int64_t i = 0; i < n; ++i) {
            if (i >= through) { miss_ok = miss_ok && cold[i] == kBackground && inside[i] == 0; continue; }
            inside_ok = inside_ok && inside[i] == 1;
            colours_ok = colours_ok && (cold[i] == kTriangle || cold[i] == kBackground);
            triangle += cold[i] == kTriangle; background += cold[i] == kBackground;
        }
        std::printf("%d lines see the triangle, %d the background; %llu entries filled\n", triangle, background, (unsigned long long)filled);
        bad += Check("a line that misses the sphere: background, inside 0", miss_ok);
        bad += Check("a line through the sphere: inside 1", inside_ok);
        bad += Check("every colour is the triangle's or the background's", colours_ok);
        bad += Check("both occur, and cells were filled", triangle > 0 && background > 0 && filled > 0 && filled <= (uint64_t)through);
        const uint64_t again = renderer.LightFieldRays(n, starts.data(), dirs.data(), warm.data(), inside2.data());
        bad += Check("cold equals warm, the warm call fills nothing", warm == cold && inside2 == inside && again == 0);
        renderer.ResetLightField();
        const int64_t cut = 19;
        const uint64_t fa = renderer.LightFieldRays(cut, starts.data(), dirs.data(), parts.data(), nullptr);
        const uint64_t fb = renderer.LightFieldRays(n - cut, starts.data() + 3 * cut, dirs.data() + 3 * cut, parts.data() + cut, nullptr);
        bad += Check("split equals whole", parts == cold && fa + fb == filled);
        bad += Check("an empty batch is legal", renderer.LightFieldRays(0, nullptr, nullptr, nullptr) == 0);
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 3;
    }
}
