// occluded_rays_tests.cpp -- Renderer::OccludedRays() of the C++ host mirror softray_amd/host/Engine3D.hpp (sr_occluded_rays): "is anything in
// the way before distance L" on a model of one triangle in the plane z = 0.001 (TriangleTests.cs:368-393's), where every answer is known:
//   a segment through the triangle is blocked from exactly one side (triangles are one-sided); from that side it is blocked with the
//   default limit 1.0 and with 0.6, not with 0.25 (the crossing is at about half its length); a segment that stops short of the plane is not
//   blocked with 1.0 and is with 2.0; a segment beside the triangle never is; a NaN limit and a negative one give 0, +inf gives "any hit";
//   end points (dirs - starts) and plain directions give the same bytes.
// usage: occluded_rays_tests        exit 0 = every answer as stated; 3 = no HIP device
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../softray_amd/host/Engine3D.hpp"

using namespace Engine3D;

static int Check(const char* what, const std::vector<uint8_t>& got, const std::vector<uint8_t>& want) {
    const bool ok = got == want;
    std::printf("%-34s", what);
    for (uint8_t b : got) std::printf(" %d", (int)b);
    std::printf(ok ? "  ok\n" : "  <-- FAILED\n");
    return ok ? 0 : 1;
}

int main() {
    try {
        auto kat = std::make_shared<Model>();
        kat->v9 = {-0.5, -0.5, 0.001, 0.5, 0.5, 0.001, -0.5, 0.5, 0.001};
        kat->argb = {0xFF40C080u};
        kat->Min = Vector(-0.5, -0.5, -0.5); kat->Max = Vector(0.5, 0.5, 0.5);
        Renderer renderer(0);
        renderer.Model(kat);
        renderer.rayTrace = true;
        int bad = 0;
        // which side blocks: a segment through (-0.2, 0.2), inside the outline, both ways
        const double through[2][6] = {{-0.2, 0.2, 0.4, -0.2, 0.2, -0.4}, {-0.2, 0.2, -0.4, -0.2, 0.2, 0.4}};
        std::vector<double> starts, ends;
        for (int k = 0; k < 2; ++k) { starts.insert(starts.end(), through[k], through[k] + 3); ends.insert(ends.end(), through[k] + 3, through[k] + 6); }
        std::vector<uint8_t> side(2, 9);
        renderer.OccludedRays(2, starts.data(), ends.data(), nullptr, side.data(), true);
        if (side[0] + side[1] != 1) { Check("one side blocks", side, {1, 0}); std::printf("FAILED (the triangle blocks from %d sides)\n", side[0] + side[1]); return 1; }
        const double zf = side[0] ? 0.4 : -0.4;                  // the z of the side that sees the triangle's front
        std::printf("the front is seen from z = %+.1f\n", zf);
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        struct Ray { double s[3], e[3], limit; uint8_t want; };
        const std::vector<Ray> rays = {
            {{-0.2, 0.2, zf}, {-0.2, 0.2, -zf}, 1.0, 1},           // through the triangle
            {{-0.2, 0.2, zf}, {-0.2, 0.2, -zf}, 0.6, 1},
            {{-0.2, 0.2, zf}, {-0.2, 0.2, -zf}, 0.25, 0},          // the crossing lies beyond the limit
            {{-0.2, 0.2, zf}, {-0.2, 0.2, 0.25 * zf}, 1.0, 0},     // stops short of the plane
            {{-0.2, 0.2, zf}, {-0.2, 0.2, 0.25 * zf}, 2.0, 1},     // ... twice as far it does not
            {{0.2, -0.2, zf}, {0.2, -0.2, -zf}, 1.0, 0},           // beside the triangle
            {{0.2, -0.2, zf}, {0.2, -0.2, -zf}, inf, 0},
            {{-0.2, 0.2, zf}, {-0.2, 0.2, -zf}, nan, 0},
            {{-0.2, 0.2, zf}, {-0.2, 0.2, -zf}, -1.0, 0},
            {{-0.2, 0.2, zf}, {-0.2, 0.2, 0.25 * zf}, inf, 1},     // any hit
            {{-0.2, 0.2, -zf}, {-0.2, 0.2, zf}, inf, 0},           // from behind: never
            {{-0.2, 0.2, zf}, {-0.2, 0.2, zf}, 1.0, 0},            // a segment of length zero
        };
        const int64_t n = (int64_t)rays.size();
        std::vector<double> s, e, d, lim;
        std::vector<uint8_t> want;
        for (const Ray& r : rays) {
            for (int k = 0; k < 3; ++k) { s.push_back(r.s[k]); e.push_back(r.e[k]); d.push_back(r.e[k] - r.s[k]); }
            lim.push_back(r.limit);
            want.push_back(r.want);
        }
        // with no limits every ray has the limit 1.0
        const std::vector<uint8_t> want1 = {1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0};
        const char* names[3] = {"brute force", "reference tree", "own BVH"};
        for (int m = 0; m < 3; ++m) {
            renderer.rayTraceSubdivision = m != 0;
            renderer.gpuTraceMode = m == 2 ? SR_MODE_BVH : -1;
            std::vector<uint8_t> a(n, 9), b(n, 9), c(n, 9);
            renderer.OccludedRays(n, s.data(), e.data(), lim.data(), a.data(), true);
            renderer.OccludedRays(n, s.data(), d.data(), lim.data(), b.data(), false, true);
            renderer.OccludedRays(n, s.data(), e.data(), nullptr, c.data(), true);
            bad += Check((std::string("end points, ") + names[m]).c_str(), a, want);
            bad += Check((std::string("directions, ") + names[m]).c_str(), b, want);
            bad += Check((std::string("no limits, ") + names[m]).c_str(), c, want1);
        }
        renderer.OccludedRays(0, nullptr, nullptr, nullptr, nullptr);      // an empty batch is legal
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 3;
    }
}
