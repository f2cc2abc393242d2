// nearest_rays_tests.cpp -- Renderer::NearestRays() of the C++ host mirror softray_amd/host/Engine3D.hpp (sr_nearest_rays): the nearest hit
// within a distance on a model of one triangle in the plane z = 0.001 (TriangleTests.cs:368-393's), where every answer is known:
//   a segment through the triangle hits it from exactly one side (triangles are one-sided), at about half its length; with a limit of 0.6
//   or none it keeps the hit (triangle 0, the triangle's colour, the crossing point), with 0.25 it loses it; a segment that stops short of
//   the plane hits with the limit 2.0 and not with 1.0; a segment beside the triangle never hits; a NaN limit and a negative one give a
//   miss, +inf any hit; a miss is hit 0, zeros and tri_index -1; end points (dirs - starts) and plain directions give the same answers,
//   and OccludedRays() the same hit bytes.
// usage: nearest_rays_tests        exit 0 = every answer as stated; 3 = no HIP device
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../softray_amd/host/Engine3D.hpp"

using namespace Engine3D;

struct Answers {
    std::vector<uint8_t> hit;
    std::vector<double> frac, pos, nrm;
    std::vector<uint32_t> color;
    std::vector<int32_t> tri;
    explicit Answers(size_t n) : hit(n, 9), frac(n, -7.0), pos(3 * n, -7.0), nrm(3 * n, -7.0), color(n, 0x12345678u), tri(n, 77) {}
};

static int Check(const char* what, bool ok) {
    std::printf("%-40s%s", what, ok ? "  ok\n" : "  <-- FAILED\n");
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
        // which side sees the front: a segment through (-0.2, 0.2), inside the outline, both ways
        const double through[2][6] = {{-0.2, 0.2, 0.4, -0.2, 0.2, -0.4}, {-0.2, 0.2, -0.4, -0.2, 0.2, 0.4}};
        std::vector<double> starts, ends;
        for (int k = 0; k < 2; ++k) { starts.insert(starts.end(), through[k], through[k] + 3); ends.insert(ends.end(), through[k] + 3, through[k] + 6); }
        Answers side(2);
        renderer.NearestRays(2, starts.data(), ends.data(), nullptr, side.hit.data(), nullptr, nullptr, nullptr, nullptr, nullptr, true);
        if (side.hit[0] + side.hit[1] != 1) { std::printf("FAILED (the triangle is hit from %d sides)\n", side.hit[0] + side.hit[1]); return 1; }
        const double zf = side.hit[0] ? 0.4 : -0.4;              // the z of the side that sees the triangle's front
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
        // without limits every ray that meets the front hits
        const std::vector<uint8_t> want_free = {1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0};
        const auto known = [&](const Answers& a, const std::vector<uint8_t>& w) {
            bool ok = a.hit == w;
            for (int64_t i = 0; i < n && ok; ++i) {
                if (w[i]) {
                    // the crossing: z = 0.001 on the segment from zf towards its end
                    const double f = (0.001 - s[3 * i + 2]) / d[3 * i + 2];
                    ok = std::fabs(a.frac[i] - f) < 1e-12 && a.tri[i] == 0 && a.color[i] == 0xFF40C080u && std::fabs(a.pos[3 * i] + 0.2) < 1e-12 &&
                         std::fabs(a.pos[3 * i + 1] - 0.2) < 1e-12 && std::fabs(a.pos[3 * i + 2] - 0.001) < 1e-12 &&
                         std::fabs(std::fabs(a.nrm[3 * i + 2]) - 1.0) < 1e-12;
                } else {
                    ok = a.frac[i] == 0.0 && a.tri[i] == -1 && a.color[i] == 0u;
                    for (int k = 0; k < 3 && ok; ++k) ok = a.pos[3 * i + k] == 0.0 && a.nrm[3 * i + k] == 0.0;
                }
            }
            return ok;
        };
        const char* names[3] = {"brute force", "reference tree", "own BVH"};
        for (int m = 0; m < 3; ++m) {
            renderer.rayTraceSubdivision = m != 0;
            renderer.gpuTraceMode = m == 2 ? SR_MODE_BVH : -1;
            Answers a(n), b(n), c(n);
            renderer.NearestRays(n, s.data(), e.data(), lim.data(), a.hit.data(), a.frac.data(), a.pos.data(), a.nrm.data(), a.color.data(), a.tri.data(), true);
            renderer.NearestRays(n, s.data(), d.data(), lim.data(), b.hit.data(), b.frac.data(), b.pos.data(), b.nrm.data(), b.color.data(), b.tri.data(), false, true);
            renderer.NearestRays(n, s.data(), e.data(), nullptr, c.hit.data(), c.frac.data(), c.pos.data(), c.nrm.data(), c.color.data(), c.tri.data(), true);
            std::vector<uint8_t> occ(n, 9);
            renderer.OccludedRays(n, s.data(), e.data(), lim.data(), occ.data(), true);
            bad += Check((std::string("end points, ") + names[m]).c_str(), known(a, want));
            bad += Check((std::string("directions, ") + names[m]).c_str(), known(b, want));
            bad += Check((std::string("no limits, ") + names[m]).c_str(), known(c, want_free));
            bad += Check((std::string("OccludedRays agrees, ") + names[m]).c_str(), occ == a.hit);
        }
        renderer.NearestRays(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);      // an empty batch is legal
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 3;
    }
}
