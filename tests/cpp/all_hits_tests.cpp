// all_hits_tests.cpp -- Renderer::AllHitRays() of the C++ host mirror softray_amd/host/Engine3D.hpp (sr_all_hits_rays): every hit along a ray,
// nearest first, with a count, on a stack of five parallel triangles at z = -0.2 .. 0.2 of which the middle one is there twice (six
// triangles, TriangleIndex 2 and 3 are the duplicates), where every answer is known:
//   a segment through the stack from the front crosses all six, in the order of their planes, the duplicates at the same rayFrac with the
//   lower index first; from behind it crosses none (triangles are one-sided); a limit cuts the list and the count; the count is not capped by
//   max_hits and the unused slots of a row are -1 / 0.0; max_hits = 0 counts; without `count` the rows are the same; the reference tree is
//   refused.
// usage: all_hits_tests        exit 0 = every answer as stated; 3 = no HIP device
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../softray_amd/host/Engine3D.hpp"

using namespace Engine3D;

static int Report(const char* what, bool ok) {
    std::printf("%-44s%s", what, ok ? "  ok\n" : "  <-- FAILED\n");
    return ok ? 0 : 1;
}

int main() {
    try {
        const double zs[6] = {-0.2, -0.1, 0.0, 0.0, 0.1, 0.2};
        auto stack = std::make_shared<Model>();
        for (double z : zs) {
            const double t[9] = {-0.5, -0.5, z, 0.5, 0.5, z, -0.5, 0.5, z};
            stack->v9.insert(stack->v9.end(), t, t + 9);
            stack->argb.push_back(0xFF40C080u);
        }
        stack->Min = Vector(-0.5, -0.5, -0.5); stack->Max = Vector(0.5, 0.5, 0.5);
        Renderer renderer(0);
        renderer.Model(stack);
        renderer.rayTrace = true;
        renderer.rayTraceSubdivision = false;
        int bad = 0;
        // which side sees the fronts: a segment through (-0.2, 0.2), inside the outline, both ways
        const double s2[6] = {-0.2, 0.2, 0.4, -0.2, 0.2, -0.4}, e2[6] = {-0.2, 0.2, -0.4, -0.2, 0.2, 0.4};
        uint32_t side[2] = {9, 9};
        renderer.AllHitRays(2, s2, e2, nullptr, 0, side, nullptr, nullptr, true);
        if (!((side[0] == 6 && side[1] == 0) || (side[0] == 0 && side[1] == 6))) {
            std::printf("FAILED (the stack is crossed %u and %u times)\n", side[0], side[1]);
            return 1;
        }
        const double zf = side[0] ? 0.4 : -0.4;
        std::printf("the fronts are seen from z = %+.1f\n", zf);
        // the order a ray from the front meets the triangles in, and its rayFrac at each (a segment from z = zf to z = -zf)
        std::vector<int32_t> order = zf > 0 ? std::vector<int32_t>{5, 4, 2, 3, 1, 0} : std::vector<int32_t>{0, 1, 2, 3, 4, 5};
        std::vector<double> frac;
        for (int32_t j : order) frac.push_back((zf - zs[j]) / (2.0 * zf));
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        struct Ray { double s[3], e[3], limit; uint32_t want; };
        const std::vector<Ray> rays = {
            {{-0.2, 0.2, zf}, {-0.2, 0.2, -zf}, inf, 6},           // through the stack
            {{-0.2, 0.2, zf}, {-0.2, 0.2, -zf}, 1.0, 6},
            {{-0.2, 0.2, zf}, {-0.2, 0.2, -zf}, 0.45, 2},          // the limit lies between the second plane and the duplicates
            {{-0.2, 0.2, zf}, {-0.2, 0.2, -zf}, 0.55, 4},          // ... behind the duplicates: both count
            {{-0.2, 0.2, zf}, {-0.2, 0.2, 0.0}, 1.1, 4},           // a segment that ends in the middle, and a tenth beyond it
            {{0.2, -0.2, zf}, {0.2, -0.2, -zf}, inf, 0},           // beside the triangles
            {{-0.2, 0.2, -zf}, {-0.2, 0.2, zf}, inf, 0},           // from behind
            {{-0.2, 0.2, zf}, {-0.2, 0.2, -zf}, nan, 0},
            {{-0.2, 0.2, zf}, {-0.2, 0.2, -zf}, -1.0, 0},
            {{-0.2, 0.2, zf}, {-0.2, 0.2, zf}, 1.0, 0},            // a segment of length zero
        };
        const int64_t n = (int64_t)rays.size();
        std::vector<double> s, e, d, lim;
        for (const Ray& r : rays) {
            for (int k = 0; k < 3; ++k) { s.push_back(r.s[k]); e.push_back(r.e[k]); d.push_back(r.e[k] - r.s[k]); }
            lim.push_back(r.limit);
        }
        const char* names[2] = {"brute force", "own BVH"};
        for (int m = 0; m < 2; ++m) {
            renderer.rayTraceSubdivision = m != 0;
            renderer.gpuTraceMode = m == 1 ? SR_MODE_BVH : -1;
            for (int K : {4, 64}) {
                std::vector<uint32_t> count(n, 99);
                std::vector<int32_t> index((size_t)n * K, 7), index2((size_t)n * K, 7);
                std::vector<double> rf((size_t)n * K, 7.0), rf2((size_t)n * K, 7.0);
                renderer.AllHitRays(n, s.data(), e.data(), lim.data(), K, count.data(), index.data(), rf.data(), true);
                renderer.AllHitRays(n, s.data(), d.data(), lim.data(), K, nullptr, index2.data(), rf2.data(), false, true);   // directions, no count
                bool counts_ok = true, rows_ok = true;
                for (int64_t i = 0; i < n; ++i) {
                    counts_ok = counts_ok && count[i] == rays[i].want;
                    const double scale = i == 4 ? 2.0 : 1.0;       // (the short segment: the same crossings at twice the rayFrac)
                    for (int q = 0; q < K; ++q) {
                        const bool used = q < (int)rays[i].want;
                        const int32_t wi = used ? order[q] : -1;
                        const double wf = used ? frac[q] * scale : 0.0;
                        const double gf = rf[(size_t)i * K + q];
                        rows_ok = rows_ok && index[(size_t)i * K + q] == wi && (used ? std::fabs(gf - wf) < 1e-12 : (gf == 0.0 && !std::signbit(gf)));
                    }
                    if (rays[i].want >= 4) rows_ok = rows_ok && rf[(size_t)i * K + 2] == rf[(size_t)i * K + 3];      // the duplicates tie exactly
                }
                const bool same = index == index2 && std::memcmp(rf.data(), rf2.data(), rf.size() * sizeof(double)) == 0;
                bad += Report((std::string("counts, ") + names[m] + ", K = " + std::to_string(K)).c_str(), counts_ok);
                bad += Report((std::string("rows, ") + names[m] + ", K = " + std::to_string(K)).c_str(), rows_ok);
                bad += Report((std::string("no count: same rows, ") + names[m] + ", K = " + std::to_string(K)).c_str(), same);
            }
            std::vector<uint32_t> count(n, 99);
            renderer.AllHitRays(n, s.data(), e.data(), lim.data(), 0, count.data(), nullptr, nullptr, true);                  // the counting call
            bool ok = true;
            for (int64_t i = 0; i < n; ++i) ok = ok && count[i] == rays[i].want;
            bad += Report((std::string("max_hits = 0 counts, ") + names[m]).c_str(), ok);
        }
        // the literal reference tree has no notion of all hits
        renderer.rayTraceSubdivision = true;
        renderer.gpuTraceMode = -1;
        bool refused = false;
        try {
            uint32_t c1 = 0;
            renderer.AllHitRays(1, s.data(), e.data(), nullptr, 0, &c1, nullptr, nullptr, true);
        } catch (const std::exception& ex) {
            refused = std::strstr(ex.what(), "SR_MODE_REF_TREE") != nullptr;
        }
        bad += Report("the reference tree is refused", refused);
        renderer.rayTraceSubdivision = false;
        renderer.AllHitRays(0, nullptr, nullptr, nullptr, 8, nullptr, nullptr, nullptr);      // an empty batch is legal
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 3;
    }
}
