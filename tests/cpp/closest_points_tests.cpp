// closest_points_tests.cpp -- Renderer::ClosestPoints() of the C++ host mirror softray_amd/host/Engine3D.hpp (sr_closest_points) on the right
// triangle a = (0, 0, 0), b = (1, 0, 0), c = (0, 1, 0) and a copy of it at z = -2 (TriangleIndex 0 and 1), where every answer is known: one
// point for each of the seven regions, half a unit above the plane (distance = sqrt(in-plane distance^2 + 1/4), all exact in binary), a
// point midway between the two triangles (a tie: the lower index), limits that keep and cut, a NaN point, and the reference tree's refusal.
// usage: closest_points_tests        exit 0 = every answer as stated; 3 = no HIP device
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
        auto mesh = std::make_shared<Model>();
        for (double z : {0.0, -2.0}) {
            const double t[9] = {0.0, 0.0, z, 1.0, 0.0, z, 0.0, 1.0, z};
            mesh->v9.insert(mesh->v9.end(), t, t + 9);
            mesh->argb.push_back(0xFF40C080u);
        }
        mesh->Min = Vector(-2.0, -2.0, -2.0); mesh->Max = Vector(2.0, 2.0, 2.0);
        Renderer renderer(0);
        renderer.Model(mesh);
        renderer.rayTrace = true;
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        struct Case { double q[3], limit; int32_t tri; double d2, pos[3], uv[2]; };
        const std::vector<Case> cases = {
            {{-1.0, -1.0, 0.5}, inf, 0, 2.25, {0.0, 0.0, 0.0}, {0.0, 0.0}},        // vertex a
            {{2.0, -0.5, 0.5}, inf, 0, 1.5, {1.0, 0.0, 0.0}, {1.0, 0.0}},          // vertex b
            {{-0.5, 2.0, 0.5}, inf, 0, 1.5, {0.0, 1.0, 0.0}, {0.0, 1.0}},          // vertex c
            {{0.25, -1.0, 0.5}, inf, 0, 1.25, {0.25, 0.0, 0.0}, {0.25, 0.0}},      // edge ab
            {{-1.0, 0.75, 0.5}, inf, 0, 1.25, {0.0, 0.75, 0.0}, {0.0, 0.75}},      // edge ac
            {{1.0, 1.0, 0.5}, inf, 0, 0.75, {0.5, 0.5, 0.0}, {0.5, 0.5}},          // edge bc
            {{0.25, 0.25, 0.5}, inf, 0, 0.25, {0.25, 0.25, 0.0}, {0.25, 0.25}},    // the face
            {{0.25, 0.25, -1.0}, inf, 0, 1.0, {0.25, 0.25, 0.0}, {0.25, 0.25}},    // midway between the two: the lower index
            {{0.25, 0.25, -1.5}, inf, 1, 0.25, {0.25, 0.25, -2.0}, {0.25, 0.25}},  // nearer to the copy
            {{0.25, 0.25, 0.5}, 0.5, 0, 0.25, {0.25, 0.25, 0.0}, {0.25, 0.25}},    // the limit is the distance: kept
            {{0.25, 0.25, 0.5}, 0.4375, -1, 0.0, {0.0, 0.0, 0.0}, {0.0, 0.0}},     // ... below it: cut
            {{0.25, 0.25, 0.5}, nan, -1, 0.0, {0.0, 0.0, 0.0}, {0.0, 0.0}},
            {{0.25, 0.25, 0.5}, -1.0, -1, 0.0, {0.0, 0.0, 0.0}, {0.0, 0.0}},
            {{nan, 0.25, 0.5}, inf, -1, 0.0, {0.0, 0.0, 0.0}, {0.0, 0.0}},         // a NaN point
        };
        const int64_t n = (int64_t)cases.size();
        std::vector<double> q, lim;
        for (const Case& c : cases) { q.insert(q.end(), c.q, c.q + 3); lim.push_back(c.limit); }
        int bad = 0;
        const char* names[2] = {"brute force", "own BVH"};
        for (int m = 0; m < 2; ++m) {
            renderer.rayTraceSubdivision = m != 0;
            renderer.gpuTraceMode = m == 1 ? SR_MODE_BVH : -1;
            std::vector<int32_t> tri(n, 7);
            std::vector<double> dist(n, 7.0), pos((size_t)n * 3, 7.0), uv((size_t)n * 2, 7.0);
            renderer.ClosestPoints(n, q.data(), lim.data(), tri.data(), dist.data(), pos.data(), uv.data());
            bool tri_ok = true, dist_ok = true, pos_ok = true, uv_ok = true;
            for (int64_t i = 0; i < n; ++i) {
                const Case& c = cases[i];
                tri_ok = tri_ok && tri[i] == c.tri;
                dist_ok = dist_ok && dist[i] == std::sqrt(c.d2) && !std::signbit(dist[i]);
                pos_ok = pos_ok && std::memcmp(&pos[3 * i], c.pos, sizeof c.pos) == 0;
                uv_ok = uv_ok && std::memcmp(&uv[2 * i], c.uv, sizeof c.uv) == 0;
            }
            bad += Report((std::string("triangles, ") + names[m]).c_str(), tri_ok);
            bad += Report((std::string("distances, ") + names[m]).c_str(), dist_ok);
            bad += Report((std::string("points, ") + names[m]).c_str(), pos_ok);
            bad += Report((std::string("weights, ") + names[m]).c_str(), uv_ok);
            std::vector<int32_t> tri2(n, 7);
            renderer.ClosestPoints(n, q.data(), lim.data(), tri2.data(), nullptr, nullptr, nullptr, true);       // one output, the promise of order
            bad += Report((std::string("the triangles alone, ") + names[m]).c_str(), tri2 == tri);
        }
        // the reference tree has no distance query
        renderer.rayTraceSubdivision = true;
        renderer.gpuTraceMode = -1;
        bool refused = false;
        try {
            int32_t t1 = 0;
            renderer.ClosestPoints(1, q.data(), nullptr, &t1, nullptr, nullptr, nullptr);
        } catch (const std::exception& ex) {
            refused = std::strstr(ex.what(), "SR_MODE_REF_TREE") != nullptr;
        }
        bad += Report("the reference tree is refused", refused);
        renderer.rayTraceSubdivision = false;
        renderer.ClosestPoints(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);                          // an empty batch is legal
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 3;
    }
}
