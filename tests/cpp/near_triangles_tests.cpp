// near_triangles_tests.cpp -- Renderer::NearTriangles() of the C++ host mirror softray_amd/host/Engine3D.hpp (sr_near_triangles) on three
// copies of the right triangle a = (0, 0, z), b = (1, 0, z), c = (0, 1, z) at z = 0, -2 and 0 again (TriangleIndex 0, 1 and 2: 0 and 2 are
// the same triangle, a tie that the index breaks), where every answer is known and exact in binary: counts under limits that keep and cut,
// rows ordered by (squared distance, index) and padded, slot 0 against Renderer::ClosestPoints(), the K-nearest form, the counting call, and
// the reference tree's refusal.
// usage: near_triangles_tests        exit 0 = every answer as stated; 3 = no HIP device
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
        for (double z : {0.0, -2.0, 0.0}) {
            const double t[9] = {0.0, 0.0, z, 1.0, 0.0, z, 0.0, 1.0, z};
            mesh->v9.insert(mesh->v9.end(), t, t + 9);
            mesh->argb.push_back(0xFF40C080u);
        }
        mesh->Min = Vector(-2.0, -2.0, -3.0); mesh->Max = Vector(2.0, 2.0, 2.0);
        Renderer renderer(0);
        renderer.Model(mesh);
        renderer.rayTrace = true;
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        constexpr int K = 2;
        // the point (0.25, 0.25, z) lies above the face of every copy: the distances are |z - copy's z|
        struct Case { double q[3], limit; uint32_t count; int32_t index[K]; double dist[K]; };
        const std::vector<Case> cases = {
            {{0.25, 0.25, 0.5}, inf, 3, {0, 2}, {0.5, 0.5}},                      // the twin triangles tie: index order; the copy at -2 is third
            {{0.25, 0.25, -1.5}, inf, 3, {1, 0}, {0.5, 1.5}},
            {{0.25, 0.25, 0.5}, 0.5, 2, {0, 2}, {0.5, 0.5}},                      // the limit is the distance: kept
            {{0.25, 0.25, 0.5}, 0.4375, 0, {-1, -1}, {0.0, 0.0}},                 // ... below it: cut
            {{0.25, 0.25, -1.5}, 1.0, 1, {1, -1}, {0.5, 0.0}},                    // one of three within reach: the row is padded
            {{0.25, 0.25, 0.5}, nan, 0, {-1, -1}, {0.0, 0.0}},
            {{0.25, 0.25, 0.5}, -1.0, 0, {-1, -1}, {0.0, 0.0}},
            {{nan, 0.25, 0.5}, inf, 0, {-1, -1}, {0.0, 0.0}},                     // a NaN point
        };
        const int64_t n = (int64_t)cases.size();
        std::vector<double> q, lim;
        for (const Case& c : cases) { q.insert(q.end(), c.q, c.q + 3); lim.push_back(c.limit); }
        int bad = 0;
        const char* names[2] = {"brute force", "own BVH"};
        for (int m = 0; m < 2; ++m) {
            renderer.rayTraceSubdivision = m != 0;
            renderer.gpuTraceMode = m == 1 ? SR_MODE_BVH : -1;
            std::vector<uint32_t> count(n, 7u);
            std::vector<int32_t> index((size_t)n * K, 7);
            std::vector<double> dist((size_t)n * K, 7.0), pos((size_t)n * K * 3, 7.0), uv((size_t)n * K * 2, 7.0);
            renderer.NearTriangles(n, q.data(), lim.data(), K, count.data(), index.data(), dist.data(), pos.data(), uv.data());
            bool count_ok = true, index_ok = true, dist_ok = true, pos_ok = true;
            for (int64_t i = 0; i < n; ++i) {
                const Case& c = cases[i];
                count_ok = count_ok && count[i] == c.count;
                for (int s = 0; s < K; ++s) {
                    const size_t at = (size_t)i * K + s;
                    index_ok = index_ok && index[at] == c.index[s];
                    dist_ok = dist_ok && dist[at] == c.dist[s] && !std::signbit(dist[at]);
                    const bool kept = c.index[s] >= 0;
                    const double z = kept ? (c.index[s] == 1 ? -2.0 : 0.0) : 0.0, xy = kept ? 0.25 : 0.0;
                    const double want_pos[3] = {xy, xy, z}, want_uv[2] = {xy, xy};
                    pos_ok = pos_ok && std::memcmp(&pos[at * 3], want_pos, sizeof want_pos) == 0 && std::memcmp(&uv[at * 2], want_uv, sizeof want_uv) == 0;
                }
            }
            bad += Report((std::string("counts, ") + names[m]).c_str(), count_ok);
            bad += Report((std::string("indices, ") + names[m]).c_str(), index_ok);
            bad += Report((std::string("distances, ") + names[m]).c_str(), dist_ok);
            bad += Report((std::string("points and weights, ") + names[m]).c_str(), pos_ok);
            // the K-nearest form and the promise of order: the same rows; the counting call: the same counts
            std::vector<int32_t> index2((size_t)n * K, 7);
            renderer.NearTriangles(n, q.data(), lim.data(), K, nullptr, index2.data(), nullptr, nullptr, nullptr, true);
            bad += Report((std::string("the indices alone, ") + names[m]).c_str(), index2 == index);
            std::vector<uint32_t> count2(n, 7u);
            renderer.NearTriangles(n, q.data(), lim.data(), 0, count2.data(), nullptr, nullptr, nullptr, nullptr);
            bad += Report((std::string("the counting call, ") + names[m]).c_str(), count2 == count);
            // slot 0 is ClosestPoints' answer
            std::vector<int32_t> tri(n, 7);
            std::vector<double> cdist(n, 7.0);
            renderer.ClosestPoints(n, q.data(), lim.data(), tri.data(), cdist.data(), nullptr, nullptr);
            bool slot0 = true;
            for (int64_t i = 0; i < n; ++i) slot0 = slot0 && tri[i] == index[(size_t)i * K] && std::memcmp(&cdist[i], &dist[(size_t)i * K], 8) == 0;
            bad += Report((std::string("slot 0 is the closest point, ") + names[m]).c_str(), slot0);
        }
        // the reference tree has no distance query
        renderer.rayTraceSubdivision = true;
        renderer.gpuTraceMode = -1;
        bool refused = false;
        try {
            uint32_t c1 = 0;
            renderer.NearTriangles(1, q.data(), nullptr, 0, &c1, nullptr, nullptr, nullptr, nullptr);
        } catch (const std::exception& ex) {
            refused = std::strstr(ex.what(), "SR_MODE_REF_TREE") != nullptr;
        }
        bad += Report("the reference tree is refused", refused);
        renderer.rayTraceSubdivision = false;
        renderer.NearTriangles(0, nullptr, nullptr, K, nullptr, nullptr, nullptr, nullptr, nullptr);              // an empty batch is legal
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 3;
    }
}
