// overlap_triangles_tests.cpp -- Renderer::OverlapTriangles() of the C++ host mirror softray_amd/host/Engine3D.hpp (sr_overlap_triangles) on
// three copies of the right triangle a = (0, 0, z), b = (1, 0, z), c = (0, 1, z) at z = 0, -2 and 0 again (TriangleIndex 0, 1 and 2: 0 and 2
// are the same triangle), where every answer is known and exact in binary: a needle through two of them, a triangle that pierces one and is
// pierced by it, a miss, a NaN, the triangle itself (never reported), a touch in one vertex, three crossings in a row of two; the counting
// call, SR_OVERLAP_ANY, the indices alone, and the reference tree's refusal.
// usage: overlap_triangles_tests        exit 0 = every answer as stated; 3 = no HIP device
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
        const double nan = std::numeric_limits<double>::quiet_NaN();
        constexpr int K = 2;
        struct Case { double t[9]; uint32_t count; int32_t index[K]; uint8_t mask[K]; };
        const std::vector<Case> cases = {
            {{0.25, 0.25, -1, 0.25, 0.25, 1, 0.25, 0.25, 1}, 2, {0, 2}, {5, 5}},       // a needle (two equal vertices) through the twins: its edges 0 and 2
            {{0.25, 0.25, -3, 0.25, 0.25, -1, 5, 5, -1}, 1, {1, -1}, {17, 0}},         // its edge 0 pierces the copy at -2, whose edge 1 pierces it
            {{10, 10, 10, 11, 10, 10, 10, 11, 12}, 0, {-1, -1}, {0, 0}},
            {{nan, 0.25, -1, 0.25, 0.25, 1, 0.5, 0.25, 1}, 0, {-1, -1}, {0, 0}},       // a NaN: nothing is reported
            {{0, 0, 0, 1, 0, 0, 0, 1, 0}, 0, {-1, -1}, {0, 0}},                        // the triangle itself: neither it nor its copy
            {{0, 0, 0, -1, -1, 1, -1, -1, -1}, 2, {0, 2}, {45, 45}},                   // a touch in the vertex a: the four edges that end there
            {{0.25, 0.25, -3, 0.25, 0.25, 1, 0.5, 0.125, 1}, 3, {0, 1}, {5, 5}},       // three crossings, a row of two: the lowest indices
        };
        const int64_t n = (int64_t)cases.size();
        std::vector<double> q;
        for (const Case& c : cases) q.insert(q.end(), c.t, c.t + 9);
        int bad = 0;
        const char* names[2] = {"brute force", "own BVH"};
        for (int m = 0; m < 2; ++m) {
            renderer.rayTraceSubdivision = m != 0;
            renderer.gpuTraceMode = m == 1 ? SR_MODE_BVH : -1;
            std::vector<uint32_t> count(n, 7u);
            std::vector<int32_t> index((size_t)n * K, 7);
            std::vector<uint8_t> mask((size_t)n * K, 7);
            renderer.OverlapTriangles(n, q.data(), K, count.data(), index.data(), mask.data());
            bool count_ok = true, index_ok = true, mask_ok = true;
            for (int64_t i = 0; i < n; ++i) {
                const Case& c = cases[i];
                count_ok = count_ok && count[i] == c.count;
                for (int s = 0; s < K; ++s) {
                    index_ok = index_ok && index[(size_t)i * K + s] == c.index[s];
                    mask_ok = mask_ok && mask[(size_t)i * K + s] == c.mask[s];
                }
            }
            bad += Report((std::string("counts, ") + names[m]).c_str(), count_ok);
            bad += Report((std::string("indices, ") + names[m]).c_str(), index_ok);
            bad += Report((std::string("masks, ") + names[m]).c_str(), mask_ok);
            // the indices alone under the promise of order: the same rows; the masks alone; the counting call; SR_OVERLAP_ANY
            std::vector<int32_t> index2((size_t)n * K, 7);
            renderer.OverlapTriangles(n, q.data(), K, nullptr, index2.data(), nullptr, true);
            bad += Report((std::string("the indices alone, ") + names[m]).c_str(), index2 == index);
            std::vector<uint8_t> mask2((size_t)n * K, 7);
            renderer.OverlapTriangles(n, q.data(), K, nullptr, nullptr, mask2.data());
            bad += Report((std::string("the masks alone, ") + names[m]).c_str(), mask2 == mask);
            std::vector<uint32_t> count2(n, 7u);
            renderer.OverlapTriangles(n, q.data(), 0, count2.data(), nullptr, nullptr);
            bad += Report((std::string("the counting call, ") + names[m]).c_str(), count2 == count);
            std::vector<uint32_t> any(n, 7u);
            renderer.OverlapTriangles(n, q.data(), 0, any.data(), nullptr, nullptr, false, true);
            bool any_ok = true;
            for (int64_t i = 0; i < n; ++i) any_ok = any_ok && any[i] == (count[i] > 0 ? 1u : 0u);
            bad += Report((std::string("SR_OVERLAP_ANY, ") + names[m]).c_str(), any_ok);
        }
        // SR_OVERLAP_ANY keeps no rows; the reference tree has no overlap query
        bool refused = false;
        try {
            std::vector<int32_t> index((size_t)n * K, 7);
            renderer.OverlapTriangles(n, q.data(), K, nullptr, index.data(), nullptr, false, true);
        } catch (const std::exception& ex) {
            refused = std::strstr(ex.what(), "max_hits must be 0") != nullptr;
        }
        bad += Report("SR_OVERLAP_ANY with rows is refused", refused);
        renderer.rayTraceSubdivision = true;
        renderer.gpuTraceMode = -1;
        refused = false;
        try {
            uint32_t c1 = 0;
            renderer.OverlapTriangles(1, q.data(), 0, &c1, nullptr, nullptr);
        } catch (const std::exception& ex) {
            refused = std::strstr(ex.what(), "SR_MODE_REF_TREE") != nullptr;
        }
        bad += Report("the reference tree is refused", refused);
        renderer.rayTraceSubdivision = false;
        renderer.OverlapTriangles(0, nullptr, K, nullptr, nullptr, nullptr);                                      // an empty batch is legal
        std::printf(bad ? "FAILED (%d)\n" : "ALL OK\n", bad);
        return bad ? 1 : 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 3;
    }
}
