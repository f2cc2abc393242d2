// tri_overlap_check.cpp -- the pair predicate and the row of softray_amd/csrc/sr_tri_overlap.h on the host: a stand-alone program (its own main,
// no library) that tests/test_overlap_model.py builds with g++ -ffp-contract=off under the address and undefined-behaviour sanitizers.
//   tri_overlap_check <query file> <out file>
// query file: int64 T, int64 n, T x 9 doubles (the scene), n x 9 doubles (the queries).
// out file: the masks of all pairs, uint8 [n][T]; then for the reported triangles of every query offered in ascending and in descending
// TriangleIndex, and for K = 1, 4 and 64: count uint32 [n], index int32 [n][K], mask uint8 [n][K].
// tri_overlap_mask (sides shared between edges, the equal-points rule through a table) must equal the mask made edge by edge from the
// definition's own functions (ov_edge_meets on ov_vol) for every pair: a difference ends the program with status 2.  Every row lies
// between guard words that are checked afterwards (status 3).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../softray_amd/csrc/sr_tri_overlap.h"

namespace {

unsigned int mask_by_definition(const double* A, const double* B) {
    if (!sr::ov_finite9(A) || !sr::ov_finite9(B)) return 0u;
    double alo[3], ahi[3], blo[3], bhi[3];
    sr::ov_box(A, alo, ahi);
    sr::ov_box(B, blo, bhi);
    for (int k = 0; k < 3; ++k)
        if (!(alo[k] <= bhi[k] && blo[k] <= ahi[k])) return 0u;
    unsigned int m = 0u;
    for (int e = 0; e < 3; ++e) {
        const int e1 = (e + 1) % 3;
        if (sr::ov_edge_meets(A + 3 * e, A + 3 * e1, B, B + 3, B + 6)) m |= 1u << e;
        if (sr::ov_edge_meets(B + 3 * e, B + 3 * e1, A, A + 3, A + 6)) m |= 8u << e;
    }
    return m;
}

constexpr int kGuard = 16;
constexpr int32_t kGuardWord = 0x5A5A5A5A;

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: tri_overlap_check <query file> <out file>\n"); return 1; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    int64_t head[2];
    if (std::fread(head, sizeof(int64_t), 2, f) != 2 || head[0] < 0 || head[1] < 0) { std::fprintf(stderr, "bad header\n"); return 1; }
    const size_t T = (size_t)head[0], n = (size_t)head[1];
    std::vector<double> v9(T * 9 + 1), q(n * 9 + 1);
    if (std::fread(v9.data(), sizeof(double), T * 9, f) != T * 9 || std::fread(q.data(), sizeof(double), n * 9, f) != n * 9) {
        std::fprintf(stderr, "short file\n");
        return 1;
    }
    std::fclose(f);
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }

    std::vector<uint8_t> all(n * T + 1);
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < T; ++j) {
            const unsigned int m = sr::tri_overlap_mask(&q[i * 9], &v9[j * 9]);
            if (m != mask_by_definition(&q[i * 9], &v9[j * 9])) {
                std::fprintf(stderr, "query %zu, triangle %zu: tri_overlap_mask %u, the definition %u\n", i, j, m, mask_by_definition(&q[i * 9], &v9[j * 9]));
                return 2;
            }
            all[i * T + j] = (uint8_t)m;
        }
    std::fwrite(all.data(), 1, n * T, out);

    const int ks[3] = {1, 4, 64};
    for (int descending = 0; descending < 2; ++descending)
        for (int kk = 0; kk < 3; ++kk) {
            const int K = ks[kk];
            std::vector<uint32_t> count(n + 1);
            std::vector<int32_t> index(n * K + 1);
            std::vector<uint8_t> mask(n * K + 1);
            std::vector<int32_t> row(kGuard + K + kGuard);
            std::vector<uint8_t> mrow(kGuard + K + kGuard);
            for (size_t i = 0; i < n; ++i) {
                for (auto& w : row) w = kGuardWord;
                for (auto& w : mrow) w = 0x5A;
                sr::OverlapList L;
                L.init(row.data() + kGuard, K);
                for (size_t s = 0; s < T; ++s) {
                    const size_t j = descending ? T - 1 - s : s;
                    if (all[i * T + j]) L.offer((int32_t)j);
                }
                L.finish(&q[i * 9], v9.data(), mrow.data() + kGuard);
                for (int g = 0; g < kGuard; ++g)
                    if (row[g] != kGuardWord || row[kGuard + K + g] != kGuardWord || mrow[g] != 0x5A || mrow[kGuard + K + g] != 0x5A) {
                        std::fprintf(stderr, "query %zu, K %d: a guard word was overwritten\n", i, K);
                        return 3;
                    }
                count[i] = L.count;
                for (int s = 0; s < K; ++s) { index[i * K + s] = row[kGuard + s]; mask[i * K + s] = mrow[kGuard + s]; }
            }
            std::fwrite(count.data(), sizeof(uint32_t), n, out);
            std::fwrite(index.data(), sizeof(int32_t), n * K, out);
            std::fwrite(mask.data(), 1, n * K, out);
        }
    std::fclose(out);
    return 0;
}
