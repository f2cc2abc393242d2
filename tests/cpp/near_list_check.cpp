// near_list_check.cpp -- the list of sr_near_triangles (softray_amd/csrc/sr_near_list.h) on the host, for tests/test_near_triangles_model.py.
// The program reads the point file of closest_point_check.cpp (int64 T, int64 P, T x 9 doubles of triangles, P x 3 doubles of points) and a
// limits file (P doubles).  For each of two limit sets -- none, then the file's -- and each K of 1, 4 and 64 it runs, per point, what
// k_nt_loop runs: the routine for every triangle in index order, the set's test (d2 a number, d2 <= near_threshold(limit)), NearList::offer,
// NearList::finish -- with the point's four rows in host memory, each between guard words that are checked afterwards -- and once more
// with the triangles offered in descending index order, which must give the same rows.  It writes, per limit set and K: count [P] uint32,
// index [P][K] int32, dist [P][K], pos [P][K][3], uv [P][K][2] doubles.  No library, no device: built with g++ -ffp-contract=off (and a
// sanitizer).
// usage: near_list_check <point file> <limits file> <output file>     exit 0 = written; 2 = usage or file error; 3 = a guard word or the
// second order differs
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../softray_amd/csrc/sr_near_list.h"

namespace {

constexpr int kGuard = 4;                                    // guard words before and behind every row
constexpr int32_t kGuardI = 0x5A5A5A5A;
constexpr double kGuardD = -1234.5678;

template <class T>
struct Row {
    std::vector<T> mem;
    T guard;
    Row(size_t n, T g) : mem(n + 2 * kGuard, g), guard(g) {}
    T* data() { return mem.data() + kGuard; }
    size_t size() const { return mem.size() - 2 * kGuard; }
    bool intact() const {
        for (int k = 0; k < kGuard; ++k)
            if (std::memcmp(&mem[k], &guard, sizeof(T)) != 0 || std::memcmp(&mem[mem.size() - 1 - k], &guard, sizeof(T)) != 0) return false;
        return true;
    }
};

struct PointRows {
    Row<int32_t> idx; Row<double> key, pos, uv;
    uint32_t count = 0;
    explicit PointRows(int K) : idx((size_t)K, kGuardI), key((size_t)K, kGuardD), pos((size_t)K * 3, kGuardD), uv((size_t)K * 2, kGuardD) {}
    bool intact() const { return idx.intact() && key.intact() && pos.intact() && uv.intact(); }
    bool same(PointRows& o) {
        return count == o.count && std::memcmp(idx.data(), o.idx.data(), idx.size() * 4) == 0 && std::memcmp(key.data(), o.key.data(), key.size() * 8) == 0 &&
               std::memcmp(pos.data(), o.pos.data(), pos.size() * 8) == 0 && std::memcmp(uv.data(), o.uv.data(), uv.size() * 8) == 0;
    }
};

void run_point(const double* q, const std::vector<double>& tris, size_t T, bool no_lim, double lim, int K, bool descending, PointRows& r) {
    const double thr = sr::near_threshold(no_lim ? (double)INFINITY : lim);
    sr::NearList L;
    L.init(r.idx.data(), r.key.data(), K);
    for (size_t n = 0; n < T; ++n) {
        const size_t j = descending ? T - 1 - n : n;
        double c[3], v, w;
        sr::closest_point_triangle(q, &tris[9 * j], c, v, w);
        const double d2 = sr::closest_d2(q, c);
        if (d2 == d2 && (no_lim || d2 <= thr)) L.offer(d2, (int32_t)j);
    }
    L.finish(q, tris.data(), r.pos.data(), r.uv.data());
    r.count = L.count;
}

bool read_doubles(const char* path, std::vector<double>& out, size_t n) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    out.resize(n);
    const bool ok = std::fread(out.data(), sizeof(double), n, f) == n;
    std::fclose(f);
    return ok;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: near_list_check <point file> <limits file> <output file>\n"); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int64_t head[2] = {0, 0};
    if (std::fread(head, sizeof(int64_t), 2, in) != 2 || head[0] < 0 || head[1] < 0 || head[0] > 4096 || head[1] > 4096) { std::fclose(in); return 2; }
    const size_t T = (size_t)head[0], P = (size_t)head[1];
    std::vector<double> tris(T * 9), pts(P * 3), limits;
    const bool read_ok = std::fread(tris.data(), sizeof(double), tris.size(), in) == tris.size() &&
                         std::fread(pts.data(), sizeof(double), pts.size(), in) == pts.size();
    std::fclose(in);
    if (!read_ok) { std::fprintf(stderr, "short point file\n"); return 2; }
    if (!read_doubles(argv[2], limits, P)) { std::fprintf(stderr, "cannot read %zu limits from %s\n", P, argv[2]); return 2; }
    std::FILE* f = std::fopen(argv[3], "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    bool ok = true;
    const int ks[3] = {1, 4, 64};
    for (int set = 0; set < 2; ++set)
        for (int K : ks) {
            std::vector<uint32_t> count(P);
            std::vector<int32_t> index(P * K);
            std::vector<double> dist(P * K), pos(P * K * 3), uv(P * K * 2);
            for (size_t i = 0; i < P; ++i) {
                PointRows a(K), b(K);
                run_point(&pts[3 * i], tris, T, set == 0, limits[i], K, false, a);
                run_point(&pts[3 * i], tris, T, set == 0, limits[i], K, true, b);
                if (!a.intact() || !b.intact()) { std::fprintf(stderr, "guard words of point %zu, K %d\n", i, K); std::fclose(f); return 3; }
                if (!a.same(b)) { std::fprintf(stderr, "descending order differs at point %zu, K %d\n", i, K); std::fclose(f); return 3; }
                count[i] = a.count;
                std::memcpy(&index[i * K], a.idx.data(), (size_t)K * 4);
                std::memcpy(&dist[i * K], a.key.data(), (size_t)K * 8);
                std::memcpy(&pos[i * K * 3], a.pos.data(), (size_t)K * 24);
                std::memcpy(&uv[i * K * 2], a.uv.data(), (size_t)K * 16);
            }
            ok = ok && std::fwrite(count.data(), 4, count.size(), f) == count.size() && std::fwrite(index.data(), 4, index.size(), f) == index.size() &&
                 std::fwrite(dist.data(), 8, dist.size(), f) == dist.size() && std::fwrite(pos.data(), 8, pos.size(), f) == pos.size() &&
                 std::fwrite(uv.data(), 8, uv.size(), f) == uv.size();
        }
    return std::fclose(f) == 0 && ok ? 0 : 2;
}
