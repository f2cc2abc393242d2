// closest_point_check.cpp -- the header routine of softray_amd/csrc/sr_closest.h on the host, for tests/test_closest_points_model.py: the
// program reads a point file (int64 T, int64 P, T x 9 doubles of triangles, P x 3 doubles of points), runs closest_point_triangle and
// closest_d2 for every (point, triangle) pair in that order and writes seven doubles per pair -- region, c.x, c.y, c.z, v, w, d2 -- to the
// output file.  No library, no device: built with g++ -ffp-contract=off (and, where asked for, with a sanitizer).
// usage: closest_point_check <point file> <output file>        exit 0 = written; 2 = usage or file error
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../softray_amd/csrc/sr_closest.h"

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: closest_point_check <point file> <output file>\n"); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int64_t head[2] = {0, 0};
    if (std::fread(head, sizeof(int64_t), 2, in) != 2 || head[0] < 0 || head[1] < 0 || head[0] > 4096 || head[1] > 4096) { std::fclose(in); return 2; }
    const size_t T = (size_t)head[0], P = (size_t)head[1];
    std::vector<double> tris(T * 9), pts(P * 3);
    const bool read_ok = std::fread(tris.data(), sizeof(double), tris.size(), in) == tris.size() &&
                         std::fread(pts.data(), sizeof(double), pts.size(), in) == pts.size();
    std::fclose(in);
    if (!read_ok) { std::fprintf(stderr, "short point file\n"); return 2; }
    std::vector<double> out(P * T * 7);
    for (size_t i = 0; i < P; ++i)
        for (size_t j = 0; j < T; ++j) {
            double c[3], v, w;
            const int region = sr::closest_point_triangle(&pts[3 * i], &tris[9 * j], c, v, w);
            double* o = &out[(i * T + j) * 7];
            o[0] = (double)region; o[1] = c[0]; o[2] = c[1]; o[3] = c[2]; o[4] = v; o[5] = w; o[6] = sr::closest_d2(&pts[3 * i], c);
        }
    std::FILE* f = std::fopen(argv[2], "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok ? 0 : 2;
}
