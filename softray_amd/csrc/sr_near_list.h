// sr_near_list.h -- the list of one point of sr_near_triangles: the K nearest triangles seen so far by (d2, TriangleIndex), kept in the
// point's own ROW of memory.  One text for the kernels (sr_near.hip: rows in device memory, one lane per point) and the stand-alone host
// program tests/cpp/near_list_check.cpp (rows in host memory between guard words).  AhList's design (sr_allhits.hip): the fill
// count, the worst kept slot and the worst kept key live in the struct (registers on the device), a displacement rescans the K slots once,
// the sort runs once at the end; no array is indexed in private memory.
// Compiled with -ffp-contract=off, as sr_closest.h, whose routine gives every value kept here.
#pragma once
#include <cmath>

#include "sr_closest.h"

namespace sr {

// the order of the rows: d2 ascending, then TriangleIndex ascending.  A NaN d2 is never offered
SR_HOST_DEVICE inline bool near_precedes(double da, int32_t ja, double db, int32_t jb) { return da < db || (da == db && ja < jb); }

// The largest d2 that a limit admits: dist_j <= lim <=> fl(sqrt(d2_j)) <= lim <=> d2_j <= near_threshold(lim), since the rounded square root
// never decreases as d2 grows.  fl(lim lim) is within a few steps of it: down while the square root is beyond the limit (0 ends that:
// sqrt(0) = 0 <= lim), then up while the next double is still admitted (+inf ends that).  A NaN, negative or -inf limit admits nothing:
// -inf, which no d2 is <=.  (-0.0 is 0: it admits d2 == 0.)
SR_HOST_DEVICE inline double near_threshold(double lim) {
    if (!(lim >= 0.0)) return -(double)INFINITY;
    double t = lim * lim;
    while (sqrt(t) > lim) t = nextafter(t, -(double)INFINITY);
    for (;;) {
        const double u = nextafter(t, (double)INFINITY);
        if (u == t || !(sqrt(u) <= lim)) break;
        t = u;
    }
    return t;
}

// One point's list.  K slots per row; every slot index used below is < K: `fill` only grows while fill < K, `wslot` is either a former
// `fill` or comes out of a scan over [0, K).  The key row holds d2 until finish() replaces it by the distances.
struct NearList {
    int32_t* idx;        // the point's rows (K == 0: never dereferenced)
    double*  key;
    int      K, fill, wslot;
    double   wkey;       // the worst kept (d2, index) (valid when fill > 0)
    int32_t  widx;
    uint32_t count;      // every member of the set, kept or not

    SR_HOST_DEVICE inline void init(int32_t* idx_row, double* key_row, int k) {
        idx = idx_row; key = key_row; K = k; fill = 0; wslot = 0; wkey = 0.0; widx = 0; count = 0u;
    }
    SR_HOST_DEVICE inline bool full() const { return fill >= K; }
    // a member of the set.  Returns true when the worst kept key changed while the row is full (the caller's cull bound follows it)
    SR_HOST_DEVICE inline bool offer(double d2, int32_t j) {
        count++;
        if (K <= 0) return false;
        if (fill < K) {
            idx[fill] = j; key[fill] = d2;
            if (fill == 0 || !near_precedes(d2, j, wkey, widx)) { wkey = d2; widx = j; wslot = fill; }
            fill++;
            return fill == K;
        }
        if (!near_precedes(d2, j, wkey, widx)) return false;
        idx[wslot] = j; key[wslot] = d2;                     // displaces the worst; one rescan of the K slots finds the new worst
        int ws = 0;
        double wd = key[0];
        int32_t wj = idx[0];
        for (int s = 1; s < K; ++s) {
            const double ds = key[s];
            const int32_t js = idx[s];
            if (near_precedes(wd, wj, ds, js)) { wd = ds; wj = js; ws = s; }
        }
        wslot = ws; wkey = wd; widx = wj;
        return true;
    }
    // Sort the kept entries by (d2, index) (insertion sort, K <= 64), replace every d2 by its rounded square root, pad the rest of the row
    // (-1, 0.0); then pos_row ([K][3]) / uv_row ([K][2]), where wanted: the routine once more per kept slot on q and v9[index] -- the values
    // sr_closest_points stores for its winner -- and zeros in the other slots
    SR_HOST_DEVICE inline void finish(const double q[3], const double* v9, double* pos_row, double* uv_row) {
        for (int a = 1; a < fill; ++a) {
            const double d = key[a];
            const int32_t j = idx[a];
            int b = a - 1;
            while (b >= 0) {
                const double db = key[b];
                const int32_t jb = idx[b];
                if (!near_precedes(d, j, db, jb)) break;
                key[b + 1] = db; idx[b + 1] = jb;            // (b + 1 <= a < fill <= K)
                --b;
            }
            key[b + 1] = d; idx[b + 1] = j;
        }
        for (int s = 0; s < fill; ++s) key[s] = sqrt(key[s]);
        for (int s = fill; s < K; ++s) { idx[s] = -1; key[s] = 0.0; }
        if (!pos_row && !uv_row) return;
        for (int s = 0; s < K; ++s) {
            double c[3] = {0.0, 0.0, 0.0}, v = 0.0, w = 0.0;
            if (s < fill) closest_point_triangle(q, v9 + (size_t)idx[s] * 9, c, v, w);
            if (pos_row) { pos_row[3 * s] = c[0]; pos_row[3 * s + 1] = c[1]; pos_row[3 * s + 2] = c[2]; }
            if (uv_row) { uv_row[2 * s] = v; uv_row[2 * s + 1] = w; }
        }
    }
};

}  // namespace sr
