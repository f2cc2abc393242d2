// sr_tri_overlap.h -- do two triangles cross?  The pair predicate of sr_overlap_triangles in FP64 and the row of one query: the one text that
// the kernels (sr_overlap.hip), the stand-alone host program (tests/cpp/tri_overlap_check.cpp) and, operation for operation, the numpy
// model (tests/overlap_model.py) compute.  Compiled with -ffp-contract=off everywhere; only + - * and comparisons, every expression in the
// operand order written here.
//
// vol(a, b, c, d): with u = b - a, v = c - a, w = d - a and n = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x) the value
// (n.x w.x + n.y w.y) + n.z w.z -- six times the signed volume of the tetrahedron.  WHEN ANY TWO OF THE FOUR POINTS ARE EQUAL (== on all
// three components) vol IS EXACTLY 0: without that rule the rounding of (u x v) . u makes a triangle of a mesh "cross" its neighbours'
// shared vertices at random, and itself.
// Edge (p, q) MEETS triangle (a, b, c): sp = vol(a, b, c, p), sq = vol(a, b, c, q); no when both are > 0, both < 0, both == 0 (the edge lies
// in the plane) or either is NaN; otherwise s1 = vol(p, q, a, b), s2 = vol(p, q, b, c), s3 = vol(p, q, c, a) and the edge meets the
// triangle iff all three are >= 0 or all three are <= 0.  The test is closed (touching counts); a NaN fails every comparison.
// The MASK of the pair (query A, scene B): bit e (0..2) = edge (A[e], A[(e + 1) % 3]) meets B; bit 3 + e = edge (B[e], B[(e + 1) % 3]) meets A.
// The pair is REPORTED iff all 18 coordinates are finite, the FP64 bounding boxes of A and B overlap on every axis (closed <= on the
// coordinates as given: exact) and the mask is not 0.  The box condition never changes a true answer (two triangles that meet share a
// point); it is part of the definition so that the tree's cull is conservative by construction.
// Consequences: coplanar pairs are never reported (every edge lies in the other's plane, or on one side of it); a triangle without area
// can be pierced by nothing (two of its vertices are equal, or its normal is 0 up to rounding: every side is 0) but its edges can pierce;
// a triangle never crosses itself or an exact copy (every vol has two equal points); swapping the roles of A and B swaps the two halves
// of the mask.
// Out of scope: the intersection segment or contact points, penetration depth, coplanar overlap, excluding the neighbours in a self-query
// (the caller drops the pairs that share vertices).
#pragma once
#include "sr_types.h"

#if defined(__HIPCC__)
#define SR_OV_UNROLL _Pragma("unroll")
#else
#define SR_OV_UNROLL
#endif

namespace sr {

SR_HOST_DEVICE inline bool ov_same(const double* a, const double* b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }

// vol without the equal-points rule
SR_HOST_DEVICE inline double ov_vol_raw(const double* a, const double* b, const double* c, const double* d) {
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double wx = d[0] - a[0], wy = d[1] - a[1], wz = d[2] - a[2];
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    return nx * wx + ny * wy + nz * wz;
}
// the definition, on its own (the host check compares tri_overlap_mask with the mask made from these two)
SR_HOST_DEVICE inline double ov_vol(const double* a, const double* b, const double* c, const double* d) {
    if (ov_same(a, b) || ov_same(a, c) || ov_same(a, d) || ov_same(b, c) || ov_same(b, d) || ov_same(c, d)) return 0.0;
    return ov_vol_raw(a, b, c, d);
}
SR_HOST_DEVICE inline bool ov_sides_apart(double sp, double sq) {
    return (sp > 0.0 && sq > 0.0) || (sp < 0.0 && sq < 0.0) || (sp == 0.0 && sq == 0.0) || sp != sp || sq != sq;
}
SR_HOST_DEVICE inline bool ov_one_sign(double s1, double s2, double s3) {
    return (s1 >= 0.0 && s2 >= 0.0 && s3 >= 0.0) || (s1 <= 0.0 && s2 <= 0.0 && s3 <= 0.0);
}
SR_HOST_DEVICE inline bool ov_edge_meets(const double* p, const double* q, const double* a, const double* b, const double* c) {
    if (ov_sides_apart(ov_vol(a, b, c, p), ov_vol(a, b, c, q))) return false;
    return ov_one_sign(ov_vol(p, q, a, b), ov_vol(p, q, b, c), ov_vol(p, q, c, a));
}

SR_HOST_DEVICE inline bool ov_finite9(const double t[9]) {
    bool ok = true;
    SR_OV_UNROLL
    for (int k = 0; k < 9; ++k) ok = ok && t[k] >= -1.7976931348623157e308 && t[k] <= 1.7976931348623157e308;
    return ok;
}
SR_HOST_DEVICE inline double ov_min3(double a, double b, double c) { const double m = a < b ? a : b; return m < c ? m : c; }
SR_HOST_DEVICE inline double ov_max3(double a, double b, double c) { const double m = a > b ? a : b; return m > c ? m : c; }
// the FP64 bounding box of a triangle with finite coordinates
SR_HOST_DEVICE inline void ov_box(const double t[9], double lo[3], double hi[3]) {
    SR_OV_UNROLL
    for (int k = 0; k < 3; ++k) { lo[k] = ov_min3(t[k], t[3 + k], t[6 + k]); hi[k] = ov_max3(t[k], t[3 + k], t[6 + k]); }
}

// The three edge tests of one half of the mask: the edges of P = {P[0], P[1], P[2]} against the triangle T.  side[e] = vol(T, P[e]) is
// made once per vertex and shared by the two edges that end there; every vol is the value of the definition: the equal-points rule is
// applied through `same`, the pairs of equal points -- bit e: P[e] == P[(e + 1) % 3]; bit 3 + f: T[f] == T[(f + 1) % 3]; bit 6 + 3 e + f:
// P[e] == T[f].
SR_HOST_DEVICE inline unsigned int ov_half(const double P[9], const double T[9], unsigned int same) {
    const bool t_flat = (same & 0x38u) != 0u;
    double side[3];
    SR_OV_UNROLL
    for (int e = 0; e < 3; ++e) side[e] = (t_flat || ((same >> (6 + 3 * e)) & 7u) != 0u) ? 0.0 : ov_vol_raw(T, T + 3, T + 6, P + 3 * e);
    unsigned int bits = 0u;
    SR_OV_UNROLL
    for (int e = 0; e < 3; ++e) {
        const int e1 = e == 2 ? 0 : e + 1;
        if (ov_sides_apart(side[e], side[e1])) continue;
        const double* p = P + 3 * e;
        const double* q = P + 3 * e1;
        // vol(p, q, T[f], T[f1]) is 0 when p == q (z0), T[f] == T[f1], or p or q equals T[f] or T[f1] (touch: bit f)
        const bool z0 = (same & (1u << e)) != 0u;
        const unsigned int touch = ((same >> (6 + 3 * e)) & 7u) | ((same >> (6 + 3 * e1)) & 7u);
        const double s1 = (z0 || (same & 0x08u) || (touch & 3u)) ? 0.0 : ov_vol_raw(p, q, T, T + 3);
        const double s2 = (z0 || (same & 0x10u) || (touch & 6u)) ? 0.0 : ov_vol_raw(p, q, T + 3, T + 6);
        const double s3 = (z0 || (same & 0x20u) || (touch & 5u)) ? 0.0 : ov_vol_raw(p, q, T + 6, T);
        if (ov_one_sign(s1, s2, s3)) bits |= 1u << e;
    }
    return bits;
}

// The mask of the pair (A, B) as REPORTED: 0 unless all coordinates are finite and the boxes overlap
SR_HOST_DEVICE inline unsigned int tri_overlap_mask(const double A[9], const double B[9]) {
    if (!ov_finite9(A) || !ov_finite9(B)) return 0u;
    double alo[3], ahi[3], blo[3], bhi[3];
    ov_box(A, alo, ahi);
    ov_box(B, blo, bhi);
    SR_OV_UNROLL
    for (int k = 0; k < 3; ++k)
        if (!(alo[k] <= bhi[k] && blo[k] <= ahi[k])) return 0u;
    unsigned int same = 0u;
    SR_OV_UNROLL
    for (int e = 0; e < 3; ++e) {
        const int e1 = e == 2 ? 0 : e + 1;
        if (ov_same(A + 3 * e, A + 3 * e1)) same |= 1u << e;
        if (ov_same(B + 3 * e, B + 3 * e1)) same |= 8u << e;
        SR_OV_UNROLL
        for (int f = 0; f < 3; ++f)
            if (ov_same(A + 3 * e, B + 3 * f)) same |= 1u << (6 + 3 * e + f);
    }
    // the other half sees the transposed table: bits 0..2 and 3..5 change places, bit 6 + 3 e + f becomes 6 + 3 f + e
    unsigned int swapped = ((same & 7u) << 3) | ((same >> 3) & 7u);
    for (int e = 0; e < 3; ++e)
        for (int f = 0; f < 3; ++f)
            if (same & (1u << (6 + 3 * e + f))) swapped |= 1u << (6 + 3 * f + e);
    return ov_half(A, B, same) | (ov_half(B, A, swapped) << 3);
}

// The row of one query: the K lowest TriangleIndex among the reported triangles, offered in any order, kept in the query's own ROW of
// memory (NearList's design, sr_near_list.h: the fill count, the worst kept slot and index live in the struct -- registers on the device --
// a displacement rescans the K slots once, the sort runs once at the end; no array is indexed in private memory).  Every slot index used
// below is < K: `fill` only grows while fill < K, `wslot` is a former `fill` or comes out of a scan over [0, K).
struct OverlapList {
    int32_t* idx;        // the query's row (K == 0: never dereferenced)
    int      K, fill, wslot;
    int32_t  widx;       // the highest kept index (valid when fill > 0)
    uint32_t count;      // every reported triangle, kept or not

    SR_HOST_DEVICE inline void init(int32_t* idx_row, int k) { idx = idx_row; K = k; fill = 0; wslot = 0; widx = 0; count = 0u; }
    SR_HOST_DEVICE inline void offer(int32_t j) {
        count++;
        if (K <= 0) return;
        if (fill < K) {
            idx[fill] = j;
            if (fill == 0 || j > widx) { widx = j; wslot = fill; }
            fill++;
            return;
        }
        if (!(j < widx)) return;
        idx[wslot] = j;                                      // displaces the highest; one rescan of the K slots finds the new highest
        int ws = 0;
        int32_t wj = idx[0];
        for (int s = 1; s < K; ++s) {
            const int32_t js = idx[s];
            if (js > wj) { wj = js; ws = s; }
        }
        wslot = ws; widx = wj;
    }
    // Sort the kept indices ascending (insertion sort, K <= 64), pad the rest of the row with -1; then mask_row ([K]), where wanted: the
    // predicate once more per kept slot on A and v9[index], 0 in the other slots
    SR_HOST_DEVICE inline void finish(const double A[9], const double* v9, uint8_t* mask_row) {
        for (int a = 1; a < fill; ++a) {
            const int32_t j = idx[a];
            int b = a - 1;
            while (b >= 0) {
                const int32_t jb = idx[b];
                if (!(j < jb)) break;
                idx[b + 1] = jb;                             // (b + 1 <= a < fill <= K)
                --b;
            }
            idx[b + 1] = j;
        }
        for (int s = fill; s < K; ++s) idx[s] = -1;
        if (!mask_row) return;
        for (int s = 0; s < K; ++s) mask_row[s] = s < fill ? (uint8_t)tri_overlap_mask(A, v9 + (size_t)idx[s] * 9) : (uint8_t)0;
    }
};

}  // namespace sr
