// sr_closest.h -- the closest point of a triangle to a point, in FP64: the one text that sr_closest_points' kernels (sr_closest.hip), the host
// test program (tests/cpp/closest_point_check.cpp) and, operation for operation, the numpy model (tests/closest_points_model.py) compute.
// Compiled with -ffp-contract=off everywhere; only + - * / and comparisons, every expression in the operand order written here.
#pragma once
#include "sr_types.h"

namespace sr {

// The Voronoi-region routine (Ericson, Real-Time Collision Detection 5.1.5) for q against the triangle t = {a, b, c} (vertices 1, 2, 3):
// three vertex regions, three edge regions, the face, tested in the order A, B, AB, C, AC, BC, face.  c_out = a + v (b - a) + w (c - a) in
// exact terms; (v, w) are the weights of vertices 2 and 3 and are exactly 0 or 1 where a region pins them, and in a vertex region c_out is
// the vertex itself, bit for bit.  `region` (optional use): 0 A, 1 B, 2 C, 3 AB, 4 AC, 5 BC, 6 face.
// A collinear triangle can divide 0 by 0: then c_out is NaN and the caller's squared distance is NaN (never an answer).
SR_HOST_DEVICE inline int closest_point_triangle(const double q[3], const double t[9], double c_out[3], double& v, double& w) {
    const double abx = t[3] - t[0], aby = t[4] - t[1], abz = t[5] - t[2];
    const double acx = t[6] - t[0], acy = t[7] - t[1], acz = t[8] - t[2];
    const double apx = q[0] - t[0], apy = q[1] - t[1], apz = q[2] - t[2];
    const double d1 = abx * apx + aby * apy + abz * apz;
    const double d2 = acx * apx + acy * apy + acz * apz;
    if (d1 <= 0.0 && d2 <= 0.0) {
        c_out[0] = t[0]; c_out[1] = t[1]; c_out[2] = t[2]; v = 0.0; w = 0.0;
        return 0;
    }
    const double bpx = q[0] - t[3], bpy = q[1] - t[4], bpz = q[2] - t[5];
    const double d3 = abx * bpx + aby * bpy + abz * bpz;
    const double d4 = acx * bpx + acy * bpy + acz * bpz;
    if (d3 >= 0.0 && d4 <= d3) {
        c_out[0] = t[3]; c_out[1] = t[4]; c_out[2] = t[5]; v = 1.0; w = 0.0;
        return 1;
    }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        v = d1 / (d1 - d3); w = 0.0;
        c_out[0] = t[0] + abx * v; c_out[1] = t[1] + aby * v; c_out[2] = t[2] + abz * v;
        return 3;
    }
    const double cpx = q[0] - t[6], cpy = q[1] - t[7], cpz = q[2] - t[8];
    const double d5 = abx * cpx + aby * cpy + abz * cpz;
    const double d6 = acx * cpx + acy * cpy + acz * cpz;
    if (d6 >= 0.0 && d5 <= d6) {
        c_out[0] = t[6]; c_out[1] = t[7]; c_out[2] = t[8]; v = 0.0; w = 1.0;
        return 2;
    }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        v = 0.0; w = d2 / (d2 - d6);
        c_out[0] = t[0] + acx * w; c_out[1] = t[1] + acy * w; c_out[2] = t[2] + acz * w;
        return 4;
    }
    const double va = d3 * d6 - d5 * d4;
    const double d43 = d4 - d3, d56 = d5 - d6;
    if (va <= 0.0 && d43 >= 0.0 && d56 >= 0.0) {
        w = d43 / (d43 + d56); v = 1.0 - w;
        c_out[0] = t[3] + (t[6] - t[3]) * w; c_out[1] = t[4] + (t[7] - t[4]) * w; c_out[2] = t[5] + (t[8] - t[5]) * w;
        return 5;
    }
    const double sum = va + vb + vc;
    v = vb / sum; w = vc / sum;
    c_out[0] = t[0] + abx * v + acx * w; c_out[1] = t[1] + aby * v + acy * w; c_out[2] = t[2] + abz * v + acz * w;
    return 6;
}

// d2 = (q - c).x^2 + (q - c).y^2 + (q - c).z^2, summed in that order
SR_HOST_DEVICE inline double closest_d2(const double q[3], const double c[3]) {
    const double dx = q[0] - c[0], dy = q[1] - c[1], dz = q[2] - c[2];
    return dx * dx + dy * dy + dz * dz;
}

// The REGULAR points of sr_closest_points (k_cp_keys): finite, and no component further from the root box's centre than 2^20 box diagonals
// (and 2^60: the fp32 squares of the walk's bound must not overflow).  diag = closest_diag(root).  DESIGN 5.32 derives the rule.
SR_HOST_DEVICE inline double closest_diag(const double mn[3], const double mx[3]) {
    const double ex = mx[0] - mn[0], ey = mx[1] - mn[1], ez = mx[2] - mn[2];
    return sqrt(ex * ex + ey * ey + ez * ez);
}
SR_HOST_DEVICE inline bool closest_regular(const double q[3], const double centre[3], double diag) {
    const double reach = diag * 1048576.0 < 0x1p60 ? diag * 1048576.0 : 0x1p60;
    const double rx = q[0] - centre[0], ry = q[1] - centre[1], rz = q[2] - centre[2];
    // (a NaN or infinite component fails its comparison)
    return rx >= -reach && rx <= reach && ry >= -reach && ry <= reach && rz >= -reach && rz <= reach;
}

}  // namespace sr
