// sr_light_cone.h -- the per-(light, triangle) penumbra planes of the packet shaft walk (LightCone, sr_types.h): how the record is
// made (FP64, rounded once) and how a surface point is tested against it (fp32).  One text for the gfx950 kernels (k_light_cones,
// k_shaft_pkt4 in sr_pipeline.hip) and for a host compiler (tests/cpp/light_cone_tests.cpp); DESIGN.md 5.2 has the argument.
//
// In the cross-section perpendicular to edge k of a triangle (coordinates g = n.x - d, k = m_k.x - c_k) the surface point is
// E = (G0, K0) and the light centre is Lc = (GL, KL), rho = |Lc|.  shaft_touches' edge condition A_k + R L_k >= 0 is
//     rho |E| (sin(thE - thL) + sin gamma) >= 0,        sin gamma = R / rho,
// a condition on the angle thE alone.  For G0 <= 0 (thE in [pi/2, 3pi/2]) and GL > R (|thL| < pi/2 - gamma) the difference
// thE - thL lies in (gamma, 2pi - gamma), where the condition reads thE <= thL + pi + gamma: ONE half-plane through the edge
// line, the outer tangent plane of the ball,
//     o_k(x) = cos(thL + gamma) (m_k.x - c_k) - sin(thL + gamma) (n.x - d) >= 0.
// The umbra condition A_k - R L_k > 0 is, on the same set, thE < thL + pi - gamma: the inner tangent plane i_k (gamma -> -gamma).
// A ball that STRADDLES the plane: only its part S' in front of the plane holds sample starts that can hit (Triangle.IntersectRay is
// one-sided).  A ray from P in S' (angle thP in [-pi/2, pi/2]) to E passes inside edge k iff sin(thE - thP) >= 0 iff thP >= thE - pi, so
// the condition is thE <= pi + max thP over S': the same plane o_k when the ball's upper tangent point lies in front of the plane
// (cos(thL + gamma) > 0), and no condition at all (max thP = pi/2) when the ball reaches the plane on the inner side of the edge line.
#pragma once
#include <math.h>
#include <stdint.h>

#include "sr_types.h"

namespace sr {

// the light radius as every shaft kernel inflates it (make_shaft_ray): R, and Rm = 1.001 R for the edge terms
SR_HOST_DEVICE inline float shaft_radius(double light_radius) { return (float)light_radius * 1.00001f + 1e-30f; }
SR_HOST_DEVICE inline float shaft_radius_edges(double light_radius) { return shaft_radius(light_radius) * 1.001f; }

constexpr float kLcAlways = 1e30f;      // offset of a plane with a zero normal that every point passes (-kLcAlways: no point does)

// The record of triangle v = {v1, v2, v3} for the light ball (centre L, radius light_radius), planes in coordinates relative to
// `centre` (the root-box centre: the frame of TriSlab).  `degenerate`: the triangle's TriSlab is all zeros (k_make_slabs).
// Classes (the slack is relative to the light's distance and the triangle's):
//   ball entirely behind the plane (GL + Rm < -slack)  every sample ray starts behind the plane: never a candidate
//   ball not entirely in front     (GL <= Rm + slack)  inner planes never pass; the outer plane of edge k passes always unless the ball's
//                                                      upper tangent point in the edge's cross-section lies in front of the plane
//   edge line inside the ball      (rho_k <= Rm)       that edge's outer plane always passes, its inner plane never
//   degenerate                                         always a candidate, never umbra
SR_HOST_DEVICE inline LightCone light_cone_record(const double v[9], const double centre[3], const double L[3], double light_radius, bool degenerate) {
    LightCone c;
    for (int j = 0; j < 2; ++j) {
        c.gx_o1x[j] = c.gy_o1y[j] = c.gz_o1z[j] = 0.0f; c.gd_o1d[j] = kLcAlways;
        c.o23x[j] = c.o23y[j] = c.o23z[j] = 0.0f; c.o23d[j] = kLcAlways;
        c.i12x[j] = c.i12y[j] = c.i12z[j] = 0.0f; c.i12d[j] = -kLcAlways;
    }
    c.i3[0] = c.i3[1] = c.i3[2] = 0.0f; c.i3[3] = -kLcAlways;
    c.GL = 0.0f; c.pad[0] = c.pad[1] = c.pad[2] = 0.0f;
    if (degenerate) return c;
    const double Rm = (double)shaft_radius_edges(light_radius);
    const double P[3][3] = {{v[0] - centre[0], v[1] - centre[1], v[2] - centre[2]},
                            {v[3] - centre[0], v[4] - centre[1], v[5] - centre[2]},
                            {v[6] - centre[0], v[7] - centre[1], v[8] - centre[2]}};
    const double Lc[3] = {L[0] - centre[0], L[1] - centre[1], L[2] - centre[2]};
    const double e1[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]}, e2[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
    double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double nl = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(nl > 0.0) || !isfinite(nl)) return c;
    n[0] /= nl; n[1] /= nl; n[2] /= nl;
    const double d = n[0] * P[0][0] + n[1] * P[0][1] + n[2] * P[0][2];
    const double GL = n[0] * Lc[0] + n[1] * Lc[1] + n[2] * Lc[2] - d;
    double scale = fabs(Lc[0]) + fabs(Lc[1]) + fabs(Lc[2]);
    for (int k = 0; k < 3; ++k) scale += fabs(P[k][0]) + fabs(P[k][1]) + fabs(P[k][2]);
    const double slack = 1e-9 * scale + 1e-30;
    // the plane itself, negated: the filter's first value is -G0, so that all four candidate conditions read "value >= -margin"
    c.gx_o1x[0] = (float)-n[0]; c.gy_o1y[0] = (float)-n[1]; c.gz_o1z[0] = (float)-n[2]; c.gd_o1d[0] = (float)d;
    c.GL = (float)GL;
    if (GL + Rm < -slack) {                                             // never a candidate
        c.gx_o1x[0] = c.gy_o1y[0] = c.gz_o1z[0] = 0.0f; c.gd_o1d[0] = -kLcAlways;
        return c;
    }
    const bool front = GL > Rm + slack;                                 // the whole ball in front of the plane: inner planes exist
    float* ox[3] = {&c.gx_o1x[1], &c.o23x[0], &c.o23x[1]};
    float* oy[3] = {&c.gy_o1y[1], &c.o23y[0], &c.o23y[1]};
    float* oz[3] = {&c.gz_o1z[1], &c.o23z[0], &c.o23z[1]};
    float* od[3] = {&c.gd_o1d[1], &c.o23d[0], &c.o23d[1]};
    float* ix[3] = {&c.i12x[0], &c.i12x[1], &c.i3[0]};
    float* iy[3] = {&c.i12y[0], &c.i12y[1], &c.i3[1]};
    float* iz[3] = {&c.i12z[0], &c.i12z[1], &c.i3[2]};
    float* id[3] = {&c.i12d[0], &c.i12d[1], &c.i3[3]};
    for (int k = 0; k < 3; ++k) {
        const double* p0 = P[k];
        const double* p1 = P[(k + 1) % 3];
        const double* p2 = P[(k + 2) % 3];
        const double t[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
        double m[3] = {n[1] * t[2] - n[2] * t[1], n[2] * t[0] - n[0] * t[2], n[0] * t[1] - n[1] * t[0]};
        const double ml = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
        if (!(ml > 0.0) || !isfinite(ml)) continue;                     // (k_make_slabs calls such a triangle degenerate)
        double sgn = 1.0 / ml;
        if (m[0] * (p2[0] - p0[0]) + m[1] * (p2[1] - p0[1]) + m[2] * (p2[2] - p0[2]) < 0.0) sgn = -sgn;
        m[0] *= sgn; m[1] *= sgn; m[2] *= sgn;
        const double ck = m[0] * p0[0] + m[1] * p0[1] + m[2] * p0[2];
        const double KL = m[0] * Lc[0] + m[1] * Lc[1] + m[2] * Lc[2] - ck;
        const double rho = sqrt(GL * GL + KL * KL);
        if (!(rho > Rm + slack)) continue;
        const double lg = GL / rho, lk = KL / rho;                      // (cos thL, sin thL)
        const double sg = Rm / rho, cg = sqrt(fmax(0.0, 1.0 - sg * sg));  // (sin gamma, cos gamma)
        const double co = lg * cg - lk * sg, so = lk * cg + lg * sg;    // thL + gamma
        const double ci = lg * cg + lk * sg, si = lk * cg - lg * sg;    // thL - gamma
        // o_k(x) = co (m.x - ck) - so (n.x - d); the upper tangent point must lie in front of the plane (cos(thL + gamma) > 0: always so
        // for a ball in front), else the ball reaches the plane on the inner side of the edge and every point behind the plane passes
        if (!(co > 0.0)) continue;
        *ox[k] = (float)(co * m[0] - so * n[0]); *oy[k] = (float)(co * m[1] - so * n[1]); *oz[k] = (float)(co * m[2] - so * n[2]);
        *od[k] = (float)(so * d - co * ck);
        if (!front) continue;
        *ix[k] = (float)(ci * m[0] - si * n[0]); *iy[k] = (float)(ci * m[1] - si * n[1]); *iz[k] = (float)(ci * m[2] - si * n[2]);
        *id[k] = (float)(si * d - ci * ck);
    }
    return c;
}

// ---- the fp32 evaluation: two planes per chain of three (packed) FMAs, value = x ex + (y ey + (z ez + d)) ----
struct LcPair { float a, b; };

SR_HOST_DEVICE inline LcPair lc_planes2(const float x[2], const float y[2], const float z[2], const float d[2], float ex, float ey, float ez) {
#if defined(__HIPCC__)
    typedef float lc_f2 __attribute__((ext_vector_type(2)));
    const lc_f2 X = {x[0], x[1]}, Y = {y[0], y[1]}, Z = {z[0], z[1]}, D = {d[0], d[1]}, EX = {ex, ex}, EY = {ey, ey}, EZ = {ez, ez};
    const lc_f2 r = __builtin_elementwise_fma(X, EX, __builtin_elementwise_fma(Y, EY, __builtin_elementwise_fma(Z, EZ, D)));
    return LcPair{r.x, r.y};
#else
    return LcPair{fmaf(x[0], ex, fmaf(y[0], ey, fmaf(z[0], ez, d[0]))), fmaf(x[1], ex, fmaf(y[1], ey, fmaf(z[1], ez, d[1])))};
#endif
}
SR_HOST_DEVICE inline float lc_plane1(const float p[4], float ex, float ey, float ez) {
#if defined(__HIPCC__)
    return __builtin_fmaf(p[0], ex, __builtin_fmaf(p[1], ey, __builtin_fmaf(p[2], ez, p[3])));
#else
    return fmaf(p[0], ex, fmaf(p[1], ey, fmaf(p[2], ez, p[3])));
#endif
}

// first line: (-G0, o_1) and (o_2, o_3); a lane is a candidate iff none of the four values lies below -a0 (a NaN passes)
SR_HOST_DEVICE inline LcPair lc_stage_a(const LightCone& c, float ex, float ey, float ez) { return lc_planes2(c.gx_o1x, c.gy_o1y, c.gz_o1z, c.gd_o1d, ex, ey, ez); }
SR_HOST_DEVICE inline LcPair lc_stage_b(const LightCone& c, float ex, float ey, float ez) { return lc_planes2(c.o23x, c.o23y, c.o23z, c.o23d, ex, ey, ez); }
// second line: the smallest of the three inner-plane values.  (fminf drops a NaN operand; the coefficients are finite, so a NaN here
// needs a NaN in E', which makes G0 a NaN too, and the umbra test's `G0 < -4 a0` fails)
SR_HOST_DEVICE inline float lc_inner_min(const LightCone& c, float ex, float ey, float ez) {
    const LcPair i12 = lc_planes2(c.i12x, c.i12y, c.i12z, c.i12d, ex, ey, ez);
    return fminf(fminf(i12.a, i12.b), lc_plane1(c.i3, ex, ey, ez));
}

// (the kernels' v_rcp_f32 is good to 1 ulp, the host's division to half of one; the factors 0.999998 / 1.000002 cover both)
SR_HOST_DEVICE inline float lc_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}

// The per-lane constants of the filter (ShaftRay's, by name) and its verdict for one surface point: 0 no sample ray can hit the
// triangle, 1 candidate, 2 umbra.  k_shaft_pkt4 evaluates the same expressions with wave votes (shaft_cones_wave).
struct LcLane {
    float ex, ey, ez;           // E' relative to the root centre
    float dx, dy, dz;           // L - E'
    float Rm, a0, a01, umargin;
    float hbx, hby, hbz;        // half extents of the root box
};

// the constants as make_shaft_ray (sr_pipeline.hip) derives them for the surface point E' = centre + e, d = L - E', from the root box's
// extents b (the kernel takes its square roots with v_sqrt_f32, 1 ulp: the factors 1.002 / 1.0001 cover that)
SR_HOST_DEVICE inline LcLane make_lc_lane(const float b[3], const float e[3], const float d[3], double light_radius) {
    LcLane s;
    const float R = shaft_radius(light_radius), u = 5.9604645e-8f;
    s.ex = e[0]; s.ey = e[1]; s.ez = e[2]; s.dx = d[0]; s.dy = d[1]; s.dz = d[2];
    s.Rm = R * 1.001f;
    s.hbx = 0.5f * b[0]; s.hby = 0.5f * b[1]; s.hbz = 0.5f * b[2];
    const float s0 = (sqrtf(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]) * 0.5f + fabsf(e[0]) + fabsf(e[1]) + fabsf(e[2])) * 1.002f + 0.004f;
    const float dmax = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) * 1.0001f + R;
    s.a0 = 12.0f * u * s0;
    s.a01 = s.a0 + 20.0f * u * dmax + 0.002f * R;
    s.umargin = 3e-5f * fmaxf(fmaxf(b[0], b[1]), b[2]);
    return s;
}

SR_HOST_DEVICE inline int light_cone_verdict(const LightCone& c, const LcLane& s) {
    const LcPair A = lc_stage_a(c, s.ex, s.ey, s.ez);
    if (A.a < -s.a0 || A.b < -s.a0) return 0;
    const LcPair B = lc_stage_b(c, s.ex, s.ey, s.ez);
    if (B.a < -s.a0 || B.b < -s.a0) return 0;
    const float G0 = -A.a, N1 = c.GL - G0;
    const bool pre = lc_inner_min(c, s.ex, s.ey, s.ez) > s.a0 && N1 > 2.0f * s.Rm + s.a01 && G0 < -4.0f * s.a0;
    if (!pre) return 1;
    // the crossing parameters of all samples lie in [ulo, uhi]; the crossing region must be inside the root box (shaft_touches)
    const float ulo = -G0 * lc_rcp(N1 + s.Rm) * 0.999998f, uhi = -G0 * lc_rcp(N1 - s.Rm) * 1.000002f;
    const float margin = fmaf(s.Rm, uhi, s.umargin);
    const float xl = fmaf(ulo, s.dx, s.ex), xh = fmaf(uhi, s.dx, s.ex), yl = fmaf(ulo, s.dy, s.ey), yh = fmaf(uhi, s.dy, s.ey), zl = fmaf(ulo, s.dz, s.ez), zh = fmaf(uhi, s.dz, s.ez);
    const bool umbra = ulo > 1e-6f && uhi < 0.5f && fmaxf(fabsf(xl), fabsf(xh)) + margin < s.hbx && fmaxf(fabsf(yl), fabsf(yh)) + margin < s.hby &&
                       fmaxf(fabsf(zl), fabsf(zh)) + margin < s.hbz;
    return umbra ? 2 : 1;
}

}  // namespace sr
