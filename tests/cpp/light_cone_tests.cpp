// light_cone_tests.cpp -- the penumbra-plane filter of the packet shaft walk (softray_amd/csrc/sr_light_cone.h) against FP64 ground truth,
// on the CPU: no GPU, no library.  For random (triangle, light ball, surface point) triples in the unit-cube frame the program makes the
// LightCone record, runs the fp32 filter (light_cone_verdict: the expressions k_shaft_pkt4 evaluates) and traces a few thousand sample
// rays from points on and in the ball to the surface point with Triangle.IntersectRay's conditions as tri_blocks (sr_pipeline.hip)
// states them.  Required:   verdict 0 (rejected)  ->  no sample ray is blocked by the triangle
//                           verdict 2 (umbra)     ->  every sample ray is blocked
// It also counts the pairs on which the filter and the TriSlab filter it replaces (shaft_touches, restated below) disagree.
// usage: light_cone_tests [pairs per class]        exit 0 = both requirements hold for every pair
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../softray_amd/csrc/sr_light_cone.h"

using sr::LcLane;
using sr::LightCone;
using sr::TriSlab;

namespace {

struct V3 { double x, y, z; };
V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 operator*(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double len(V3 a) { return std::sqrt(dot(a, a)); }

// the unit cube, a little off the origin; lo / hi as RootBox has them
const V3 kCentre = {0.03, -0.02, 0.01};
const double kLo[3] = {kCentre.x - 0.5 - 1e-10, kCentre.y - 0.5 - 1e-10, kCentre.z - 0.5 - 1e-10};
const double kHi[3] = {kCentre.x + 0.5 + 1e-10, kCentre.y + 0.5 + 1e-10, kCentre.z + 0.5 + 1e-10};

bool inside(V3 p) { return kLo[0] < p.x && p.x < kHi[0] && kLo[1] < p.y && p.y < kHi[1] && kLo[2] < p.z && p.z < kHi[2]; }

// the part of the ray s + t d, t >= 0, inside the box: its first point (AxisAlignedBox.ClipLineSegment's start)
bool clip_start(V3& s, V3 d) {
    if (inside(s)) return true;
    double t0 = 0.0, t1 = 10000.0;
    const double sv[3] = {s.x, s.y, s.z}, dv[3] = {d.x, d.y, d.z};
    for (int a = 0; a < 3; ++a) {
        if (dv[a] == 0.0) { if (!(kLo[a] < sv[a] && sv[a] < kHi[a])) return false; continue; }
        double ta = (kLo[a] - sv[a]) / dv[a], tb = (kHi[a] - sv[a]) / dv[a];
        if (ta > tb) std::swap(ta, tb);
        t0 = std::max(t0, ta); t1 = std::min(t1, tb);
    }
    if (!(t0 <= t1)) return false;
    s = s + d * t0;
    return true;
}

// Triangle.cs:29-57 (triangle_record)
struct Tri { sr::Rec128 rec; double v[9]; };

// tri_blocks (sr_pipeline.hip): the sample ray from rs to rs + rd, rd = E' - rs
bool blocks(const double* p, V3 rs, V3 rd) {
    V3 s = rs;
    if (!clip_start(s, rd)) return false;
    const double offset = len(rs - s) / len(rd);
    const double startDist = s.x * p[0] + s.y * p[1] + s.z * p[2];
    const double dirDist = rd.x * p[0] + rd.y * p[1] + rd.z * p[2];
    if (dirDist >= 0.0) return false;
    double rf = p[3] - startDist;
    if (!(rf <= 0.0)) return false;
    rf = rf / dirDist;
    if (!(rf + offset <= 1.0)) return false;
    const V3 q = s + rd * rf;
    if (!inside(q)) return false;
    const V3 w = {q.x - p[4], q.y - p[5], q.z - p[6]};
    const double sv = (w.x * p[7] + w.y * p[8] + w.z * p[9]) / p[10];
    if (sv < 0.0 || sv > 1.0) return false;
    const double tv = (w.x * p[11] + w.y * p[12] + w.z * p[13]) / p[14];
    return sv >= 0.0 && tv >= 0.0 && sv + tv <= 1.0;
}

// k_make_slabs (sr_lbvh.hip) for a triangle that is not degenerate
TriSlab make_slab(const double* v) {
    const V3 a = V3{v[0], v[1], v[2]} - kCentre, b = V3{v[3], v[4], v[5]} - kCentre, c = V3{v[6], v[7], v[8]} - kCentre;
    V3 n = cross(b - a, c - a);
    n = n * (1.0 / len(n));
    TriSlab t;
    const V3 P[3] = {a, b, c};
    float* mm[3] = {t.m1, t.m2, t.m3};
    float* cc[3] = {&t.c1, &t.c2, &t.c3};
    for (int k = 0; k < 3; ++k) {
        V3 m = cross(n, P[(k + 1) % 3] - P[k]);
        m = m * (1.0 / len(m));
        if (dot(m, P[(k + 2) % 3] - P[k]) < 0) m = m * -1.0;
        mm[k][0] = (float)m.x; mm[k][1] = (float)m.y; mm[k][2] = (float)m.z;
        *cc[k] = (float)dot(m, P[k]);
    }
    t.n[0] = (float)n.x; t.n[1] = (float)n.y; t.n[2] = (float)n.z;
    t.d = (float)dot(n, a);
    return t;
}

// shaft_touches (sr_pipeline.hip) per lane: 0 / 1 / 2
int old_verdict(const TriSlab& s, const LcLane& q, double light_radius) {
    const float R = sr::shaft_radius(light_radius), u = 5.9604645e-8f;
    const float adl = fabsf(q.dx) + fabsf(q.dy) + fabsf(q.dz);
    const float backface = R * 1.001f + 1e-6f * adl + 1e-30f;
    const float dmax = sqrtf(q.dx * q.dx + q.dy * q.dy + q.dz * q.dz) * 1.0001f + R;
    const float s0 = q.a0 / (12.0f * u);
    const float c0 = 15.0f * u * s0 * dmax + 1e-9f * dmax, c1 = 16.0f * u * dmax;
    auto val = [&](const float* m, float c) { return fmaf(m[0], q.ex, fmaf(m[1], q.ey, fmaf(m[2], q.ez, -c))); };
    auto slope = [&](const float* m) { return fmaf(m[0], q.dx, fmaf(m[1], q.dy, fmaf(m[2], q.dz, 0.0f))); };
    const float G0 = val(s.n, s.d), N1 = slope(s.n);
    if (N1 < -backface || G0 > q.a0 || G0 + N1 + R < -q.a01) return 0;
    const float g2 = G0 * G0, ag = fabsf(G0);
    const float* mk[3] = {s.m1, s.m2, s.m3};
    const float ck[3] = {s.c1, s.c2, s.c3};
    float lo = 1e30f;
    for (int k = 0; k < 3; ++k) {
        const float K0 = val(mk[k], ck[k]), K1 = slope(mk[k]);
        const float A = fmaf(K0, N1, -(G0 * K1)), L = q.Rm * sqrtf(fmaf(K0, K0, g2)), e = fmaf(c1, fabsf(K0) + ag, c0);
        if (A + L + e < 0.0f) return 0;
        lo = fminf(lo, A - L - e);
    }
    if (!(lo > 0.0f && N1 > 2.0f * q.Rm + q.a01 && G0 < -4.0f * q.a0)) return 1;
    const float ulo = -G0 * (1.0f / (N1 + q.Rm)) * 0.999998f, uhi = -G0 * (1.0f / (N1 - q.Rm)) * 1.000002f;
    const float margin = fmaf(q.Rm, uhi, q.umargin);
    const float xl = fmaf(ulo, q.dx, q.ex), xh = fmaf(uhi, q.dx, q.ex), yl = fmaf(ulo, q.dy, q.ey), yh = fmaf(uhi, q.dy, q.ey), zl = fmaf(ulo, q.dz, q.ez), zh = fmaf(uhi, q.dz, q.ez);
    const bool umbra = ulo > 1e-6f && uhi < 0.5f && fmaxf(fabsf(xl), fabsf(xh)) + margin < q.hbx && fmaxf(fabsf(yl), fabsf(yh)) + margin < q.hby &&
                       fmaxf(fabsf(zl), fabsf(zh)) + margin < q.hbz;
    return umbra ? 2 : 1;
}

std::mt19937_64 rng(20261018);
double uni(double a, double b) { return a + (b - a) * std::uniform_real_distribution<double>(0.0, 1.0)(rng); }
V3 in_box(double shrink) { return {kCentre.x + uni(-0.5, 0.5) * shrink, kCentre.y + uni(-0.5, 0.5) * shrink, kCentre.z + uni(-0.5, 0.5) * shrink}; }
V3 unit_dir() {
    for (;;) { V3 d = {uni(-1, 1), uni(-1, 1), uni(-1, 1)}; const double l = len(d); if (l > 0.05 && l <= 1.0) return d * (1.0 / l); }
}

// unit offsets on (the first half) and in (the second half) the ball, the centre among them; scaled by the radius per case
std::vector<V3> ball;
void make_ball(int n) {
    ball.clear();
    ball.push_back({0, 0, 0});
    const double ga = 3.14159265358979323846 * (3.0 - std::sqrt(5.0));
    const int ns = n / 2;
    for (int i = 0; i < ns; ++i) {                                       // Fibonacci points on the sphere
        const double z = 1.0 - 2.0 * (i + 0.5) / ns, r = std::sqrt(std::max(0.0, 1.0 - z * z));
        ball.push_back({r * std::cos(ga * i), r * std::sin(ga * i), z});
    }
    for (const V3 axis : {V3{1, 0, 0}, V3{0, 1, 0}, V3{0, 0, 1}}) { ball.push_back(axis); ball.push_back(axis * -1.0); }
    while ((int)ball.size() < n) ball.push_back(unit_dir() * std::cbrt(uni(0.0, 1.0)));
}

enum Class { GENERIC = 0, STRADDLE, EDGE_TOUCH, POINT_LIGHT, FAR_LIGHT, NEAR_PLANE, NEAR_EDGE, INSIDE_BIG, NUM_CLASSES };
const char* kClassName[NUM_CLASSES] = {"generic", "ball straddles the plane", "ball touches an edge line", "R = 0", "light 1e3 x extent away",
                                       "points 1e-6 from the plane", "points near an edge line", "light among the triangles, R = 0.08"};

struct Tally { long pairs = 0, some_hit = 0, all_hit = 0, v0 = 0, v1 = 0, v2 = 0, bad_reject = 0, bad_umbra = 0, new_keeps = 0, old_keeps = 0, new_umbra_only = 0, old_umbra_only = 0; };

}  // namespace

int main(int argc, char** argv) {
    const int per_class = argc > 1 ? std::atoi(argv[1]) : 2500;
    const int kSamples = 2048;
    make_ball(kSamples);
    Tally tally[NUM_CLASSES];
    const float bext[3] = {1.0f, 1.0f, 1.0f};
    const double centre[3] = {kCentre.x, kCentre.y, kCentre.z};
    for (int cls = 0; cls < NUM_CLASSES; ++cls) {
        for (int it = 0; it < per_class; ++it) {
            // ---- the triangle: anything from a sliver of the box to most of it ----
            const double size = std::pow(10.0, uni(-2.5, 0.0));
            const V3 t0 = in_box(1.0 - size);
            double v[9];
            V3 tv[3];
            for (int k = 0; k < 3; ++k) {
                tv[k] = t0 + V3{uni(-0.5, 0.5), uni(-0.5, 0.5), uni(-0.5, 0.5)} * size;
                v[3 * k] = tv[k].x; v[3 * k + 1] = tv[k].y; v[3 * k + 2] = tv[k].z;
            }
            V3 n = cross(tv[1] - tv[0], tv[2] - tv[0]);
            if (len(n) < 1e-3 * size * size) { --it; continue; }         // (needles: k_make_slabs' all-zero record, never filtered)
            n = n * (1.0 / len(n));
            const sr::Rec128 rec = sr::triangle_record(v, 0u, 0);
            // ---- the light ----
            double radius = (it % 4 == 0) ? 0.2 : (it % 4 == 1 ? 0.08 : (it % 4 == 2 ? 0.02 : 0.0));
            V3 L = kCentre + unit_dir() * uni(0.2, 3.0);
            const int ek = it % 3;
            const V3 ea = tv[ek], eb = tv[(ek + 1) % 3];
            const V3 et = (eb - ea) * (1.0 / len(eb - ea));
            V3 em = cross(n, et);
            if (cls == STRADDLE) {
                if (radius == 0.0) radius = 0.05;
                L = tv[0] + (tv[1] - tv[0]) * uni(-2, 3) + (tv[2] - tv[0]) * uni(-2, 3) + n * (radius * uni(-1.2, 1.2));
            } else if (cls == EDGE_TOUCH) {
                if (radius == 0.0) radius = 0.05;
                const double ang = uni(0.0, 6.283185307179586), dist = radius * (it % 2 ? uni(0.9, 1.1) : uni(0.999, 1.003));
                L = ea + et * (len(eb - ea) * uni(-1, 2)) + (n * std::cos(ang) + em * std::sin(ang)) * dist;
            } else if (cls == POINT_LIGHT) radius = 0.0;
            else if (cls == FAR_LIGHT) L = kCentre + unit_dir() * 1000.0;
            else if (cls == INSIDE_BIG) { radius = 0.08; L = in_box(0.8); }
            const double Lv[3] = {L.x, L.y, L.z};
            const LightCone cone = sr::light_cone_record(v, centre, Lv, radius, false);
            const TriSlab slab = make_slab(v);
            // ---- surface points: four per (triangle, light) ----
            for (int pi = 0; pi < 4; ++pi) {
                V3 E;
                const double b1 = uni(-0.3, 1.3), b2 = uni(-0.3, 1.3);
                const V3 onplane = tv[0] + (tv[1] - tv[0]) * b1 + (tv[2] - tv[0]) * (b2 * (1.0 - std::min(1.0, std::max(0.0, b1))));
                if (cls == NEAR_PLANE) E = onplane + n * uni(-1e-6, 1e-6);
                else if (cls == NEAR_EDGE) {
                    const double mag = std::pow(10.0, uni(-7.0, -2.0));
                    E = ea + et * (len(eb - ea) * uni(-0.2, 1.2)) + (n * uni(-1, 1) + em * uni(-1, 1)) * mag;
                } else if (pi < 3) {
                    // in the (pen)umbra region: behind a point of the plane near the triangle, as seen from somewhere in the ball
                    const V3 from = L + unit_dir() * (radius * uni(0.0, 1.3));
                    V3 dir = onplane - from;
                    dir = dir * (1.0 / std::max(1e-12, len(dir)));
                    E = onplane + dir * std::pow(10.0, uni(-4.0, 0.0));
                } else E = in_box(1.0);
                // E' relative to the centre and L - E' as the kernels round them
                const float e[3] = {(float)(E.x - kCentre.x), (float)(E.y - kCentre.y), (float)(E.z - kCentre.z)};
                const float d[3] = {(float)(L.x - E.x), (float)(L.y - E.y), (float)(L.z - E.z)};
                const LcLane lane = sr::make_lc_lane(bext, e, d, radius);
                const int verdict = sr::light_cone_verdict(cone, lane);
                const int old = old_verdict(slab, lane, radius);
                long hits = 0;
                for (int si = 0; si < kSamples; ++si) {
                    const V3 rs = L + ball[si] * radius;
                    if (blocks(rec.p, rs, E - rs)) ++hits;
                }
                Tally& t = tally[cls];
                t.pairs++;
                if (hits > 0) t.some_hit++;
                if (hits == kSamples) t.all_hit++;
                (verdict == 0 ? t.v0 : (verdict == 1 ? t.v1 : t.v2))++;
                if (verdict == 0 && hits > 0) {
                    if (t.bad_reject++ < 5) std::printf("REJECTED A HIT: class %d it %d point %d hits %ld\n", cls, it, pi, hits);
                }
                if (verdict == 2 && hits < kSamples) {
                    if (t.bad_umbra++ < 5) std::printf("UMBRA WITH A MISS: class %d it %d point %d hits %ld\n", cls, it, pi, hits);
                }
                if (verdict != 0 && old == 0) t.new_keeps++;
                if (verdict == 0 && old != 0) t.old_keeps++;
                if (verdict == 2 && old != 2) t.new_umbra_only++;
                if (verdict != 2 && old == 2) t.old_umbra_only++;
            }
        }
    }
    long bad = 0;
    Tally sum;
    std::printf("%-38s %8s %8s %8s | %8s %8s %8s | %9s %9s | %9s %9s %9s %9s\n", "class", "pairs", "some hit", "all hit", "rejected", "cand", "umbra", "bad rej", "bad umbra",
                "new keeps", "old keeps", "new umbra", "old umbra");
    for (int cls = 0; cls < NUM_CLASSES; ++cls) {
        const Tally& t = tally[cls];
        std::printf("%-38s %8ld %8ld %8ld | %8ld %8ld %8ld | %9ld %9ld | %9ld %9ld %9ld %9ld\n", kClassName[cls], t.pairs, t.some_hit, t.all_hit, t.v0, t.v1, t.v2, t.bad_reject,
                    t.bad_umbra, t.new_keeps, t.old_keeps, t.new_umbra_only, t.old_umbra_only);
        bad += t.bad_reject + t.bad_umbra;
        sum.pairs += t.pairs; sum.some_hit += t.some_hit; sum.all_hit += t.all_hit; sum.v0 += t.v0; sum.v2 += t.v2;
        sum.new_keeps += t.new_keeps; sum.old_keeps += t.old_keeps; sum.new_umbra_only += t.new_umbra_only; sum.old_umbra_only += t.old_umbra_only;
    }
    std::printf("TOTAL pairs=%ld some_hit=%ld all_hit=%ld rejected=%ld umbra=%ld new_keeps_old_rejects=%ld old_keeps_new_rejects=%ld new_umbra_only=%ld old_umbra_only=%ld violations=%ld\n",
                sum.pairs, sum.some_hit, sum.all_hit, sum.v0, sum.v2, sum.new_keeps, sum.old_keeps, sum.new_umbra_only, sum.old_umbra_only, bad);
    // a run that never rejects, never meets a hit or never says umbra would prove nothing
    const bool vacuous = sum.v0 == 0 || sum.v2 == 0 || sum.some_hit == 0 || sum.all_hit == 0;
    if (vacuous) std::printf("VACUOUS: some verdict or some ground-truth class never occurred\n");
    return (bad || vacuous) ? 1 : 0;
}
