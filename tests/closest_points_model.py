"""The definition of sr_closest_points (include/softray.h) in numpy: the Voronoi-region routine of softray_amd/csrc/sr_closest.h operation for
operation -- elementwise float64 + - * / and comparisons in the header routine's operand order -- vectorised over (points x triangles), then
the answer: the triangle that minimises (d2, TriangleIndex) over the triangles whose d2 is a number, and the limit on sqrt(d2).
A vectorised routine cannot branch, so every region's result is computed for every pair and the first region whose condition holds is selected,
which is what the header's if-chain does."""
import numpy as np

REGIONS = ("A", "B", "C", "AB", "AC", "BC", "face")          # the routine's return values 0 .. 6
CHUNK = 256                                                  # points per block of the (points x triangles) arrays


def closest_pairs(q, v9):
    """closest_point_triangle for every pair: q [P][3], v9 [T][9] or [T][3][3] -> (c [P][T][3], v [P][T], w [P][T], region [P][T])."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 1, 3)
    t = np.asarray(v9, dtype=np.float64).reshape(1, -1, 9)
    with np.errstate(all="ignore"):
        a, b, c = t[..., 0:3], t[..., 3:6], t[..., 6:9]
        abx, aby, abz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
        acx, acy, acz = c[..., 0] - a[..., 0], c[..., 1] - a[..., 1], c[..., 2] - a[..., 2]
        apx, apy, apz = q[..., 0] - a[..., 0], q[..., 1] - a[..., 1], q[..., 2] - a[..., 2]
        d1 = abx * apx + aby * apy + abz * apz
        d2 = acx * apx + acy * apy + acz * apz
        bpx, bpy, bpz = q[..., 0] - b[..., 0], q[..., 1] - b[..., 1], q[..., 2] - b[..., 2]
        d3 = abx * bpx + aby * bpy + abz * bpz
        d4 = acx * bpx + acy * bpy + acz * bpz
        cpx, cpy, cpz = q[..., 0] - c[..., 0], q[..., 1] - c[..., 1], q[..., 2] - c[..., 2]
        d5 = abx * cpx + aby * cpy + abz * cpz
        d6 = acx * cpx + acy * cpy + acz * cpz
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        d43, d56 = d4 - d3, d5 - d6
        conds = [(d1 <= 0.0) & (d2 <= 0.0), (d3 >= 0.0) & (d4 <= d3), (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), (d6 >= 0.0) & (d5 <= d6),
                 (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), (va <= 0.0) & (d43 >= 0.0) & (d56 >= 0.0)]
        codes = [0, 1, 3, 2, 4, 5]
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = d43 / (d43 + d56)
        s = va + vb + vc
        v_f, w_f = vb / s, vc / s
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        shape = d1.shape
        full = lambda x: np.broadcast_to(x, shape)                                           # noqa: E731
        cands = [
            (zero, zero, [full(a[..., k]) for k in range(3)]),
            (one, zero, [full(b[..., k]) for k in range(3)]),
            (v_ab, zero, [a[..., 0] + abx * v_ab, a[..., 1] + aby * v_ab, a[..., 2] + abz * v_ab]),
            (zero, one, [full(c[..., k]) for k in range(3)]),
            (zero, w_ac, [a[..., 0] + acx * w_ac, a[..., 1] + acy * w_ac, a[..., 2] + acz * w_ac]),
            (1.0 - w_bc, w_bc, [b[..., k] + (c[..., k] - b[..., k]) * w_bc for k in range(3)]),
        ]
        v, w = v_f, w_f
        pt = [a[..., 0] + abx * v_f + acx * w_f, a[..., 1] + aby * v_f + acy * w_f, a[..., 2] + abz * v_f + acz * w_f]
        region = np.full(shape, 6, dtype=np.int8)
        for cond, code, (cv, cw, cp) in reversed(list(zip(conds, codes, cands))):            # the FIRST condition that holds wins
            v = np.where(cond, cv, v)
            w = np.where(cond, cw, w)
            pt = [np.where(cond, cp[k], pt[k]) for k in range(3)]
            region = np.where(cond, np.int8(code), region)
    return np.stack(pt, axis=-1), v, w, region


def squared_distance(q, c):
    """closest_d2: (q - c).x^2 + (q - c).y^2 + (q - c).z^2, summed in that order; q [P][3] against c [P][T][3]."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 1, 3)
    with np.errstate(all="ignore"):
        dx, dy, dz = q[..., 0] - c[..., 0], q[..., 1] - c[..., 1], q[..., 2] - c[..., 2]
        return dx * dx + dy * dy + dz * dz


class Answers:
    """The answers of `points` against `v9` without a limit, computed once: tri [P] (-1: no triangle with a numeric d2), d2, dist, pos, uv,
    region of the answer, `ties` [P] (another triangle has the same d2), `nan_pairs` [P] (triangles skipped for a NaN d2)."""

    def __init__(self, points, v9):
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        P = points.shape[0]
        self.points = points
        self.tri = np.full(P, -1, dtype=np.int32)
        self.d2 = np.zeros(P)
        self.pos = np.zeros((P, 3))
        self.uv = np.zeros((P, 2))
        self.region = np.full(P, -1, dtype=np.int8)
        self.ties = np.zeros(P, dtype=bool)
        self.nan_pairs = np.zeros(P, dtype=np.int64)
        T = np.asarray(v9).reshape(-1, 9).shape[0]
        for lo in range(0, P if T else 0, CHUNK):
            sl = slice(lo, min(P, lo + CHUNK))
            c, v, w, region = closest_pairs(points[sl], v9)
            d2 = squared_distance(points[sl], c)
            valid = ~np.isnan(d2)
            key = np.where(valid, d2, np.inf)
            j = np.argmin(key, axis=1)                                                       # the first minimum: the lowest TriangleIndex
            rows = np.arange(j.shape[0])
            has = valid.any(axis=1)
            wrong = has & ~valid[rows, j]                                                    # every numeric d2 is +inf: the first of those
            j[wrong] = np.argmax(valid[wrong], axis=1)
            self.tri[sl] = np.where(has, j, -1)
            self.d2[sl] = np.where(has, d2[rows, j], 0.0)
            self.pos[sl] = np.where(has[:, None], c[rows, j], 0.0)
            self.uv[sl] = np.where(has[:, None], np.stack([v[rows, j], w[rows, j]], axis=1), 0.0)
            self.region[sl] = np.where(has, region[rows, j], -1)
            self.ties[sl] = has & ((valid & (d2 == d2[rows, j][:, None])).sum(axis=1) > 1)
            self.nan_pairs[sl] = (~valid).sum(axis=1)
        with np.errstate(all="ignore"):
            self.dist = np.sqrt(self.d2)

    def outputs(self, max_dist=None):
        """What the call reports under `max_dist` ([P] or None): dict(tri_index, dist, pos, uv)."""
        ok = self.tri >= 0
        if max_dist is not None:
            with np.errstate(all="ignore"):
                ok = ok & (self.dist <= np.asarray(max_dist, dtype=np.float64))
        return dict(tri_index=np.where(ok, self.tri, -1).astype(np.int32), dist=np.where(ok, self.dist, 0.0),
                    pos=np.where(ok[:, None], self.pos, 0.0), uv=np.where(ok[:, None], self.uv, 0.0))


def regular(points, bmin, bmax):
    """closest_regular (sr_closest.h): finite and no component further from the box centre than min(2^20 box diagonals, 2^60)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    bmin, bmax = np.asarray(bmin, dtype=np.float64), np.asarray(bmax, dtype=np.float64)
    e = bmax - bmin
    diag = np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
    reach = diag * 1048576.0 if diag * 1048576.0 < 2.0 ** 60 else 2.0 ** 60
    centre = (bmin + bmax) * 0.5
    with np.errstate(all="ignore"):
        r = points - centre
        return ((r >= -reach) & (r <= reach)).all(axis=1)


def same_bits(a, b):
    """Exact equality of two arrays, NaN payloads and the sign of zero included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
