"""The definition of sr_near_triangles (include/softray.h) in numpy, on the model of sr_closest_points (tests/closest_points_model.py): every
pair's closest point and d2 (closest_pairs, squared_distance), the set under the limit -- d2 a number and sqrt(d2) <= limit, IEEE <= on the
rounded square root -- a stable sort by (d2, TriangleIndex), then counts and rows.  The pairs of a block of points are formed once and every
limit set is answered from them; a row is kept to SLOTS = 64 entries (SR_HITS_MAX), rows(K) cuts it to K."""
import numpy as np

import closest_points_model as cpm

SLOTS = 64
KEYS = ("count", "index", "dist", "pos", "uv")
NP_TYPES = dict(count=np.uint32, index=np.int32, dist=np.float64, pos=np.float64, uv=np.float64)


def shapes(n, k):
    return dict(count=(n,), index=(n, k), dist=(n, k), pos=(n, k, 3), uv=(n, k, 2))


class Rows:
    """The answers of P points under one limit set: count [P] (not capped), and to SLOTS entries per point index (-1 beyond the set), d2,
    dist, pos, uv (zeros beyond the set)."""

    def __init__(self, P):
        self.count = np.zeros(P, dtype=np.uint32)
        self.index = np.full((P, SLOTS), -1, dtype=np.int32)
        self.d2 = np.zeros((P, SLOTS))
        self.dist = np.zeros((P, SLOTS))
        self.pos = np.zeros((P, SLOTS, 3))
        self.uv = np.zeros((P, SLOTS, 2))

    def rows(self, k):
        """What the call reports with max_hits = k: dict(count, index, dist, pos, uv)."""
        return dict(count=self.count.copy(), index=np.ascontiguousarray(self.index[:, :k]), dist=np.ascontiguousarray(self.dist[:, :k]),
                    pos=np.ascontiguousarray(self.pos[:, :k]), uv=np.ascontiguousarray(self.uv[:, :k]))

    def closest(self):
        """Slot 0 in sr_closest_points' form: dict(tri_index, dist, pos, uv)."""
        return dict(tri_index=np.ascontiguousarray(self.index[:, 0]), dist=np.ascontiguousarray(self.dist[:, 0]), pos=np.ascontiguousarray(self.pos[:, 0]),
                    uv=np.ascontiguousarray(self.uv[:, 0]))


def _fill(out, sl, member, d2, c, v, w):
    """The rows of one block: `member` [p][T] is the set, ordered by (d2, index) with a stable sort."""
    p, T = d2.shape
    order = np.lexsort((np.where(member, d2, 0.0), ~member), axis=1)[:, :SLOTS]               # members first, d2 ascending, ties in index order
    r = np.arange(p)[:, None]
    keep = member[r, order]
    s = order.shape[1]
    out.count[sl] = member.sum(axis=1)
    out.index[sl, :s] = np.where(keep, order, -1)
    kd2 = np.where(keep, d2[r, order], 0.0)
    out.d2[sl, :s] = kd2
    with np.errstate(all="ignore"):
        out.dist[sl, :s] = np.sqrt(kd2)
    out.pos[sl, :s] = np.where(keep[..., None], c[r, order], 0.0)
    out.uv[sl, :s] = np.where(keep[..., None], np.stack([v[r, order], w[r, order]], axis=-1), 0.0)


def near_sets(points, v9, make_limits=None):
    """{"none": Rows without a limit, name: Rows under make_limits(first, none_block)[name]}.  make_limits(first, block) is called per block of
    points with the index of its first point and the block's Rows without a limit (block.dist[:, 0] the nearest distance, [:, 3] the 4th
    neighbour's), and returns {name: limits [p]}.  Also "nan_pairs" [P]: the pairs of a point skipped for a NaN d2."""
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    P = points.shape[0]
    T = np.asarray(v9).reshape(-1, 9).shape[0]
    out = {"none": Rows(P), "nan_pairs": np.zeros(P, dtype=np.int64)}
    for lo in range(0, P if T else 0, cpm.CHUNK):
        sl = slice(lo, min(P, lo + cpm.CHUNK))
        c, v, w, _ = cpm.closest_pairs(points[sl], v9)
        d2 = cpm.squared_distance(points[sl], c)
        valid = ~np.isnan(d2)
        out["nan_pairs"][sl] = (~valid).sum(axis=1)
        _fill(out["none"], sl, valid, d2, c, v, w)
        if make_limits is None:
            continue
        block = Rows(sl.stop - sl.start)
        for k in ("count", "index", "d2", "dist", "pos", "uv"):
            getattr(block, k)[...] = getattr(out["none"], k)[sl]
        with np.errstate(all="ignore"):
            dist = np.sqrt(d2)
            for name, lim in make_limits(lo, block).items():
                if name not in out:
                    out[name] = Rows(P)
                member = valid & (dist <= np.asarray(lim, dtype=np.float64)[:, None])
                _fill(out[name], sl, member, d2, c, v, w)
    return out


def same_bits(a, b):
    return cpm.same_bits(a, b)
