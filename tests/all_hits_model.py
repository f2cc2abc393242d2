"""The model of sr_all_hits_rays, shared by tests/test_all_hits_model.py (CPU) and tests/test_gpu_all_hits.py.

Triangle j is in the hit set of a ray iff a scene that holds triangle j ALONE, in the same box, answers the ray with a hit, and ray_frac is
that answer's: for the own BVH the oracle's Scene.trace(3, ...) (NearestIntersect: the start clipped to the box, the hit inside it, ray_frac =
t + offset), for brute force its target 0 (GeometryCollection's loop from the unclipped start).  Extra element e likewise: an empty model with
set_extra([e]), traced with target 2; a ray_frac of DBL_MAX or more does not count; it is reported with index -2 - e.
A hit qualifies iff ray_frac <= limit (IEEE <=; no limit: every hit).  count = the qualifying hits; a row = the first min(count, K) of them by
(ray_frac, extra elements before triangles, element / TriangleIndex), the other slots index -1 / ray_frac 0.0."""
import numpy as np

from helpers import orc

TRACE_BRUTE, TRACE_ROOT_TREE, TRACE_NEAREST = 0, 2, 3
DBL_MAX = np.finfo(np.float64).max


class Candidates:
    """Every (ray, triangle / extra element) answer of a ray set: hit [C][n] bool, frac [C][n], and per candidate its index and its class key
    (extra elements first: key e, triangles 2^31 + j)."""

    def __init__(self, tris, prims, starts, D, brute):
        v9, argb, lo, hi = tris
        v9 = np.ascontiguousarray(v9, dtype=np.float64).reshape(-1, 9)
        starts = np.ascontiguousarray(starts)
        D = np.ascontiguousarray(D)
        n = starts.shape[0]
        hit, frac, index, key = [], [], [], []
        for e, p in enumerate(prims):
            o = orc.Scene()
            o.set_triangles(np.zeros((0, 9)), np.zeros(0, dtype=np.uint32), lo, hi)
            o.set_extra([p])
            assert o.build_tree() == 0
            res = o.trace(TRACE_ROOT_TREE, starts, D)
            with np.errstate(invalid="ignore"):
                hit.append(np.asarray(res["hit"]).astype(bool) & (np.asarray(res["ray_frac"]) < DBL_MAX))
            frac.append(np.array(res["ray_frac"]))
            index.append(-2 - e)
            key.append(e)
        for j in range(v9.shape[0]):
            o = orc.Scene()
            o.set_triangles(v9[j:j + 1], argb[j:j + 1], lo, hi)
            if brute:
                res = o.trace(TRACE_BRUTE, starts, D)
            else:
                assert o.build_tree() == 0
                res = o.trace(TRACE_NEAREST, starts, D)
            hit.append(np.asarray(res["hit"]).astype(bool))
            frac.append(np.array(res["ray_frac"]))
            index.append(j)
            key.append(2 ** 31 + j)
        self.n = n
        self.hit = np.array(hit, dtype=bool).reshape(len(index), n)
        self.frac = np.array(frac, dtype=np.float64).reshape(len(index), n)
        self.index = np.array(index, dtype=np.int64)
        self.key = np.array(key, dtype=np.int64)
        for a in (self.hit, self.frac, self.index, self.key):
            a.setflags(write=False)

    def lists(self, limits=None):
        """Per ray the qualifying hits in the order: a list of (ray_frac [c], index [c])."""
        out = []
        for i in range(self.n):
            q = self.hit[:, i].copy()
            if limits is not None:
                with np.errstate(invalid="ignore"):
                    q &= self.frac[:, i] <= limits[i]
            c = np.flatnonzero(q)
            order = np.lexsort((self.key[c], self.frac[c, i]))
            c = c[order]
            out.append((self.frac[c, i], self.index[c]))
        return out


def merged(extra, tris):
    """The candidates of a root geometry from those of its extra elements and of its triangles (the same rays)."""
    out = Candidates.__new__(Candidates)
    out.n = tris.n
    out.hit = np.concatenate([extra.hit, tris.hit])
    out.frac = np.concatenate([extra.frac, tris.frac])
    out.index = np.concatenate([extra.index, tris.index])
    out.key = np.concatenate([extra.key, tris.key])
    return out


def rows(lists, K):
    """dict(count uint32 [n], index int32 [n][K], ray_frac float64 [n][K]) of lists()."""
    n = len(lists)
    count = np.array([f.shape[0] for f, _ in lists], dtype=np.uint32)
    index = np.full((n, K), -1, dtype=np.int32)
    frac = np.zeros((n, K), dtype=np.float64)
    for i, (f, ix) in enumerate(lists):
        m = min(K, f.shape[0])
        index[i, :m] = ix[:m]
        frac[i, :m] = f[:m]
    return dict(count=count, index=index, ray_frac=frac)


def tied(lists):
    """Per ray: two qualifying hits share a ray_frac."""
    return np.array([bool(f.shape[0] > 1 and np.any(f[1:] == f[:-1])) for f, _ in lists])


def first_tied(lists):
    """Per ray: another qualifying hit shares the first one's ray_frac."""
    return np.array([bool(f.shape[0] > 1 and f[1] == f[0]) for f, _ in lists])


def same_rows(got, want, keys=("count", "index", "ray_frac")):
    """Equal bit for bit (a -0.0 is not a 0.0), same shapes."""
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
            return False
    return True
