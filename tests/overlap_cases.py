"""Scenes and query triangles of the sr_overlap_triangles tests (tests/test_gpu_overlap_triangles.py), shared with tests/test_overlap_model.py,
which pins on the CPU what they hold.  The scenes are the closest-point tests' own (tests/closest_points_cases.py, imported and not edited):
at most about 2200 triangles; at most 1024 queries per scene, in these sets (queries(scene) concatenates them; slices(scene)[set]):
  self       128 evenly strided triangles of the scene itself: never themselves, always their neighbours
  moved      the same triangles translated by (0.013, -0.021, 0.017) x the largest box extent
  probes     4 x 128 random triangles: a point of the box plus three offsets of up to 2^-6, 2^-3, 0.5 and 4 largest extents (default_rng(5))
  flat       triangles without area about scene vertices and box points: a point, two equal vertices, three collinear vertices
  far        one or three vertices at 2^19 (regular), 2^21 and 2^40 (beyond the regular bound) box diagonals from the centre
  irregular  NaN, +inf, -inf or 1e300 in one coordinate of a scene triangle or of a probe
model(scene) answers the scene's queries once and is left unchanged."""
import functools

import numpy as np

import closest_points_cases as cpc
import overlap_model as om

SCENES = cpc.SCENES
KS = (0, 1, 4, 64)
SET_NAMES = ("self", "moved", "probes", "flat", "far", "irregular")
MOVE = (0.013, -0.021, 0.017)
PROBE_SIZES = (2.0 ** -6, 2.0 ** -3, 0.5, 4.0)
PROBES_PER_SIZE = 128
FAR = (2.0 ** 19, 2.0 ** 21, 2.0 ** 40)


@functools.lru_cache(maxsize=None)
def _sets(name):
    v9, _, bmin, bmax = cpc.scene(name)
    T = v9.shape[0]
    e = bmax - bmin
    ext = float(e.max())
    diag = float(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]))
    centre = (bmin + bmax) * 0.5
    rng = np.random.default_rng(5)
    sets = {}
    strided = cpc._strided(T, 128)
    sets["self"] = v9[strided].copy()
    sets["moved"] = v9[strided] + np.array(MOVE) * ext
    probes = []
    for size in PROBE_SIZES:
        at = bmin + rng.uniform(0.0, 1.0, size=(PROBES_PER_SIZE, 1, 3)) * e
        probes.append(at + rng.uniform(-1.0, 1.0, size=(PROBES_PER_SIZE, 3, 3)) * (size * ext))
    sets["probes"] = np.concatenate(probes)
    # without area: about vertices of the scene (a touch) and about points of the box
    flat = []
    for t in v9[cpc._strided(T, 12)]:
        a, b, c = t
        m = (a + b) * 0.5
        flat += [(a, a, a), (a, a, b), (a, b, b), (c, a, c), (a, m, b), (m, b, a)]
    for at in bmin + rng.uniform(0.0, 1.0, size=(12, 3)) * e:
        d = rng.uniform(-1.0, 1.0, size=3) * ext
        flat += [(at, at, at), (at - d, at - d, at + d), (at - d, at + d, at + d), (at - d, at, at + d), (at - d * 0.25, at + d * 0.5, at - d)]
    sets["flat"] = np.array(flat, dtype=np.float64)
    # far away: a vertex out there and the two others those of a scene triangle, or the whole triangle out there
    dirs = np.array(cpc.FAR_DIRS, dtype=np.float64)
    dirs /= np.abs(dirs).max(axis=1, keepdims=True)
    far = []
    for f in FAR:
        for k, d in enumerate(dirs):
            t = v9[(k * 37) % T]
            out = centre + d * (f * diag)
            far.append((out, t[1], t[2]) if k % 2 == 0 else (out, out + e * 0.25, out - e[::-1] * 0.125))
            if k % 4 == 0:
                far.append((t[0] + (t[1] - t[2]) * 0.25, out, centre - d * (f * diag)))
    sets["far"] = np.array(far, dtype=np.float64)
    irr = []
    base = np.concatenate([v9[cpc._strided(T, 6)], sets["probes"][2 * PROBES_PER_SIZE + np.arange(6)]])
    for n, val in enumerate((np.nan, np.inf, -np.inf, 1e300, -1e300)):
        for m, t in enumerate(base):
            q = t.copy()
            q[(n + m) % 3, (n + 2 * m) % 3] = val
            irr.append(q)
    sets["irregular"] = np.array(irr, dtype=np.float64)
    return {k: np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3, 3) for k, v in sets.items()}


@functools.lru_cache(maxsize=None)
def queries(name):
    """Every query of the scene's sets, [n][3][3], read-only."""
    q = np.ascontiguousarray(np.concatenate([_sets(name)[k] for k in SET_NAMES]))
    assert q.shape[0] <= 1024
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def slices(name):
    out, lo = {}, 0
    for k in SET_NAMES:
        n = _sets(name)[k].shape[0]
        out[k] = slice(lo, lo + n)
        lo += n
    return out


def regular(q, bmin, bmax):
    """Which queries walk the tree: each vertex passes closest_regular (softray_amd/csrc/sr_closest.h)."""
    e = bmax - bmin
    diag = float(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]))
    reach = min(diag * 1048576.0, 2.0 ** 60)
    with np.errstate(invalid="ignore"):
        r = q.reshape(-1, 9).reshape(-1, 3, 3) - (bmin + bmax) * 0.5
        return ((r >= -reach) & (r <= reach)).all(axis=(1, 2))


class Model:
    """queries [n][3][3]; rows: overlap_model.Rows of them against the scene (computed once, read-only)."""

    def __init__(self, name):
        self.name = name
        self.queries = queries(name)
        self.rows = om.overlap_rows(self.queries, cpc.scene(name)[0])
        for k in ("count", "index", "mask"):
            getattr(self.rows, k).setflags(write=False)

    def want(self, k):
        return self.rows.rows(k)

    def any(self):
        return self.rows.any()


@functools.lru_cache(maxsize=None)
def model(name):
    return Model(name)


def write_check_file(path, v9, q):
    """int64 T, int64 n, T x 9 doubles, n x 9 doubles."""
    with open(path, "wb") as f:
        np.array([v9.shape[0], q.shape[0]], dtype=np.int64).tofile(f)
        np.ascontiguousarray(v9, dtype=np.float64).tofile(f)
        np.ascontiguousarray(q, dtype=np.float64).tofile(f)
