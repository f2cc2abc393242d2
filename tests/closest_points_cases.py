"""Scenes and point sets of the closest-point tests (tests/test_gpu_closest_points.py), shared with tests/test_closest_points_model.py,
which pins on the CPU -- with the model of tests/closest_points_model.py -- what the sets hold.  Everything is small: at most 4096 points
and about 2000 triangles per scene.

Scenes: all_hits_cases' "small" (host-built tree), "cube" and "layers"; mesh_cases' torus at 40 x 20 ("torus") and its slivers; bvh_shape_cases'
tree at the depth limit ("limit"), exact duplicates ("duplicates") and the flat root box ("flat_thin"); placement_cases' "far_probe" and "cut" with
1500 triangles (away from the origin; triangles that stick out of the root box); "degenerate": a soup of 200 triangles and, at the indices
DEGENERATE_AT on, six triangles without area -- two with vertex 1 == vertex 2 (the edge region ab divides 0 by 0 for the points before
vertex 3: a NaN distance, skipped), one with all vertices equal, one with vertex 2 == vertex 3, two with three distinct collinear vertices.
Point sets of a scene (points(scene) concatenates them; SETS[name] is the slice):
  vertices   every distinct vertex of the mesh, at most 1024 (evenly strided): distance 0, ties among all incident triangles
  offsets    edge midpoints and centroids of 40 evenly strided triangles pushed along the triangle's normal by +-2^-16, +-2^-8, +-2^-3 and +-1
             largest box extents
  lattice    9^3 points through and around the box (1.5 x the box about its centre), and the box centre
  between    centroids of 128 evenly strided triangles moved half way to the centroid of the triangle 7 further on (duplicates: a copy
             perhaps; layers: the next layer perhaps), and those centroids themselves
  far        14 directions (axes and diagonals) at 2^10, 2^19, 2^18, 2^21 and 2^40 box diagonals from the centre: the last two lie beyond the
             regular bound
  irregular  NaN, +inf, -inf and 1e300 in each component of the box centre
Limits: limit_kinds(dist) rotates +inf, 0, the exact distance, one ulp below it, NaN, -inf, -1 and twice the distance over the points."""
import functools

import numpy as np

import all_hits_cases as ahc
import bvh_shape_cases as bsc
import bvh_shapes as bs
import mesh_cases as mc
import placement_cases as pc

SCENES = ("small", "cube", "layers", "torus", "slivers", "limit", "duplicates", "flat_thin", "far_probe", "cut", "degenerate")
DEGENERATE_AT = 200
HOST_BUILT_ONLY = ("small",)                 # at most 64 triangles: the library builds on the host by itself
SET_NAMES = ("vertices", "offsets", "lattice", "between", "far", "irregular")
OFFSETS = (2.0 ** -16, 2.0 ** -8, 2.0 ** -3, 1.0)
FAR = (2.0 ** 10, 2.0 ** 19, 2.0 ** 18, 2.0 ** 21, 2.0 ** 40)
FAR_DIRS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 1), (-1, -1, -1), (1, -1, 0), (0, 1, -1), (-1, 0, 1), (1, 1, -1),
            (-1, 1, 1), (1, -1, 1))
LIMIT_KINDS = ("inf", "zero", "exact", "below", "nan", "-inf", "negative", "double")


@functools.lru_cache(maxsize=None)
def scene(name):
    """(v9 [T][3][3] float64, argb, bmin, bmax), read-only."""
    if name in ahc.SCENES:
        made = ahc.scene_data(name)[0]
    elif name == "torus":
        made = mc._pack(mc._torus_tris(n_major=40, n_minor=20), mc.UNIT_LO, mc.UNIT_HI)
    elif name == "slivers":
        made = mc.scene("slivers")
    elif name in ("limit", "duplicates", "flat_thin"):
        made = bsc.scene(name)
    elif name == "degenerate":
        p, q, r = (0.125, 0.25, -0.125), (-0.25, 0.125, 0.375), (0.25, -0.375, 0.0)
        mid = tuple((a + b) * 0.5 for a, b in zip(p, q))
        flat = np.array([(p, p, q), (r, r, p), (q, q, q), (r, p, p), (p, mid, q), (q, p, mid)], dtype=np.float64)
        made = bs._pack([bs.soup(DEGENERATE_AT, (0.0, 0.0, 0.0), 0.8, 21), flat])
    else:
        made = pc.placed(name, n=1500)
    v9, argb, bmin, bmax = made
    v9 = np.ascontiguousarray(np.asarray(v9, dtype=np.float64).reshape(-1, 3, 3))
    out = (v9, np.ascontiguousarray(argb, dtype=np.uint32), np.ascontiguousarray(bmin, dtype=np.float64), np.ascontiguousarray(bmax, dtype=np.float64))
    for a in out:
        a.setflags(write=False)
    return out


def _strided(n, count):
    return np.unique(np.linspace(0, n - 1, min(n, count)).astype(np.int64))


@functools.lru_cache(maxsize=None)
def _sets(name):
    v9, _, bmin, bmax = scene(name)
    T = v9.shape[0]
    ext = float((bmax - bmin).max())
    e = bmax - bmin
    diag = float(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]))
    centre = (bmin + bmax) * 0.5
    sets = {}
    verts = np.unique(v9.reshape(-1, 3), axis=0)
    sets["vertices"] = verts[_strided(verts.shape[0], 1024)]
    t = v9[_strided(T, 40)]
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    nrm = np.cross(b - a, c - a)
    ln = np.sqrt((nrm * nrm).sum(axis=1, keepdims=True))
    nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), np.array([0.0, 0.0, 1.0]))
    base = np.concatenate([(a + b) * 0.5, (b + c) * 0.5, (c + a) * 0.5, (a + b + c) / 3.0])
    nn = np.concatenate([nrm] * 4)
    sets["offsets"] = np.concatenate([base + nn * (sgn * o * ext) for o in OFFSETS for sgn in (1.0, -1.0)])
    g = np.linspace(-0.75, 0.75, 9)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * e + centre
    sets["lattice"] = np.concatenate([lat, centre[None, :]])
    idx = _strided(T, 128)
    cen = v9.mean(axis=1)
    sets["between"] = np.concatenate([(cen[idx] + cen[(idx + 7) % T]) * 0.5, cen[idx]])
    dirs = np.array(FAR_DIRS, dtype=np.float64)
    dirs /= np.abs(dirs).max(axis=1, keepdims=True)
    sets["far"] = np.concatenate([centre + dirs * (f * diag) for f in FAR])
    irr = []
    for val in (np.nan, np.inf, -np.inf, 1e300):
        for k in range(3):
            p = centre.copy()
            p[k] = val
            irr.append(p)
    sets["irregular"] = np.array(irr)
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in sets.items()}


@functools.lru_cache(maxsize=None)
def points(name):
    """Every point of the scene's sets, [P][3], read-only; SETS(name)[set] is its slice."""
    p = np.ascontiguousarray(np.concatenate([_sets(name)[k] for k in SET_NAMES]))
    assert p.shape[0] <= 4096
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def slices(name):
    out, lo = {}, 0
    for k in SET_NAMES:
        n = _sets(name)[k].shape[0]
        out[k] = slice(lo, lo + n)
        lo += n
    return out


def limit_kinds(dist):
    """([P] limits, [P] kind index into LIMIT_KINDS): the eight kinds in rotation around every point's own distance."""
    dist = np.asarray(dist, dtype=np.float64)
    kind = np.arange(dist.shape[0]) % len(LIMIT_KINDS)
    table = np.stack([np.full_like(dist, np.inf), np.zeros_like(dist), dist, np.nextafter(dist, -np.inf), np.full_like(dist, np.nan),
                      np.full_like(dist, -np.inf), np.full_like(dist, -1.0), dist * 2.0])
    return np.ascontiguousarray(table[kind, np.arange(dist.shape[0])]), kind


CHECK_FILE = "closest_points_check.bin"      # under tests/golden/: int64 T, int64 P, T x 9 doubles, P x 3 doubles (tests/cpp/closest_point_check.cpp)


def check_file_contents():
    """(triangles [T][9], points [P][3]) of the committed point file, as it was made: the right triangle (0,0,0), (1,0,0), (0,1,0), 24 seeded
    triangles in [-1, 1]^3, a needle, the area-less triangles of "degenerate"; the right triangle's seven region points, every vertex of the
    first eight triangles, 96 seeded points in [-2, 2]^3, and NaN, +-inf, 1e300 and 1e-300 in one component each."""
    rng = np.random.default_rng(532)
    tris = [np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], dtype=np.float64), rng.uniform(-1.0, 1.0, size=(24, 9)),
            np.array([[0.0, 0.0, 0.0, 1.0, 2.0 ** -30, 0.0, 2.0, 0.0, 0.0]]), scene("degenerate")[0][DEGENERATE_AT:].reshape(-1, 9)]
    tris = np.ascontiguousarray(np.concatenate(tris))
    region_points = np.array([(-1, -1, .5), (2, -.5, .5), (-.5, 2, .5), (.25, -1, .5), (-1, .75, .5), (1, 1, .5), (.25, .25, .5)], dtype=np.float64)
    special = []
    for val in (np.nan, np.inf, -np.inf, 1e300, 1e-300):
        for k in range(3):
            p = np.array([0.25, 0.125, -0.5])
            p[k] = val
            special.append(p)
    pts = np.concatenate([region_points, tris[:8].reshape(-1, 3), rng.uniform(-2.0, 2.0, size=(96, 3)), np.array(special)])
    return tris, np.ascontiguousarray(pts)


def read_check_file(path):
    raw = np.fromfile(path, dtype=np.uint8)
    T, P = (int(x) for x in raw[:16].view(np.int64))
    body = raw[16:].view(np.float64)
    assert body.shape[0] == T * 9 + P * 3
    return body[:T * 9].reshape(T, 9).copy(), body[T * 9:].reshape(P, 3).copy()
