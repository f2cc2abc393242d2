"""Scenes, ray sets and limits of the any-hit tests (tests/test_gpu_occluded_rays.py), shared with tests/test_occluded_rays_model.py, which
checks on the CPU -- with the oracle -- that between 10 % and 90 % of the regular rays of every set are occluded and that every kind of
limit and of irregular ray occurs.

Scenes (tests/gbuffer_cases.py): "small", 48 large triangles (at most 64: the own BVH is built on the host); "cube", unit_cube_scene(2000),
traced alone and -- SR_TARGET_ROOT -- with its extra primitives (a plane, a sphere and a box outside the root box).
Ray sets: "segments" seeded segments between points inside and around the box (end points); "shadow" segments from a light point to
pos + n * 0.001 of the oracle's hits of a 24 x 20 grid (end points); "probes" seeded hemisphere directions from those points; "far" starts
several box sizes outside the box, aimed at it, so that the clip offset of a ray exceeds some of its limits; "n1" .. "n449" 1, 63, 64, 65 and
64 * 7 + 1 segments; "irregular" directions and "irregular_ends" end points with an irregular ray of every kind in every eighth position.
Limits: "rot" -- with f the oracle's ray_frac of a hitting ray (1.0 for a miss) the twelve kinds of LIMIT_KINDS in rotation; the end-point sets
also with None (the default 1.0: "the segment is blocked"), the probes also with 2.0 throughout (AmbientOcclusion.cs)."""
import numpy as np

import gbuffer_cases as gbc
import origin_rays_cases as oc
import pathtrace_model as ptm

SCENES = ("small", "cube")
SETS = ("segments", "shadow", "probes", "far", "n1", "n63", "n64", "n65", "n449", "irregular", "irregular_ends")
LIMIT_KINDS = ("f", "f-", "f+", "0.5f", "2f", "0", "-1", "nan", "+inf", "-inf", "1e300", "5e-324")
# the kinds of irregular ray: per direction (oc.IRREGULAR_KINDS), a start that is not finite, a segment of length zero
IRREGULAR_DIR_KINDS = oc.IRREGULAR_KINDS + ("start-nan", "start-inf")
IRREGULAR_END_KINDS = ("zero-length", "end-nan", "end-inf", "start-nan", "x1e300")
PROBE_OFFSET = 0.001
LIGHT = np.array([0.15, 0.45, -0.3])               # a point inside the box, above its middle: some of the grid's hit points see it


def box(scene):
    return oc.box(scene)


def _grid_hits(scene):
    """(pos, normal) of the oracle's nearest hits of the 24 x 20 grid from the "out" origin."""
    tree, _ = gbc.oracle_scenes(scene)
    o = oc.origin_of(scene, "out")
    dirs = oc.grid_dirs(scene, "out")
    res = tree.trace(ptm.TRACE_NEAREST, np.tile(o, (dirs.shape[0], 1)), dirs)
    hit = np.asarray(res["hit"]).astype(bool)
    return np.ascontiguousarray(np.asarray(res["pos"])[hit]), np.ascontiguousarray(np.asarray(res["normal"])[hit])


_CACHE = {}


def grid_hits(scene):
    if scene not in _CACHE:
        _CACHE[scene] = _grid_hits(scene)
    return _CACHE[scene]


def _tri_points(scene, rng, n):
    """n seeded points on seeded triangles of the model, well inside their outlines."""
    v9 = np.asarray(gbc.scene_data(scene)[0][0], dtype=np.float64).reshape(-1, 3, 3)
    t = v9[rng.integers(0, v9.shape[0], size=n)]
    w = rng.uniform(0.15, 1.0, size=(n, 3))
    w /= w.sum(axis=1, keepdims=True)
    return (t * w[:, :, None]).sum(axis=1)


def _through(scene, a, p, rng):
    """Segments from a[i] through the triangle point p[i] and on, turned round where the oracle's nearest hit does not block them that way
    (triangles are one-sided)."""
    b = p + (p - a) * rng.uniform(0.2, 2.0, size=(a.shape[0], 1))
    tree, _ = gbc.oracle_scenes(scene)
    res = tree.trace(ptm.TRACE_NEAREST, a, np.ascontiguousarray(b - a))
    blocked = np.asarray(res["hit"]).astype(bool) & (np.asarray(res["ray_frac"]) <= 1.0)
    return np.where(blocked[:, None], a, b), np.where(blocked[:, None], b, a)


def _segments(scene, n, seed):
    """Seeded segments between points inside and around the box; six in ten of them are laid through a point of a model triangle."""
    lo, hi = box(scene)
    c, e = 0.5 * (lo + hi), hi - lo
    rng = np.random.default_rng(seed)
    a = c + e * rng.uniform(-0.8, 0.8, size=(n, 3))
    b = c + e * rng.uniform(-0.8, 0.8, size=(n, 3))
    aimed = rng.uniform(size=n) < 0.6
    if aimed.any():
        p = _tri_points(scene, rng, int(aimed.sum()))
        a[aimed], b[aimed] = _through(scene, np.ascontiguousarray(a[aimed]), p, rng)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def _base(scene, name):
    """(starts, dirs or end points, endpoints, kind per ray or "")."""
    lo, hi = box(scene)
    c, e = 0.5 * (lo + hi), hi - lo
    if name == "segments":
        a, b = _segments(scene, 400, 311)
        return a, b, True, None
    if name.startswith("n"):
        n = int(name[1:])
        a, b = _segments(scene, n, 1000 + n)
        return a, b, True, None
    if name == "shadow":
        pos, nrm = grid_hits(scene)
        ends = np.ascontiguousarray(pos + nrm * PROBE_OFFSET)
        return np.ascontiguousarray(np.tile(c + e * LIGHT, (ends.shape[0], 1))), ends, True, None
    if name == "probes":
        pos, nrm = grid_hits(scene)
        # AmbientOcclusion.cs' draw: uniform in [-1, 1]^3, turned to the normal's side, not normalised.  24 seeded draws per point: two points in three
        # take the first one the oracle sees blocked within 2.0, the third the first it does not (a point without such a draw: its first)
        rng = np.random.default_rng(77)
        n, tries = pos.shape[0], 24
        s = np.ascontiguousarray(pos + nrm * PROBE_OFFSET)
        cand = rng.uniform(-1.0, 1.0, size=(tries, n, 3))
        flip = (cand * nrm[None]).sum(axis=2) < 0.0
        cand[flip] = -cand[flip]
        tree, _ = gbc.oracle_scenes(scene)
        pick = np.zeros(n, dtype=np.int64)
        found = np.zeros(n, dtype=bool)
        for k in range(tries):
            res = tree.trace(ptm.TRACE_NEAREST, s, np.ascontiguousarray(cand[k]))
            blocked = np.asarray(res["hit"]).astype(bool) & (np.asarray(res["ray_frac"]) <= 2.0)
            take = ~found & (blocked == (np.arange(n) % 3 != 0))
            pick[take] = k
            found |= take
        return s, np.ascontiguousarray(cand[pick, np.arange(n)]), False, None
    if name == "far":
        rng = np.random.default_rng(909)
        n = 384
        s = c + e * (np.array([3.0, 2.5, -3.5]) + rng.uniform(-0.3, 0.3, size=(n, 3)))
        aim = c + e * rng.uniform(-0.45, 0.45, size=(n, 3))
        aimed = rng.uniform(size=n) < 0.7                                   # ... seven in ten at a point of a model triangle
        aim[aimed] = _tri_points(scene, rng, int(aimed.sum()))
        return np.ascontiguousarray(s), np.ascontiguousarray((aim - s) * 0.8), False, None
    if name == "irregular":
        a, b = _segments(scene, 512, 4242)
        d = np.ascontiguousarray(b - a)
        kinds = [""] * 512
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            for j, i in enumerate(range(0, 512, 8)):
                kind = IRREGULAR_DIR_KINDS[j % len(IRREGULAR_DIR_KINDS)]
                base = d[i] / np.abs(d[i]).max()
                if kind == "zero":
                    d[i] = 0.0
                elif kind == "nan":
                    d[i, j % 3] = np.nan
                elif kind == "+inf":
                    d[i, j % 3] = np.inf
                elif kind == "-inf":
                    d[i, j % 3] = -np.inf
                elif kind == "x1e300":
                    d[i] = base * 1e300
                elif kind == "x1e-300":
                    d[i] = base * 1e-300
                elif kind == "start-nan":
                    a[i, j % 3] = np.nan
                else:
                    a[i, j % 3] = np.inf if j % 2 else -np.inf
                kinds[i] = kind
        return a, d, False, kinds
    if name == "irregular_ends":
        a, b = _segments(scene, 320, 5151)
        kinds = [""] * 320
        for j, i in enumerate(range(0, 320, 8)):
            kind = IRREGULAR_END_KINDS[j % len(IRREGULAR_END_KINDS)]
            if kind == "zero-length":
                b[i] = a[i]
            elif kind == "end-nan":
                b[i, j % 3] = np.nan
            elif kind == "end-inf":
                b[i, j % 3] = np.inf if j % 2 else -np.inf
            elif kind == "start-nan":
                a[i, j % 3] = np.nan
            else:
                b[i] = (b[i] - a[i]) / np.abs(b[i] - a[i]).max() * 1e300
            kinds[i] = kind
        return a, b, True, kinds
    raise KeyError(name)


def directions(starts, dirs, endpoints):
    """D of every ray: the end point minus the start is one FP64 subtraction per component, as the library's."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.ascontiguousarray(dirs - starts) if endpoints else dirs


def limit_kind(i):
    """The kind of ray i's limit: the rotation, moved on by five every eight rays so that the irregular positions meet every kind too."""
    return (i + 5 * (i // 8)) % len(LIMIT_KINDS)


def rotated_limits(f):
    """f: the oracle's ray_frac per ray (1.0 where it misses)."""
    out = np.empty(f.shape[0])
    for i, v in enumerate(f):
        k = LIMIT_KINDS[limit_kind(i)]
        out[i] = {"f": v, "f-": np.nextafter(v, -np.inf), "f+": np.nextafter(v, np.inf), "0.5f": 0.5 * v, "2f": 2.0 * v, "0": 0.0, "-1": -1.0,
                  "nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "1e300": 1e300, "5e-324": 5e-324}[k]
    return out


def regular(starts, dirs, endpoints, limits):
    """The library's routing rule (include/softray.h): the rays that take the any-hit walk on the own BVH."""
    d = directions(starts, dirs, endpoints)
    with np.errstate(invalid="ignore"):
        ok = oc.regular(d) & (np.abs(starts).max(axis=1) <= 2.0 ** 100) & np.isfinite(starts).all(axis=1)
        if limits is not None:
            ok &= ~np.isnan(limits) & (limits != -np.inf)
    return ok


class RaySet:
    """One set of one scene: starts, dirs (or end points), the end-point switch, the kinds of its irregular rays and its limit variants
    {name: limits or None}."""

    def __init__(self, scene, name):
        self.scene, self.name = scene, name
        self.starts, self.dirs, self.endpoints, self.kinds = _base(scene, name)
        self.n = self.starts.shape[0]
        self.D = directions(self.starts, self.dirs, self.endpoints)
        tree, _ = gbc.oracle_scenes(scene)
        near = tree.trace(ptm.TRACE_NEAREST, self.starts, self.D)
        f = np.where(np.asarray(near["hit"]).astype(bool), np.asarray(near["ray_frac"]), 1.0)
        self.f = f
        self.limits = {"rot": rotated_limits(f)}
        if self.endpoints:
            self.limits["default"] = None
        if name == "probes":
            self.limits["two"] = np.full(self.n, 2.0)

    def limit_array(self, variant):
        lim = self.limits[variant]
        return np.full(self.n, 1.0) if lim is None else lim

    def regular(self, variant):
        return regular(self.starts, self.dirs, self.endpoints, self.limits[variant])


_SETS = {}


def ray_set(scene, name):
    if (scene, name) not in _SETS:
        _SETS[(scene, name)] = RaySet(scene, name)
    return _SETS[(scene, name)]


def oracle_trace(tree, brute, mode, root, prims, starts, dirs):
    """tests/origin_rays_cases.py oracle_trace for rays with starts of their own: mode "tree" / "brute" / "bvh", alone or (root) with the extra
    geometry; None where the oracle has no answer for the own BVH's root geometry."""
    if mode == "tree":
        return tree.trace(ptm.TRACE_ROOT_TREE if root else 1, starts, dirs)
    if mode == "brute":
        return brute.trace(ptm.TRACE_ROOT_TREE if root else 0, starts, dirs)
    near = tree.trace(ptm.TRACE_NEAREST, starts, dirs)
    if not (root and prims):
        return near
    alone = tree.trace(1, starts, dirs)
    for k in ("hit", "ray_frac", "pos", "normal", "color", "tri_index"):
        if np.ascontiguousarray(alone[k]).tobytes() != np.ascontiguousarray(near[k]).tobytes():
            return None
    return tree.trace(ptm.TRACE_ROOT_TREE, starts, dirs)


def model(res, limits):
    """occluded = hit & (ray_frac <= limit) over an answer of trace(): IEEE <=, a NaN limit is 0."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(res["hit"]).astype(bool) & (np.asarray(res["ray_frac"]) <= limits)).astype(np.uint8)
