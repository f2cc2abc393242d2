"""Scenes and ray sets of the all-hits tests (tests/test_gpu_all_hits.py), shared with tests/test_all_hits_model.py, which pins on the CPU --
with the model of tests/all_hits_model.py -- how many hits, ties and overfull rows every set holds.

Scenes: "small" and "cube" with the ray sets of tests/occluded_rays_cases.py, unchanged (a ray crosses at most 6 triangles on them), and
"layers", which has the depth they lack: 40 layers at z_l = -0.45 + 0.9 (l + 0.5) / 40, each a 2 x 2 grid of quads over x, y in
{-0.4, 0, 0.4}, each quad the triangles (p00, p10, p11) and (p00, p11, p01); layers with l % 4 == 3 are wound the other way (the last two
vertices swapped), layers with l % 8 == 0 are emitted twice, as exact duplicates: 360 triangles in [-0.5, 0.5]^3 (more than 64: the own BVH
is built on the device).
Ray sets of "layers" (one rng = default_rng(2024) for all of them, drawn in this order, n = 256): "through" -- starts (U(-0.35, 0.35)^2, -0.48), directions (U(-0.15, 0.15)^2, 1) * 0.9,
every ray with i % 4 == 1 from z = +0.48 with direction z = -0.9; "far_through" -- the same rays with start - 3 dir (outside the box:
offset > 0); "oblique" -- segments between two U(-0.4, 0.4)^3 points (end points); "edges" -- 20 rays along +-z through shared vertices, grid
lines, diagonals and the outline."""
import numpy as np

import gbuffer_cases as gbc
import occluded_rays_cases as occ

SCENES = ("small", "cube", "layers")
LAYER_SETS = ("through", "far_through", "oblique", "edges")
EDGE_POINTS = ((0, 0), (0, .2), (.2, 0), (.2, .2), (-.2, -.2), (.4, .4), (-.4, 0), (.1, .1), (0, -.4), (.3, .3))
N_LAYERS = 40


def layers_scene():
    """(v9, argb, bmin, bmax) of "layers"."""
    tris = []
    xs = (-0.4, 0.0, 0.4)
    for l in range(N_LAYERS):
        z = -0.45 + 0.9 * (l + 0.5) / N_LAYERS
        layer = []
        for a in range(2):
            for b in range(2):
                p00, p10 = (xs[a], xs[b], z), (xs[a + 1], xs[b], z)
                p11, p01 = (xs[a + 1], xs[b + 1], z), (xs[a], xs[b + 1], z)
                for t in ((p00, p10, p11), (p00, p11, p01)):
                    layer.append((t[0], t[2], t[1]) if l % 4 == 3 else t)
        tris += layer
        if l % 8 == 0:
            tris += layer
    v9 = np.ascontiguousarray(np.array(tris, dtype=np.float64).reshape(-1, 9))
    argb = (0xFF000000 | (np.arange(v9.shape[0], dtype=np.uint32) * np.uint32(2654435761) & np.uint32(0xFFFFFF))).astype(np.uint32)
    return v9, argb, np.array([-0.5] * 3), np.array([0.5] * 3)


def scene_data(name):
    """((v9, argb, bmin, bmax), extra primitives)."""
    if name == "layers":
        return layers_scene(), ()
    return gbc.scene_data(name)


def sets_of(scene):
    return LAYER_SETS if scene == "layers" else occ.SETS


def _layer_rays():
    """{name: (starts, dirs or end points, endpoints)}: one generator, the sets drawn in the order through, oblique."""
    rng = np.random.default_rng(2024)
    n = 256
    s = np.concatenate([rng.uniform(-0.35, 0.35, size=(n, 2)), np.full((n, 1), -0.48)], axis=1)
    d = np.concatenate([rng.uniform(-0.15, 0.15, size=(n, 2)), np.ones((n, 1))], axis=1) * 0.9
    back = np.arange(n) % 4 == 1
    s[back, 2] = 0.48
    d[back, 2] = -0.9
    a = rng.uniform(-0.4, 0.4, size=(n, 3))
    b = rng.uniform(-0.4, 0.4, size=(n, 3))
    es, ed = [], []
    for x, y in EDGE_POINTS:
        for sign in (1.0, -1.0):
            es.append((x, y, -0.48 * sign))
            ed.append((0.0, 0.0, 0.96 * sign))
    return {"through": (s, d, False), "far_through": (s - 3.0 * d, d, False), "oblique": (a, b, True),
            "edges": (np.array(es, dtype=np.float64), np.array(ed, dtype=np.float64), False)}


class LayerSet:
    """A ray set of "layers", with the attributes of occ.RaySet that the tests read."""

    def __init__(self, name):
        self.scene, self.name = "layers", name
        s, d, self.endpoints = _layer_rays()[name]
        self.starts, self.dirs = np.ascontiguousarray(s), np.ascontiguousarray(d)
        self.kinds = None
        self.n = self.starts.shape[0]
        self.D = occ.directions(self.starts, self.dirs, self.endpoints)
        self.limits = {}

    def regular(self, variant=None):
        return np.ones(self.n, dtype=bool)


_SETS = {}


def ray_set(scene, name):
    if scene != "layers":
        return occ.ray_set(scene, name)
    if name not in _SETS:
        _SETS[name] = LayerSet(name)
    return _SETS[name]


def regular(rs, limits):
    """The library's routing rule for a set under `limits` ([n] or None)."""
    return occ.regular(rs.starts, rs.dirs, rs.endpoints, limits)


def torus_points(n=48, seed=77):
    """(points [2n][3], unit directions [2n][3], inside [2n]) around tests/mesh_cases.py's torus (R 0.3, r 0.12 about the y axis, closed and
    wound outward): n seeded points inside the tube and n outside it, every one at least 0.02 away from the surface, each with a seeded
    direction."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.0, 2.0 * np.pi, size=2 * n)
    v = rng.uniform(0.0, 2.0 * np.pi, size=2 * n)
    rho = np.concatenate([rng.uniform(0.0, 0.09, size=n), rng.uniform(0.15, 0.19, size=n)])      # distance from the tube's centre circle
    ring = 0.3 + rho * np.cos(v)
    p = np.stack([ring * np.cos(u), rho * np.sin(v), ring * np.sin(u)], axis=1)
    d = rng.normal(size=(2 * n, 3))
    d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
    return np.ascontiguousarray(p), np.ascontiguousarray(d), np.arange(2 * n) < n


TORUS_REACH = 2.0            # p + TORUS_REACH * d lies outside the box [-0.5, 0.5]^3 for every point of torus_points()
