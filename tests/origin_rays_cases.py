"""Scenes, origins and direction sets of the origin-ray tests (tests/test_gpu_origin_rays.py), shared with tests/test_origin_rays_model.py,
which checks on the CPU -- with the oracle -- that between 10 % and 90 % of the regular rays of every case hit and that the sets meant to
exercise irregular rays hold every kind of them.

Scenes (tests/gbuffer_cases.py): "small", 48 large triangles (at most 64: the own BVH is built on the host); "cube", unit_cube_scene(2000),
device-built, traced alone and -- SR_TARGET_ROOT -- with its extra primitives (a plane, a sphere and a box outside the root box).
Origins: "out" outside the root box's slab on all three axes, "one" outside on exactly one, "centre" the box centre, "plane" a point on the
plane of a model triangle inside its outline, "far" 2.5e5 box extents away along the diagonal.
Direction sets, aimed at the box where that makes sense: "grid" a 24x20 pinhole grid in scan order, "tiles" the same in 8x8-tile-major order,
"sphere" a 64x32 equirectangular full sphere (rays pointing away, exact axis directions, zero components of both signs), "shuffled" a seeded
permutation of it, "n1" .. "n449" 1, 63, 64, 65, 64 * 7 + 1 consecutive grid rays around the image centre, "irregular" the sphere with an irregular direction in every
eighth position."""
import numpy as np

import gbuffer_cases as gbc

SCENES = ("small", "cube")
ORIGINS = ("out", "one", "centre", "plane", "far")
SETS = ("grid", "tiles", "sphere", "shuffled", "n1", "n63", "n64", "n65", "n449", "irregular")
GRID_W, GRID_H = 24, 20
# the kinds of irregular direction: the zero vector, a NaN component, +inf, -inf, a regular direction x 1e300 and x 1e-300; the two scalings
# at the edge of the regular range stay regular
IRREGULAR_KINDS = ("zero", "nan", "+inf", "-inf", "x1e300", "x1e-300")
EDGE_KINDS = ("x2^40", "x2^-40")


def box(scene):
    tris, _ = gbc.scene_data(scene)
    return np.asarray(tris[2], dtype=np.float64), np.asarray(tris[3], dtype=np.float64)


def plane_point(scene):
    """A point of the plane of the model triangle nearest the box centre, inside its outline (the centroid, by more than rounding)."""
    v9 = np.asarray(gbc.scene_data(scene)[0][0], dtype=np.float64).reshape(-1, 3, 3)
    lo, hi = box(scene)
    cen = v9.mean(axis=1)
    area = np.linalg.norm(np.cross(v9[:, 1] - v9[:, 0], v9[:, 2] - v9[:, 0]), axis=1)
    ok = area > 0.25 * np.median(area)
    k = int(np.argmin(np.where(ok, ((cen - 0.5 * (lo + hi)) ** 2).sum(axis=1), np.inf)))
    return cen[k].copy()


def origin_of(scene, name):
    lo, hi = box(scene)
    c, e = 0.5 * (lo + hi), hi - lo
    if name == "out":
        return c + e * np.array([0.8, 0.7, -0.9])
    if name == "one":
        return c + e * np.array([0.21, -0.75, 0.13])
    if name == "centre":
        return c.copy()
    if name == "plane":
        return plane_point(scene)
    if name == "far":
        return c + 2.5e5 * e * np.array([1.0, 1.0, -1.0])
    raise KeyError(name)


def aim(scene, name):
    """(forward, right, up, half width of the image plane at distance 1) of the pinhole grid: looking at the box centre, or -- from
    inside the box -- along a fixed skew axis with a wide field."""
    lo, hi = box(scene)
    c, e = 0.5 * (lo + hi), hi - lo
    o = origin_of(scene, name)
    fwd = c - o
    dist = float(np.linalg.norm(fwd))
    inside = bool(np.all(o > lo) and np.all(o < hi))
    if inside or dist < 1e-6 * float(np.linalg.norm(e)):
        fwd, half = np.array([-1.0, -0.3, 0.4]), 1.2
    else:
        half = 0.45 * float(np.linalg.norm(e)) / dist                      # most of the box's bounding sphere: hits and misses
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(fwd, np.array([0.0, 1.0, 0.0]) if abs(fwd[1]) < 0.9 else np.array([1.0, 0.0, 0.0]))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    return fwd, right, up, half


def grid_dirs(scene, origin, w=GRID_W, h=GRID_H):
    """w x h pinhole rays in scan order, not normalised: 1.7 long on the axis, or -- from an origin further away than a ray of that length
    reaches (a ray ends 10000 |d| from its start) -- a hundredth of the distance to the box centre."""
    fwd, right, up, half = aim(scene, origin)
    lo, hi = box(scene)
    scale = max(1.7, float(np.linalg.norm(0.5 * (lo + hi) - origin_of(scene, origin))) / 100.0)
    rows, cols = np.mgrid[0:h, 0:w]
    x = ((cols + 0.5) / w - 0.5) * 2.0 * half
    y = -((rows + 0.5) / h - 0.5) * 2.0 * half * (h / w)
    return np.ascontiguousarray((fwd[None, :] + x.reshape(-1, 1) * right[None, :] + y.reshape(-1, 1) * up[None, :]) * scale)


def tile_order():
    """Scan-order indices of the grid's pixels in 8x8-tile-major order (tiles row by row, a tile's pixels row by row; edge tiles are cut)."""
    idx = []
    for ty in range(0, GRID_H, 8):
        for tx in range(0, GRID_W, 8):
            for y in range(ty, min(ty + 8, GRID_H)):
                for x in range(tx, min(tx + 8, GRID_W)):
                    idx.append(y * GRID_W + x)
    return np.array(idx, dtype=np.int64)


def sphere_for(scene, origin):
    """The full sphere -- or, from the "far" origin, where no ray of a full sphere comes near the box (it subtends a millionth of a radian) and
    a unit direction does not reach it, a 64 x 32 pinhole window on the box in its place."""
    return grid_dirs(scene, origin, 64, 32) if origin == "far" else sphere_dirs()


def sphere_dirs():
    """64 x 32 equirectangular directions: longitudes k * 2 pi / 64 snapped to exact axis values where they fall on one, latitudes from pole to
    pole inclusive with the equator among them -- so the set holds +-x, +-y, +-z exactly and components that are 0.0 and -0.0."""
    lon = np.arange(64) * (2.0 * np.pi / 64)
    lat = (np.arange(32) - 16) * (np.pi / 32)                               # -90 deg .. in steps of 5.625: row 16 is the equator
    lat[31] = 0.5 * np.pi                                                    # ... and the last row the other pole
    cl, sl = np.cos(lat), np.sin(lat)
    cx, sx = np.cos(lon), np.sin(lon)
    for a in (cl, sl, cx, sx):
        a[np.abs(a) < 1e-12] = 0.0
        a[np.abs(a - 1.0) < 1e-12] = 1.0
        a[np.abs(a + 1.0) < 1e-12] = -1.0
    d = np.stack([np.outer(cl, cx), np.outer(sl, np.ones(64)), np.outer(cl, sx)], axis=-1).reshape(-1, 3)
    for k in range(3):                                                       # the zero components alternate in sign: 0.0 and -0.0
        z = d[:, k] == 0.0
        d[z, k] = np.where(np.arange(int(z.sum())) % 2 == 0, 0.0, -0.0)
    return np.ascontiguousarray(d)


def irregular_dirs(scene="cube", origin="out"):
    """The sphere set with position 8 k replaced, kinds in turn; returns (dirs, kind per ray or "")."""
    d = sphere_for(scene, origin).copy()
    kinds = [""] * d.shape[0]
    allk = IRREGULAR_KINDS + EDGE_KINDS
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for j, i in enumerate(range(0, d.shape[0], 8)):
            kind = allk[j % len(allk)]
            base = d[i + 3] / np.abs(d[i + 3]).max()                         # a regular neighbour, largest component 1
            if kind == "zero":
                d[i] = 0.0
            elif kind == "nan":
                d[i] = base
                d[i, j % 3] = np.nan
            elif kind == "+inf":
                d[i] = base
                d[i, j % 3] = np.inf
            elif kind == "-inf":
                d[i] = base
                d[i, j % 3] = -np.inf
            elif kind == "x1e300":
                d[i] = base * 1e300
            elif kind == "x1e-300":
                d[i] = base * 1e-300
            elif kind == "x2^40":
                d[i] = base * 2.0 ** 40
            else:
                d[i] = base * 2.0 ** -40
            kinds[i] = kind
    return np.ascontiguousarray(d), kinds


def regular(dirs):
    """The library's definition (include/softray.h): finite components and 2^-40 <= max |d_k| <= 2^40."""
    with np.errstate(invalid="ignore"):
        m = np.abs(dirs).max(axis=1)
        return np.isfinite(dirs).all(axis=1) & (m >= 2.0 ** -40) & (m <= 2.0 ** 40)


def dirs_of(scene, origin, name):
    if name == "grid":
        return grid_dirs(scene, origin)
    if name == "tiles":
        return np.ascontiguousarray(grid_dirs(scene, origin)[tile_order()])
    if name == "sphere":
        return sphere_for(scene, origin)
    if name == "shuffled":
        return np.ascontiguousarray(sphere_for(scene, origin)[np.random.default_rng(20260).permutation(64 * 32)])
    if name == "irregular":
        return irregular_dirs(scene, origin)[0]
    if name.startswith("n"):
        n = int(name[1:])
        first = (GRID_W * GRID_H - n) // 2                                   # a run of scan order around the image centre
        return np.ascontiguousarray(grid_dirs(scene, origin)[first:first + n])
    raise KeyError(name)


def coherent_ok(name):
    """Sets whose order allows the caller's promise (results never depend on it: the tests pass it for every set)."""
    return name in ("tiles",)


def facing(scene, origin, dirs):
    """Rays that do not point away from the box: the half-line from the origin along the direction meets the root box (slab test; an
    origin inside the box: every ray)."""
    lo, hi = box(scene)
    o = origin_of(scene, origin)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inv = 1.0 / dirs
        t0, t1 = (lo - o) * inv, (hi - o) * inv
        near, far = np.minimum(t0, t1), np.maximum(t0, t1)
        # (a zero component: the ray stays between the planes of that axis, or never gets there)
        zero = dirs == 0.0
        between = (o >= lo) & (o <= hi)
        near = np.where(zero, np.where(between, -np.inf, np.inf), near)
        far = np.where(zero, np.where(between, np.inf, -np.inf), far)
        return (near.max(axis=1) <= far.min(axis=1)) & (far.min(axis=1) >= 0.0)


def oracle_trace(tree, brute, mode, root, prims, origin, dirs):
    """The oracle's answer for rays from `origin`, with the target mapping of tests/test_gpu_gbuffer.py: mode "tree" / "brute" / "bvh", alone or
    (root) with the extra geometry."""
    import pathtrace_model as ptm
    starts = np.ascontiguousarray(np.tile(np.asarray(origin, dtype=np.float64), (dirs.shape[0], 1)))
    if mode == "tree":
        return tree.trace(ptm.TRACE_ROOT_TREE if root else 1, starts, dirs)
    if mode == "brute":
        return brute.trace(ptm.TRACE_ROOT_TREE if root else 0, starts, dirs)
    near = tree.trace(ptm.TRACE_NEAREST, starts, dirs)
    if not (root and prims):
        return near
    # the oracle's nearest-hit target knows no extra geometry: where its answer for the model alone is the tree's, the tree's root geometry
    # is the own BVH's too -- and only then
    alone = tree.trace(1, starts, dirs)
    for k in ("hit", "ray_frac", "pos", "normal", "color", "tri_index"):
        a, b = np.ascontiguousarray(alone[k]), np.ascontiguousarray(near[k])
        if a.tobytes() != b.tobytes():
            return None
    return tree.trace(ptm.TRACE_ROOT_TREE, starts, dirs)
