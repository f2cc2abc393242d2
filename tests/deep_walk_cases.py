"""Inputs of tests/test_gpu_deep_walks.py: every walk of the library on the deep trees of tests/bvh_shape_cases.py.

Per scene one ray batch (the scene's three ray families, and for the cluster staircases the rays that see the steps from behind), two
origins with their directions, a set of points for sr_closest_points and a set of surface points (hits of the batch) for the point
calls.  Everything is computed once per process from the oracle and handed out unchanged; tests/test_deep_walk_cases.py checks on the
CPU that no case is vacuous."""
import functools

import numpy as np

import bvh_shape_cases as bsc
import bvh_shapes as bs
import occluded_rays_cases as occ
from helpers import make_frame

# scene -> (SR_DBG_BVH_LEAF or None, built on the device)
SCENES = {"chain": (1, False), "deep": (1, False), "limit": (None, True), "private_edge": (bsc.WIDE_LEAF, True), "wide_edge": (bsc.WIDE_LEAF, True),
          "wide_deep": (bsc.WIDE_LEAF, True)}
ORIGINS = {"outside": (1.3, 0.9, 1.7), "inside": (0.05, 0.21, 0.31)}        # outside the box on all axes / inside it
POINTS = 512
W, H = 64, 48
TRACE_NEAREST = 3
SHADOW_SAMPLES = 16


def readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def rays_from_behind(scene_name, count=1024):
    """Rays through the point of a cluster staircase whose directions have a positive product with both normals of its steps: the
    steps are one-sided, so these rays hit none of them and walk every level."""
    v9 = bsc.scene(scene_name)[0]
    normals = [np.cross(v9[k, 1] - v9[k, 0], v9[k, 2] - v9[k, 0]) for k in (0, 3)]
    s, d = bs.rays_through_point(bs.cluster_point(), count)
    keep = np.ones(count, dtype=bool)
    for n in normals:
        keep &= (d @ n) / (np.linalg.norm(n) * 6.0) > 0.1
    return s[keep], d[keep]


def rays_through_pairs(tris, per=4):
    """Rays through the centroids of two triangles each, from three times their distance before the first."""
    c = tris.mean(axis=1)
    n = c.shape[0]
    i = np.repeat(np.arange(n), per)
    j = (i * 7 + 3 + 11 * np.tile(np.arange(per), n)) % n
    keep = i != j
    a, b = c[i[keep]], c[j[keep]]
    return a - (b - a) * 3.0, (b - a) * 8.0


@functools.lru_cache(maxsize=None)
def ray_batch(scene_name):
    parts = [bsc.ray_batch(scene_name, family) for family in bsc.RAY_FAMILIES]
    if scene_name in bsc.WIDE_STEPS:
        parts.append(rays_from_behind(scene_name))
    if scene_name != "chain":                                           # the soup of the frames: the last 100 triangles
        v9 = bsc.scene(scene_name)[0]
        parts.append(bs.rays_at_triangles(v9, np.arange(v9.shape[0] - 100, v9.shape[0]), 3))
        parts.append(rays_through_pairs(v9[-100:]))                    # ... and rays through two of its triangles: more than one hit
    s = np.ascontiguousarray(np.concatenate([p[0] for p in parts]))
    d = np.ascontiguousarray(np.concatenate([p[1] for p in parts]))
    assert s.shape[0] <= 4096
    return readonly(s, d)


@functools.lru_cache(maxsize=None)
def oracle_batch(scene_name):
    res = bsc.oracle_scene(scene_name).trace(TRACE_NEAREST, *ray_batch(scene_name))
    readonly(*res.values())
    return res


@functools.lru_cache(maxsize=None)
def batch_limits(scene_name):
    res = oracle_batch(scene_name)
    return readonly(occ.rotated_limits(np.where(res["hit"].astype(bool), res["ray_frac"], 1.0)))


@functools.lru_cache(maxsize=None)
def origin_dirs(scene_name, origin_name):
    """Directions from the origin to the points the batch's rays aim at (the end of their direction vector), and a spiral of 256 over
    the sphere."""
    s, d = ray_batch(scene_name)
    o = np.array(ORIGINS[origin_name])
    return readonly(np.ascontiguousarray(np.concatenate([s + d - o, bs.rays_through_point((0.0, 0.0, 0.0), 256)[1]])))


@functools.lru_cache(maxsize=None)
def oracle_origin(scene_name, origin_name):
    dirs = origin_dirs(scene_name, origin_name)
    res = bsc.oracle_scene(scene_name).trace(TRACE_NEAREST, np.ascontiguousarray(np.tile(np.array(ORIGINS[origin_name]), (dirs.shape[0], 1))), dirs)
    readonly(*res.values())
    return res


@functools.lru_cache(maxsize=None)
def closest_points(scene_name):
    """POINTS points: a third anywhere in the box (and a little outside it), a third near the triangles of the deep part of the tree,
    a third on the rays through the point the tree converges to."""
    v9, _, bmin, bmax = bsc.scene(scene_name)
    r = np.random.RandomState(4100 + list(SCENES).index(scene_name))
    k = POINTS // 3
    anywhere = bmin + (r.random_sample((k, 3)) * 1.2 - 0.1) * (bmax - bmin)
    tri = r.randint(0, v9.shape[0], k)
    w = r.dirichlet((1.0, 1.0, 1.0), k)
    size = (v9[tri].max(axis=1) - v9[tri].min(axis=1)).max(axis=1)
    near = np.einsum("pk,pkc->pc", w, v9[tri]) + (r.random_sample((k, 3)) - 0.5) * size[:, None]
    s, d = bsc.ray_batch(scene_name, "through_point")
    on_rays = s[np.arange(POINTS - 2 * k) % s.shape[0]] + d[np.arange(POINTS - 2 * k) % s.shape[0]] * (0.5 + (r.random_sample((POINTS - 2 * k, 1)) - 0.5) * 0.2)
    return readonly(np.ascontiguousarray(np.concatenate([anywhere, near, on_rays])))


@functools.lru_cache(maxsize=None)
def surface_points(scene_name):
    """(pos, normal, color) of the batch's hits and of the camera samples of the scene's frame: hit points and normals of rays at the
    triangles, rays through the point and the soup's."""
    import pathtrace_model as ptm
    a = oracle_batch(scene_name)
    b = bsc.oracle_scene(scene_name).trace(TRACE_NEAREST, *ptm.camera_samples(frame(scene_name)))
    ha, hb = a["hit"].astype(bool), b["hit"].astype(bool)
    pos = np.ascontiguousarray(np.concatenate([a["pos"][ha], b["pos"][hb]])[:4096])
    nrm = np.ascontiguousarray(np.concatenate([a["normal"][ha], b["normal"][hb]])[:4096])
    col = np.ascontiguousarray(np.concatenate([a["color"][ha], b["color"][hb]])[:4096])
    return readonly(pos, nrm, col)


def frame(scene_name, **kw):
    """A small frame of the scene with its pose and light (bvh_shape_cases.frame's), 64 x 48."""
    deep = scene_name == "deep"
    f = make_frame(W, H, **(bsc.DEEP_POSE if deep else bsc.TIE_POSE), **kw)
    if deep:
        bsc.set_light(f, bsc.DEEP_LIGHT)
    return f


def share(mask):
    mask = np.asarray(mask, dtype=bool)
    return float(mask.sum()) / max(1, mask.size)
