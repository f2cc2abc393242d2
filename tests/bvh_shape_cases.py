"""The scenes, frames and ray batches of the adversarial-geometry tests (tests/bvh_shapes.py), with their oracle results.

Shared by tests/test_bvh_shapes_model.py, which settles the oracle side on the CPU, and tests/test_gpu_bvh_shapes.py, which compares the
library with it: every oracle frame and ray batch is computed once per process and handed out unchanged."""
import functools
import os

import numpy as np

import bvh_shapes as bs
from helpers import load_obj3ds, make_frame, orc

NCPU = min(16, os.cpu_count() or 1)
W, H = 96, 80
BACKGROUND = 0xFFFF00FF
TRACE_KEYS = ("hit", "tri_index", "color", "ray_frac", "pos", "normal")
CHAIN_N = 200                                 # accepted: depth 52 (leaf 4) / 54 (leaf 1) from the host builder
CHAIN_REFUSED_N = 400                         # refused: depth 102 / 104
CHAIN_HITTABLE = 29                           # triangles 0 .. 28 of the chain can be hit at all, see chain_hittable()
DEEP_SOUP = dict(n=100, centre=(0.1, -0.35, -0.3), extent=0.3, seed=3)       # behind the chain as the light sees it
DEEP_POSE = dict(yaw_deg=160.0, pitch_deg=-35.0, depth=0.8)
DEEP_LIGHT = (0.0, bs.CHAIN_Y, 1.2)           # model space: the segments from the soup to the light cross z = 0 around the chain's small end
LIMIT_SOUP = dict(n=100, centre=(0.25, 0.1, 0.2), extent=0.3, seed=5)
LIMIT_CORNER = 4
# cluster_staircase(m): steps 0 .. m - 1 and the cluster in the point's own cell, m + 1 clusters of three
WIDE_DEEP_STEPS = 56                          # device-built, one triangle per leaf: depth 60, wide depth 48 (bvh_shapes.wide_depth_model)
WIDE_EDGE_STEPS = 48                          # ... depth 52, wide depth 40: (3 x 40 + 2) x 528 B, the largest packet-walk stack there is
PRIVATE_EDGE_STEPS = 28                       # ... depth 32, wide depth 20: (3 x 20 + 2) x 1 KB, the largest stack of a four-wide private walk
WIDE_LEAF = 1                                 # SR_DBG_BVH_LEAF of both
TIE_POSE = dict()                             # the RendererTests pose


def chain_hittable():
    """The reference replaces a triangle's normal by (1, 0, 0) when every component of (v2 - v1) x (v3 - v1) is below 1e-10
    (Triangle.cs:42-43).  For the chain that product is (0, 0, 0.05 * 2^-k): triangles k >= 29 are such triangles, and neither the
    reference nor the oracle ever reports a hit on them for rays that do not lie in their plane.  They still shape the tree: every
    ray through the point the chain converges to walks all of its levels."""
    k = 0
    while 0.05 * 2.0 ** -k >= 1e-10:
        k += 1
    return k


@functools.lru_cache(maxsize=None)
def limit_staircase_length():
    """The staircase length m (with LIMIT_CORNER key-0 triangles and the soup) for which the device build gives depth 62 = the limit
    with the default leaf size, chosen with the model."""
    extra = np.concatenate([bs.corner_cluster(LIMIT_CORNER), bs.soup(**LIMIT_SOUP)])
    for m in range(bs.STAIRCASE_MAX, 8, -1):
        v9, _, bmin, bmax = bs.morton_staircase(m, extra)
        if bs.lbvh_model(v9, bmin, bmax, 4)[0] == 62:
            return m
    raise AssertionError("no staircase length gives depth 62")


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "deep":
        return bs.shrinking_chain(CHAIN_N, extra=bs.soup(**DEEP_SOUP))
    if name == "chain":
        return bs.shrinking_chain(CHAIN_N)
    if name == "chain_hittable":
        return bs.shrinking_chain(CHAIN_HITTABLE)
    if name == "chain_refused":
        return bs.shrinking_chain(CHAIN_REFUSED_N, extra=bs.soup(**DEEP_SOUP))
    if name == "limit":
        return bs.morton_staircase(limit_staircase_length(), np.concatenate([bs.corner_cluster(LIMIT_CORNER), bs.soup(**LIMIT_SOUP)]))
    if name == "wide_deep":
        return bs.cluster_staircase(WIDE_DEEP_STEPS, extra=bs.soup(**LIMIT_SOUP))
    if name == "wide_edge":
        return bs.cluster_staircase(WIDE_EDGE_STEPS, extra=bs.soup(**LIMIT_SOUP))
    if name == "private_edge":
        return bs.cluster_staircase(PRIVATE_EDGE_STEPS, extra=bs.soup(**LIMIT_SOUP))
    if name == "same_centre":
        return bs.same_centre(300)
    if name == "duplicates":
        return bs.exact_duplicates(150, 4)
    if name == "flat_thin":
        return bs.flat(300)
    if name == "flat_thick":
        return bs.flat(300, thick=True)
    if name == "obj":
        return load_obj3ds()
    raise KeyError(name)


WIDE_STEPS = {"wide_deep": WIDE_DEEP_STEPS, "wide_edge": WIDE_EDGE_STEPS, "private_edge": PRIVATE_EDGE_STEPS}
TIE_SCENES = ("same_centre", "duplicates", "flat_thin", "flat_thick")


@functools.lru_cache(maxsize=None)
def oracle_scene(name):
    o = orc.Scene()
    o.set_triangles(*scene(name))
    assert o.build_tree() == 0, name
    return o


def set_light(f, model_pos):
    t = [f.transform[i] for i in range(12)]
    for r in range(3):
        f.light_pos_view[r] = t[4 * r] * model_pos[0] + t[4 * r + 1] * model_pos[1] + t[4 * r + 2] * model_pos[2] + t[4 * r + 3]
    return f


FRAME_KW = {
    "plain": dict(),
    "sub2": dict(sub_pixel_res=2),
    "focal_blur": dict(focal_blur=True, sub_pixel_res=2),
    "shadows": dict(shadows=True),                                   # the reference's 100 samples
    "shadows_sub2": dict(shadows=True, sub_pixel_res=2, shadow_samples=16),
    "mirror": dict(),                                                # + max_bounces = 1, see frame()
    "rows": dict(start_row=17, end_row=50),
}
DEEP_FRAMES = ("plain", "sub2", "focal_blur", "shadows", "shadows_sub2", "mirror", "rows")
TIE_FRAMES = ("plain", "shadows", "sub2")


def frame(scene_name, frame_name, omode=orc.MODE_NEAREST):
    """The oracle frame (helpers.make_frame); the GPU tests convert it with as_sr."""
    deep = scene_name in ("deep", "chain_refused")
    f = make_frame(W, H, mode=omode, **(DEEP_POSE if deep else TIE_POSE), **FRAME_KW[frame_name])
    if frame_name == "mirror":
        f.max_bounces, f.reflectivity = 1, 0.5
    if deep:
        set_light(f, DEEP_LIGHT)
    return f


@functools.lru_cache(maxsize=None)
def oracle_frame(scene_name, frame_name, omode=orc.MODE_NEAREST):
    want, _ = oracle_scene(scene_name).render(frame(scene_name, frame_name, omode), threads=NCPU)
    want.setflags(write=False)
    return want


def pixel_classes(scene_name):
    """(background, lit, shadowed) pixel counts of the scene's `shadows` frame against its `plain` one.  A lit pixel of a frame with
    shadows is the plain frame's colour modulated once more, at most one step per channel away from it."""
    a, b = oracle_frame(scene_name, "plain"), oracle_frame(scene_name, "shadows")
    bg = a == BACKGROUND
    step = np.max([np.abs(((a >> s) & 0xFF).astype(np.int64) - ((b >> s) & 0xFF).astype(np.int64)) for s in (0, 8, 16)], axis=0)
    return int(bg.sum()), int(((step <= 1) & ~bg).sum()), int(((step > 1) & ~bg).sum())


@functools.lru_cache(maxsize=None)
def ray_batch(scene_name, family):
    v9 = scene(scene_name)[0]
    if scene_name in ("chain", "chain_hittable", "deep"):
        n = min(v9.shape[0], CHAIN_N)                                   # (the chain comes first in `deep`, its soup after it)
        if family == "at_triangles":
            s, d = bs.rays_at_triangles(v9, np.arange(n), 5)
        elif family == "through_point":
            s, d = bs.rays_through_point((0.0, bs.CHAIN_Y, 0.0), 64)
        elif family == "near_miss":
            s, d = bs.rays_missing_by_less_than_the_pad(v9, np.arange(min(n, CHAIN_HITTABLE)), ext=1.25)
        else:
            raise KeyError(family)
    elif scene_name == "limit":
        m = limit_staircase_length()
        if family == "at_triangles":
            s, d = bs.rays_at_triangles(v9, np.arange(m), 3)
        elif family == "through_point":                                 # the middle of a step two thirds down the staircase
            s, d = bs.rays_through_point(0.5 * (v9[m // 3].min(axis=0) + v9[m // 3].max(axis=0)), 64)
        elif family == "near_miss":
            s, d = bs.rays_missing_by_less_than_the_pad(v9, np.arange(m))
        else:
            raise KeyError(family)
    elif scene_name in WIDE_STEPS:
        stairs = np.arange(3 * (WIDE_STEPS[scene_name] + 1))
        if family == "at_triangles":
            s, d = bs.rays_at_triangles(v9, stairs, 3)
        elif family == "through_point":
            s, d = bs.rays_through_point(bs.cluster_point(), 64)
        elif family == "near_miss":
            s, d = bs.rays_missing_by_less_than_the_pad(v9, stairs)
        else:
            raise KeyError(family)
    elif scene_name == "duplicates" and family == "at_triangles":
        s, d = bs.rays_at_triangles(v9, np.arange(0, v9.shape[0], 2), 3)
    else:
        raise KeyError((scene_name, family))
    s = np.ascontiguousarray(s); d = np.ascontiguousarray(d)
    s.setflags(write=False); d.setflags(write=False)
    return s, d


RAY_FAMILIES = ("at_triangles", "through_point", "near_miss")
ORC_TARGET = {"brute": 0, "tree": 1, "nearest": 3}


@functools.lru_cache(maxsize=None)
def oracle_trace(scene_name, family, target="nearest"):
    s, d = ray_batch(scene_name, family)
    res = oracle_scene(scene_name).trace(ORC_TARGET[target], s, d)
    for a in res.values():
        a.setflags(write=False)
    return res
