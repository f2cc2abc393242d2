"""The packet walks keep their lane predicates as wave masks in scalar registers (vote helpers, sr_device.h).  These frames aim at the
places where such a mask differs from "all lanes": tiles with invalid lanes (a frame whose width and height are no multiples of 16, tiles
that straddle the silhouette), candidate lists that fill up (SR_DBG_ROUND_CAP0 = 2: nearly every lane of a shadowed tile overflows and
leaves the walk early; = 40: the default length), and lanes that an umbra triangle takes out of the walk while their neighbours go on.
The frame is as large as the ones of test_random_large_frame_on_the_persistent_shaft_walk, so that the persistent tile feed runs.

Every variant -- list length x first shaft round as packet walk / private per-lane walks x primary rays as packet walk / private walks --
must equal the oracle's frame in every pixel, with the light inside the root box (the KNOWN == 0 instantiation of k_shaft_pkt4) and
outside it on all three axes (KNOWN == 7).
"""
import functools
import itertools
import os

import numpy as np
import pytest

import softray_amd as sa
from helpers import make_frame, orc, random_triangles

pytestmark = pytest.mark.gpu
NCPU = os.cpu_count() or 8
WIDTH, HEIGHT = 523, 381                       # 32 x 23 tiles of 16 x 16 with a partial last column and row
N_TRIS, EXTENT, SEED = 6000, 0.05, 9021
# model-space light positions; the scene's root box is [-0.5, 0.5]^3
LIGHTS = {"inside": (0.25, -0.3, 0.2), "outside": (1.2, -1.1, 1.2)}


def scene_arrays():
    v9, argb, _ = random_triangles(N_TRIS, SEED, space=1.0 - EXTENT, extent=EXTENT, origin=-0.5, mask_color=True)
    return v9, argb, np.array([-0.5] * 3), np.array([0.5] * 3)


def frame_with_light(model):
    f = make_frame(WIDTH, HEIGHT, shading=True, shadows=True, sub_pixel_res=1, yaw_deg=135.0, pitch_deg=-22.0, roll_deg=0.0, depth=1.3,
                   point_light=True, specular=True, shadow_samples=33)
    f.random_seed = 20240521
    t = [f.transform[i] for i in range(12)]
    for r in range(3):
        f.light_pos_view[r] = t[4 * r] * model[0] + t[4 * r + 1] * model[1] + t[4 * r + 2] * model[2] + t[4 * r + 3]
    return f


@functools.lru_cache(maxsize=None)
def oracle_frame(light):
    v9, argb, lo, hi = scene_arrays()
    o = orc.Scene()
    o.set_triangles(v9, argb, lo, hi)
    assert o.build_tree() == 0
    want = np.zeros(WIDTH * HEIGHT, dtype=np.int32)
    o.render(frame_with_light(LIGHTS[light]), threads=NCPU, out=want)
    return want.view(np.uint32).ravel()


@functools.lru_cache(maxsize=None)
def gpu_scene():
    v9, argb, lo, hi = scene_arrays()
    g = sa.GpuScene(0)
    g.set_triangles(v9, argb, lo, hi)
    g.debug_set(sa._lib.DBG_BVH_LEAF, 4)
    g.build((sa.MODE_BVH,), on_device=True)
    return g


@pytest.mark.parametrize("light", sorted(LIGHTS))
def test_oracle_frame_has_lit_shadowed_and_background_pixels(light):
    """The frames are worth testing: background (tiles with invalid lanes), fully shadowed and fully lit pixels all occur in numbers."""
    want = oracle_frame(light)
    f = frame_with_light(LIGHTS[light])
    background = int(np.count_nonzero(want == np.uint32(0xFF000000 | f.background_argb)))
    black = int(np.count_nonzero((want & np.uint32(0xFFFFFF)) == 0))
    assert 0.1 * want.size < background < 0.6 * want.size, background       # tiles that straddle the silhouette: invalid lanes
    assert black > 1000, black                                               # fully shadowed surface points: umbra lanes
    assert len(np.unique(want)) > 1000


@pytest.mark.parametrize("per_lane_primary", [0, 1])
@pytest.mark.parametrize("per_lane_shaft", [0, 1])
@pytest.mark.parametrize("cap0", [2, 40])
@pytest.mark.parametrize("light", sorted(LIGHTS))
def test_every_pixel_equals_the_oracle(light, cap0, per_lane_shaft, per_lane_primary):
    want = oracle_frame(light)
    g = gpu_scene()
    fs = sa.Frame.from_buffer_copy(bytes(frame_with_light(LIGHTS[light])))
    fs.trace_mode = sa.MODE_BVH
    g.debug_set(sa._lib.DBG_KERNEL_SWITCH, 831)             # one workgroup per CU: the waves pull their tiles from the per-XCD lists
    g.debug_set(sa._lib.DBG_ROUND_CAP0, cap0)
    g.debug_set(sa._lib.DBG_PER_LANE_SHAFT, per_lane_shaft)
    g.debug_set(sa._lib.DBG_PER_LANE_PRIMARY, per_lane_primary)
    try:
        for turn in range(2):                                # the second frame walks the tiles longest first (k_tile_order)
            got, _ = g.render(fs)
            got = np.asarray(got).view(np.uint32).ravel()
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "frame %d: %d pixels differ (first %s)" % (turn, bad.size, bad[:5])
    finally:
        for key in (sa._lib.DBG_KERNEL_SWITCH, sa._lib.DBG_ROUND_CAP0, sa._lib.DBG_PER_LANE_SHAFT, sa._lib.DBG_PER_LANE_PRIMARY):
            g.debug_set(key, -1)
