"""k_shaft_pkt4 filters its triangles with the frame's penumbra planes (LightCone records, k_light_cones) instead of rebuilding the edge
terms per surface point from the TriSlab records.  The frames are those of test_gpu_vote_paths.py -- partial tiles, silhouette tiles, umbra
lanes, lists that overflow -- with lights chosen for the record's classes: a ball among the triangles (many planes pass within its radius:
the always-pass records), a light outside the box on three axes and on one, a light 0.01 from a box face, and a single sample with a zero
offset (R = 0: inner and outer planes coincide).  Every variant -- list length 2 / 40 x {penumbra planes on the persistent tile feed,
penumbra planes with one workgroup per tile, the TriSlab filter (SR_DBG_KERNEL_SWITCH 96)} -- must equal the oracle in every pixel.

The sequence renders light A, light B, light A again and then moves the camera with the light unchanged (the facing partition re-runs and
moves the records the planes belong to): the records must follow the light and the record order."""
import functools
import os

import numpy as np
import pytest

import softray_amd as sa
from helpers import make_frame, orc, random_triangles

pytestmark = pytest.mark.gpu
NCPU = os.cpu_count() or 8
WIDTH, HEIGHT = 523, 381                       # 32 x 23 tiles of 16 x 16 with a partial last column and row
N_TRIS, EXTENT, SEED = 6000, 0.05, 9021
TRISLAB_FILTER = 96                            # SR_DBG_KERNEL_SWITCH: the packet shaft walk filters with the TriSlab records
# name: (model-space light position, radius the offset table is scaled to or None for the table as it is, shadow samples); the root box is [-0.5, 0.5]^3
LIGHTS = {
    "inside_r008": ((0.25, -0.3, 0.2), 0.08, 33),
    "outside_three_axes": ((1.2, -1.1, 1.2), None, 33),
    "outside_one_axis": ((0.1, 0.2, 1.3), None, 33),
    "near_a_face": ((0.15, -0.2, 0.51), None, 33),
    "one_sample_zero_offset": ((0.6, -0.7, 0.9), 0.0, 1),
}
POSES = {"front": (135.0, -22.0), "moved": (100.0, 15.0)}


@functools.lru_cache(maxsize=None)
def offset_table(radius, samples):
    """The reference's table scaled to `radius` (helpers.edge_light_case); radius 0 with one sample: a single zero offset.  Cached: frames point at it."""
    if radius == 0.0:
        return np.zeros((samples, 3), dtype=np.float64)
    table = orc.area_light_offsets(1234567890, samples)
    return np.ascontiguousarray(table * (radius / np.sqrt((table * table).sum(axis=1)).max()))


def scene_arrays():
    v9, argb, _ = random_triangles(N_TRIS, SEED, space=1.0 - EXTENT, extent=EXTENT, origin=-0.5, mask_color=True)
    return v9, argb, np.array([-0.5] * 3), np.array([0.5] * 3)


def frame_with_light(light, pose="front"):
    model, radius, samples = LIGHTS[light]
    yaw, pitch = POSES[pose]
    f = make_frame(WIDTH, HEIGHT, shading=True, shadows=True, sub_pixel_res=1, yaw_deg=yaw, pitch_deg=pitch, roll_deg=0.0, depth=1.3,
                   point_light=True, specular=True, shadow_samples=samples)
    f.random_seed = 20240521
    t = [f.transform[i] for i in range(12)]
    for r in range(3):
        f.light_pos_view[r] = t[4 * r] * model[0] + t[4 * r + 1] * model[1] + t[4 * r + 2] * model[2] + t[4 * r + 3]
    if radius is not None:
        f.area_light_offsets = offset_table(radius, samples).ctypes.data
    return f


@functools.lru_cache(maxsize=None)
def oracle_frame(light, pose="front"):
    if light == "outside_three_axes" and pose == "front":
        import test_gpu_vote_paths                        # the same frame: rendered once for both files
        return test_gpu_vote_paths.oracle_frame("outside")
    v9, argb, lo, hi = scene_arrays()
    o = orc.Scene()
    o.set_triangles(v9, argb, lo, hi)
    assert o.build_tree() == 0
    want = np.zeros(WIDTH * HEIGHT, dtype=np.int32)
    o.render(frame_with_light(light, pose), threads=NCPU, out=want)
    return want.view(np.uint32).ravel()


@functools.lru_cache(maxsize=None)
def gpu_scene():
    v9, argb, lo, hi = scene_arrays()
    g = sa.GpuScene(0)
    g.set_triangles(v9, argb, lo, hi)
    g.debug_set(sa._lib.DBG_BVH_LEAF, 4)
    g.build((sa.MODE_BVH,), on_device=True)
    return g


def gpu_frame(g, light, pose="front"):
    fs = sa.Frame.from_buffer_copy(bytes(frame_with_light(light, pose)))
    fs.trace_mode = sa.MODE_BVH
    got, _ = g.render(fs)
    return np.asarray(got).view(np.uint32).ravel()


@pytest.mark.parametrize("light", sorted(LIGHTS))
def test_oracle_frame_has_lit_shadowed_and_background_pixels(light):
    """The frames are worth testing: background (tiles with invalid lanes), fully shadowed and fully lit pixels all occur in numbers."""
    want = oracle_frame(light)
    f = frame_with_light(light)
    background = int(np.count_nonzero(want == np.uint32(0xFF000000 | f.background_argb)))
    black = int(np.count_nonzero((want & np.uint32(0xFFFFFF)) == 0))
    assert 0.1 * want.size < background < 0.6 * want.size, background       # tiles that straddle the silhouette: invalid lanes
    assert black > 1000, black                                               # fully shadowed surface points: umbra lanes
    assert len(np.unique(want)) > 1000


@pytest.mark.parametrize("switch", [831, 0, TRISLAB_FILTER], ids=["planes_persistent", "planes_direct", "trislab"])
@pytest.mark.parametrize("cap0", [2, 40])
@pytest.mark.parametrize("light", sorted(LIGHTS))
def test_every_pixel_equals_the_oracle(light, cap0, switch):
    want = oracle_frame(light)
    g = gpu_scene()
    g.debug_set(sa._lib.DBG_KERNEL_SWITCH, switch)          # 831: one workgroup per CU, the waves pull their tiles from the per-XCD lists
    g.debug_set(sa._lib.DBG_ROUND_CAP0, cap0)
    try:
        for turn in range(2):                                # the second frame reuses the records (and walks the tiles longest first)
            got = gpu_frame(g, light)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "frame %d: %d pixels differ (first %s)" % (turn, bad.size, bad[:5])
    finally:
        for key in (sa._lib.DBG_KERNEL_SWITCH, sa._lib.DBG_ROUND_CAP0):
            g.debug_set(key, -1)


def test_records_follow_the_light_and_the_record_order():
    """One scene, one scratch set: light A, light B, A again, then another camera pose with light A (k_facing_partition moves the records)."""
    g = gpu_scene()
    a, b = "outside_three_axes", "inside_r008"
    for step, (light, pose) in enumerate([(a, "front"), (b, "front"), (a, "front"), (a, "moved")]):
        want = oracle_frame(light, pose)
        got = gpu_frame(g, light, pose)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "step %d (%s, %s): %d pixels differ (first %s)" % (step, light, pose, bad.size, bad[:5])
