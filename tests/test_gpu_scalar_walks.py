"""The packet walks after their scalar diet (profiles/r10_scalar_walks): same lanes, same verdicts, same pixels.

Every case renders one frame TWICE on one scene -- the second frame of a persistent launch walks with the umbra hints and the tile
order the first one left -- and compares both frames, pixel for pixel, with the oracle on the CPU and with the same two frames under
the switch that keeps the shaft walk's loop as it was (SR_DBG_KERNEL_SWITCH 63; 631 = that loop on the persistent grid of hook 831).

Covered: a seeded soup of 3 000 triangles with 17 shadow samples at 512 x 384 (the persistent tile grids, hook 831) and at 200 x 160
(one workgroup per tile); the light inside the root box's slab on 0, 1, 2 and 3 axes (the KNOWN instantiations of the shaft walk); the
camera outside the slab on every axis and inside it on two (the (near, far) and the (lo, hi) form of the primary walk); and the slots
of a four-wide node the diet touches: a node whose four children are all leaves, nodes with fewer than four children (three triangles;
a chain of shrinking triangles, whose tree is a path).
"""
import os

import numpy as np
import pytest

import bvh_shapes as bs
import softray_amd as sa
from helpers import make_frame, orc, random_triangles

pytestmark = pytest.mark.gpu
NCPU = min(16, os.cpu_count() or 8)
OLD_LOOP, PERSISTENT, OLD_LOOP_PERSISTENT = 63, 831, 631
SAMPLES = 17
BIG, SMALL = (512, 384), (200, 160)
# camera poses (yaw, pitch, depth): outside the root box's slab on all three axes / inside it on x and y
CAM_OUTSIDE, CAM_INSIDE = (135.0, -35.0, 1.3), (0.0, 0.0, 1.3)


def soup_scene():
    v9, argb, _ = random_triangles(3000, 4243, space=0.92, extent=0.08, origin=-0.5, mask_color=True)
    return v9, argb, np.array([-0.5] * 3), np.array([0.5] * 3)


def frame_with_light(res, cam, outside_mask, model_light=None):
    """The frame; the point light at a model-space position outside the box's slab on the axes of `outside_mask`, inside it on the others."""
    f = make_frame(res[0], res[1], shading=True, shadows=True, sub_pixel_res=1, yaw_deg=cam[0], pitch_deg=cam[1], roll_deg=0.0, depth=cam[2],
                   point_light=True, specular=True, shadow_samples=SAMPLES)
    f.random_seed = 20241
    if model_light is None:
        model_light = [(1.2 if a != 1 else -1.1) if (outside_mask >> a) & 1 else (0.25 if a != 2 else -0.3) for a in range(3)]
    t = [f.transform[i] for i in range(12)]
    for r in range(3):
        f.light_pos_view[r] = t[4 * r] * model_light[0] + t[4 * r + 1] * model_light[1] + t[4 * r + 2] * model_light[2] + t[4 * r + 3]
    return f


def gpu_frames(scene, f, leaf, switch):
    v9, argb, lo, hi = scene
    g = sa.GpuScene(0)
    g.set_triangles(v9, argb, lo, hi)
    g.debug_set(sa._lib.DBG_BVH_LEAF, leaf)
    g.build((sa.MODE_BVH,), on_device=True)
    if switch:
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, switch)
    fs = sa.Frame.from_buffer_copy(bytes(f))
    fs.trace_mode = sa.MODE_BVH
    return [np.asarray(g.render(fs)[0]).view(np.uint32).ravel().copy() for _ in range(2)]


def check(scene, f, leaf, persistent):
    v9, argb, lo, hi = scene
    o = orc.Scene()
    o.set_triangles(v9, argb, lo, hi)
    assert o.build_tree() == 0
    want = np.zeros(f.width * f.height, dtype=np.int32)
    o.render(f, threads=NCPU, out=want)
    want = want.view(np.uint32)
    new = gpu_frames(scene, f, leaf, PERSISTENT if persistent else 0)
    old = gpu_frames(scene, f, leaf, OLD_LOOP_PERSISTENT if persistent else OLD_LOOP)
    for k in range(2):
        bad = np.flatnonzero(new[k] != want)
        assert bad.size == 0, "frame %d: %d pixels differ from the oracle (first %s)" % (k, bad.size, bad[:5])
        bad = np.flatnonzero(new[k] != old[k])
        assert bad.size == 0, "frame %d: %d pixels differ from the loop as it was (first %s)" % (k, bad.size, bad[:5])
    assert np.unique(want).size >= 2                                   # a frame with a model in it, not the background alone


@pytest.mark.parametrize("res", [BIG, SMALL], ids=["persistent", "direct"])
@pytest.mark.parametrize("outside_mask", [7, 3, 1, 0])
def test_soup_with_the_light_inside_the_slab_on_0_to_3_axes(res, outside_mask):
    cam = CAM_OUTSIDE if outside_mask in (7, 1) else CAM_INSIDE
    check(soup_scene(), frame_with_light(res, cam, outside_mask), 4, res == BIG)


@pytest.mark.parametrize("shape", ["four_leaves", "three_children", "path"])
def test_nodes_with_leaf_children_only_and_with_fewer_than_four_children(shape):
    if shape == "four_leaves":                                         # four triangles, one per leaf: the root's four children are all leaves
        scene, leaf = (bs.soup(4, (0.0, 0.0, 0.0), 0.9, 5), bs.colours(4), bs.UNIT_MIN.copy(), bs.UNIT_MAX.copy()), 1
    elif shape == "three_children":                                    # three triangles, one per leaf: no node has four children
        scene, leaf = (bs.soup(3, (0.0, 0.0, 0.0), 0.9, 6), bs.colours(3), bs.UNIT_MIN.copy(), bs.UNIT_MAX.copy()), 1
    else:                                                              # a path: every inner node has a leaf and one inner child
        scene, leaf = bs.shrinking_chain(12, extra=bs.soup(40, (0.0, 0.1, 0.0), 0.6, 7)), 1
    f = frame_with_light(SMALL, CAM_OUTSIDE, 7, model_light=[0.3, 1.4, -1.2])
    check(scene, f, leaf, False)
