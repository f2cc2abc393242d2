"""The directed edge-light cases of tests/test_gpu_sequences.py are not vacuous: a light just outside the unit cube (by less than its
offset table's radius) with extra geometry beyond it, seen by the frame's camera.  On the CPU oracle's own geometry (Scene.trace), some
shadow segments from the extra geometry's visible points that lie beyond the light, to L + offset, are blocked by model triangles -- so
a shadow walk that drops the model for those points (a shaft direction taken from the light's side of the box) changes pixels.  With
radius 0 (hard shadows, the control) none are: the segments from beyond the light never reach the box."""
import numpy as np
import pytest

from helpers import EDGE_GAPS, EDGE_RADII, EDGE_SIGNS, camera_rays, edge_light_case, edge_light_frame, orc, unit_cube_scene

TARGET_TREE, TARGET_ROOT = 1, 2


@pytest.fixture(scope="module")
def cube():
    v9, argb, lo, hi = unit_cube_scene(20000)
    o = orc.Scene()
    o.set_triangles(v9, argb, lo, hi)
    assert o.build_tree() == 0
    return o


def blocked_points(o, c, res=(64, 48)):
    """(visible extra-geometry points beyond the light on one of its outside axes, those of them with a segment blocked by the model)"""
    o.set_extra(c["prims"])
    start, dirs = camera_rays(edge_light_frame(c, *res))
    r = o.trace(TARGET_ROOT, np.broadcast_to(start, dirs.shape), dirs)
    s = np.array(c["signs"])
    p = r["pos"][(r["hit"] == 1) & (r["tri_index"] < 0)]            # camera rays that end on the extra geometry
    p = p[((s * (p - c["light"]) > 0) & (s != 0)).any(axis=1)]
    ends = c["light"] + c["table"]
    starts = np.repeat(p, len(ends), axis=0)
    d = np.tile(ends, (len(p), 1)) - starts
    t = o.trace(TARGET_TREE, starts + d * 1e-6, d)
    hit = ((t["hit"] == 1) & (t["ray_frac"] <= 1.0)).reshape(len(p), len(ends))
    return len(p), int(hit.any(axis=1).sum())


@pytest.mark.parametrize("signs", EDGE_SIGNS)
def test_edge_light_segments_are_blocked_by_the_model(cube, signs):
    for gap in EDGE_GAPS:
        for radius in EDGE_RADII:
            c = edge_light_case(signs, gap, radius)
            seen, blocked = blocked_points(cube, c)
            assert seen > 200, (signs, gap, radius, seen)             # the camera sees the extra geometry beyond the light
            if radius > gap:
                assert blocked > 0, (signs, gap, radius, seen)
            else:
                assert blocked == 0, (signs, gap, radius, blocked)
