"""The "box smaller than the model" case of tests/test_gpu_interior.py is not vacuous, shown with the CPU oracle alone: with the root
box shrunk to [-0.44, 0.44]^3 a band of the soup's triangles sticks out through every face, and for the light beyond that band some
shadow segments (light sample -> visible point) cross a triangle at a point OUTSIDE the root box.  The reference ignores such a crossing
(SpatialSubdivision.cs:394-401, 652), so Scene.trace does not report the segment blocked -- a classification that took a protruding
triangle for an interior one (no per-sample box exit) would block it and darken the pixel.

Counts found (32 x 24 frame, 6000 triangles, 100 samples, light (0.35, 1.1, -0.55)): 381 visible points, 38100 segments, 15062 of them
blocked in the full-size box, 14040 in the small one; 1022 segments cross a triangle outside the small box only and are not reported
blocked; 142 of the 346 pixels that show the same triangle under both boxes have a different colour (shadow factor)."""
import numpy as np

import interior_cases as ic
from helpers import camera_rays, orc

TARGET_NEAREST = 3                          # Scene.trace: the tree's clip + the nearest hit inside the root box, no tree needed
NCPU = 8


def test_segments_cross_protruding_triangles_outside_the_small_box():
    v9, argb = ic.soup()
    lo, hi = ic.small_box()
    flo, fhi = ic.roomy_box()
    small, full = orc.Scene(), orc.Scene()
    small.set_triangles(v9, argb, lo, hi)
    full.set_triangles(v9, argb, flo, fhi)
    p9 = np.asarray(v9).reshape(-1, 3, 3)
    sticks_out = ((p9 < lo) | (p9 > hi)).any(axis=(1, 2))
    inside = ((p9 >= lo) & (p9 <= hi)).any(axis=(1, 2))
    assert (sticks_out & inside).sum() > 500                           # the band: triangles with vertices on both sides of a face

    f = ic.light_frame(32, 24, ic.LIGHT_OUTSIDE, mode=orc.MODE_NEAREST)
    start, dirs = camera_rays(f)
    prim_s = small.trace(TARGET_NEAREST, np.broadcast_to(start, dirs.shape), dirs)
    prim_f = full.trace(TARGET_NEAREST, np.broadcast_to(start, dirs.shape), dirs)
    vis = prim_s["hit"] == 1
    e = prim_s["pos"][vis] + 0.001 * prim_s["normal"][vis]              # ShadowMethod's probe point
    ends = np.array(ic.LIGHT_OUTSIDE) + orc.area_light_offsets(f.random_seed, ic.SAMPLES)
    rs = np.tile(ends, (len(e), 1))                                    # the reference's shadow ray: from the light sample to the probe point
    rd = np.repeat(e, len(ends), axis=0) - rs
    a = small.trace(TARGET_NEAREST, rs, rd)
    b = full.trace(TARGET_NEAREST, rs, rd)
    blocked_small = (a["hit"] == 1) & (a["ray_frac"] <= 1.0)
    blocked_full = (b["hit"] == 1) & (b["ray_frac"] <= 1.0)
    assert not (blocked_small & ~blocked_full).any()                   # a crossing inside the small box is one inside the full box
    # blocked in the full box only: the segment crosses a triangle, and (the small box reports none) every crossing lies outside the small box
    only = blocked_full & ~blocked_small
    q = b["pos"][only]
    crossing_outside = ((q < lo - 1e-10) | (q > hi + 1e-10)).any(axis=1)
    print("visible", int(vis.sum()), "segments", len(rs), "blocked full", int(blocked_full.sum()), "blocked small", int(blocked_small.sum()),
          "outside-only", int(only.sum()))
    assert crossing_outside.all()
    assert int(only.sum()) > 0

    px_small, _ = small.render(f, threads=NCPU)
    px_full, _ = full.render(f, threads=NCPU)
    same_surface = vis & (prim_f["hit"] == 1) & (prim_f["tri_index"] == prim_s["tri_index"])
    differ = int((same_surface & (px_small != px_full)).sum())
    print("pixels with the same triangle", int(same_surface.sum()), "of them with another shadow factor", differ)
    assert differ > 0
