"""The placements of tests/placement_cases.py are not vacuous, shown with the CPU oracle alone: at every placement the camera rule
puts the model in the frame (hit pixels and background both), the area light casts a penumbra (the soft-shadow frame differs from the
one with an all-zero offset table), shadows occur at all, and the property each placement is named for holds -- a box centre that is
no fp32 number (`near`, `far`), triangles that leave the box and cross its faces (`cut`), probe points hit + 0.001 n that lie
outside the box (`small`: all but those along a diagonal normal; `tiny`, at half that scale: all).  The thresholds are lower bounds on the cases, not measurements of the library.

Counts found (96 x 80, 17 samples, 6000 triangles; hit pixels / penumbra pixels): origin 4079 / 2697, near 4015 / 2376, far 6717 / 4218
(20000 triangles), far_scaled 3940 / 2226, big 4079 / 2676, small 2607 / 257, flat 3333 / 517, loose 4079 / 2697, cut 1291 / 691,
far_probe 3865 / 2577; the two extra placements of the soft-shadow schedules: tiny 2636 / 60, far_limit 3862 hit pixels.  At `small`
605 of 648 probe points (48 x 40 frame) lie outside the box, at `tiny` all of them."""
import numpy as np
import pytest

import placement_cases as pc
from helpers import camera_rays, orc

NCPU = 8
RES = (96, 80)
SAMPLES = 17
TARGET_NEAREST = 3                          # Scene.trace: the nearest hit inside the root box, no tree needed
BACKGROUND = 0xff00ff
MIN_HIT, MIN_BACKGROUND, MIN_PENUMBRA = 500, 500, 200


def oracle_scene(name):
    v9, argb, lo, hi = pc.placed(name)
    o = orc.Scene()
    o.set_triangles(v9, argb, lo, hi)
    rc = o.build_tree()
    assert rc == (0 if name in pc.HAS_TREE else -2), (name, rc)        # (`cut`: the reference tree refuses vertices outside the box)
    return o, v9, lo, hi


@pytest.mark.parametrize("name", pc.NAMES + pc.EXTRA)
def test_placement_is_not_vacuous(name):
    o, v9, lo, hi = oracle_scene(name)
    mode = orc.MODE_REF_TREE if name in pc.HAS_TREE else orc.MODE_NEAREST
    table, zeros = pc.offset_table(name, SAMPLES), pc.offset_table(name, SAMPLES, zero=True)
    soft, _ = o.render(pc.frame(name, *RES, table=table, shadows=True, shadow_samples=SAMPLES, mode=mode), threads=NCPU)
    hard, _ = o.render(pc.frame(name, *RES, table=zeros, shadows=True, shadow_samples=SAMPLES, mode=mode), threads=NCPU)
    lit, _ = o.render(pc.frame(name, *RES, mode=mode), threads=NCPU)
    hit = int(((lit & 0xFFFFFF) != BACKGROUND).sum())
    penumbra = int((soft != hard).sum())
    shadowed = int((soft != lit).sum())
    print(name, "hit", hit, "of", lit.size, "penumbra", penumbra, "shadowed", shadowed, "ratio |centre| / extent", pc.offset_ratio(lo, hi))
    assert hit >= MIN_HIT and lit.size - hit >= MIN_BACKGROUND, (name, hit)
    assert penumbra >= (MIN_PENUMBRA if name in pc.NAMES else 1), (name, penumbra)
    assert shadowed > 0, name
    # a light inside the box and a directional light light the model too (the frames test_gpu_placement.py renders)
    inside, _ = o.render(pc.frame(name, *RES, table=table, light_model=pc.light_inside(lo, hi), shadows=True, shadow_samples=SAMPLES, mode=mode), threads=NCPU)
    assert not np.array_equal(inside, soft), name
    if name == "big":                                                   # the directional light's 1000-unit start lies within the model's reach
        dshadow, _ = o.render(pc.frame(name, *RES, shadows=True, point_light=False, mode=mode), threads=NCPU)
        dlit, _ = o.render(pc.frame(name, *RES, point_light=False, mode=mode), threads=NCPU)
        assert not np.array_equal(dshadow, dlit)


@pytest.mark.parametrize("name", ["near", "far"])
def test_box_centre_is_no_fp32_number(name):
    _, _, lo, hi = pc.placed(name)
    assert pc.centre_is_no_fp32_number(lo, hi)
    assert not pc.centre_is_no_fp32_number(*pc.placed("origin")[2:])


def test_cut_triangles_leave_the_box_and_cross_its_faces():
    v9, _, lo, hi = pc.placed("cut")
    out, crosses = pc.sticks_out(v9, lo, hi)
    print("cut: triangles with a vertex outside", int(out.sum()), "crossing a face plane", int(crosses.sum()), "of", len(out))
    assert out.sum() >= 1 and crosses.sum() >= 1
    vlo, vhi = v9.reshape(-1, 3).min(axis=0), v9.reshape(-1, 3).max(axis=0)
    assert (vlo < lo).all() and (vhi > hi).all()                       # the vertex bounds exceed the box on every side


def test_loose_box_is_larger_than_the_model_and_off_centre():
    v9, _, lo, hi = pc.placed("loose")
    p = v9.reshape(-1, 3)
    assert (p.min(axis=0) > lo + 0.5).all() and (p.max(axis=0) < hi - 1.0).all()
    assert (np.abs(pc.centre(lo, hi)) > 0.3).all()


def probe_points(name):
    """ShadowMethod's probe points hit + 0.001 n of the camera hits of a 48 x 40 frame, and the hits themselves."""
    o, v9, lo, hi = oracle_scene(name)
    f = pc.frame(name, 48, 40, mode=orc.MODE_NEAREST)
    start, dirs = camera_rays(f)
    hits = o.trace(TARGET_NEAREST, np.broadcast_to(start, dirs.shape), dirs)
    vis = hits["hit"] == 1
    assert vis.sum() >= 200
    nrm = hits["normal"][vis]
    assert np.allclose((nrm * nrm).sum(axis=1), 1.0)
    assert not pc.outside_box(hits["pos"][vis], lo, hi).any()
    return hits["pos"][vis] + 0.001 * nrm, lo, hi


def test_tiny_probe_points_all_leave_the_box():
    """The probe point of every camera hit lies outside the root box: a unit normal's largest component is at least 1 / sqrt(3), and
    0.001 / sqrt(3) exceeds the box's extent of 1 / 2048, so no shadow start is "inside the box"."""
    probe, lo, hi = probe_points("tiny")
    assert 0.001 / np.sqrt(3.0) > float((hi - lo).max())
    assert pc.outside_box(probe, lo, hi).all()


def test_small_probe_points_leave_the_box_except_along_diagonals():
    """Extent 1 / 1024: 0.001 exceeds it, 0.001 / sqrt(3) does not.  A probe point leaves the box whenever the normal is within about 12
    degrees of an axis (0.001 cos > 1 / 1024) and may stay inside along a diagonal: starts of both kinds occur in one frame."""
    probe, lo, hi = probe_points("small")
    assert 0.001 > float((hi - lo).max()) > 0.001 / np.sqrt(3.0)
    out = pc.outside_box(probe, lo, hi)
    print("small: probe points outside the box", int(out.sum()), "of", len(out))
    assert out.sum() >= len(out) // 2 and (~out).sum() >= 10


def test_offset_ratios():
    """far_probe sits near the documented limit of |centre| / extent (include/softray.h at sr_set_triangles)."""
    ratio = {n: pc.offset_ratio(*pc.placed(n, 10)[2:]) for n in pc.PLACEMENTS}
    assert 5.9e4 < ratio["far_probe"] < 6.1e4 and ratio["origin"] == 0.0
    assert 0.2 * pc.OFFSET_LIMIT < ratio["far_limit"] < 0.3 * pc.OFFSET_LIMIT
    assert all(r < ratio["far_probe"] for n, r in ratio.items() if n not in ("far_probe", "far_limit"))
