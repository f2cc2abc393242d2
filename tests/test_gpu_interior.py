"""The shadow classification's shortcut for candidate lists of interior triangles (cls_umax, sr_pipeline.hip): a hit point
whose candidates all lie inside the root box (shrunk by 1e-5 x its largest extent) skips the per-sample box exits.  Every frame here is
compared with the oracle rendered in the test, with the shortcut on (production) and off (SR_DBG_KERNEL_SWITCH 93); the census of the two
paths (switch 94 / 95: ray statistics [22] = hit points classified with the shortcut, [23] = with the per-sample box exits) says which
path the frame took.  100 samples, own BVH (device-built and host-built)."""
import os

import numpy as np
import pytest

import interior_cases as ic
import softray_amd as sa
from helpers import orc

pytestmark = pytest.mark.gpu
NCPU = os.cpu_count() or 8
RES = (112, 96)
SWITCH = sa._lib.DBG_KERNEL_SWITCH
GENERIC, CENSUS, CENSUS_GENERIC = 93, 94, 95


def as_bvh(frame):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = sa.MODE_BVH
    return f


def scenes(v9, argb, lo, hi, on_device, tree=True):
    g, o = sa.GpuScene(0), orc.Scene()
    for s in (g, o):
        s.set_triangles(v9, argb, lo, hi)
    g.build((sa.MODE_BVH,), on_device=on_device)
    if tree:
        assert o.build_tree() == 0
    return g, o


def check(g, o, f, tag):
    """Pixels of the frame against the oracle with the shortcut on and off; returns (hit points classified, with the shortcut, without)."""
    want, _ = o.render(f, threads=NCPU)
    census = {}
    for hook in (-1, GENERIC, CENSUS, CENSUS_GENERIC):
        g.debug_set(SWITCH, hook)
        got, _ = g.render(as_bvh(f))
        st = g.ray_stats()
        assert np.array_equal(got, want), (tag, hook, int((got != want).sum()))
        if hook in (-1, GENERIC):                                                # ... and the kernels' uncounted instantiations (the production ones)
            plain, _ = g.render(as_bvh(f), stats=False)
            assert np.array_equal(plain, want), (tag, hook, "no statistics", int((plain != want).sum()))
        census[hook] = (int(st[9]), int(st[22]), int(st[23]))
    g.debug_set(SWITCH, -1)
    items, fast, generic = census[CENSUS]
    print(tag, "census", census)
    assert census[-1][1:] == (0, 0) and census[GENERIC][1:] == (0, 0)        # the census is opt-in: [22], [23] stay the mirror rays' otherwise
    assert items > 0 and fast + generic == items, (tag, census)              # the frame reached the classification kernels
    assert census[CENSUS_GENERIC] == (items, 0, items), (tag, census)        # switched off: every hit point takes the generic block
    return items, fast, generic


@pytest.mark.parametrize("on_device", [True, False])
def test_tight_box(on_device):
    """Root box = the exact vertex bounds (what a real model gives): the extremal triangles touch it, every other one is interior."""
    v9, argb = ic.soup()
    lo, hi = ic.tight_box(v9)
    g, o = scenes(v9, argb, lo, hi, on_device)
    fast = generic = 0
    for light, kw in ((ic.LIGHT_OUTSIDE, {}), ((1.1, 0.3, -0.4), dict(yaw_deg=20.0, pitch_deg=35.0)), ((0.2, 0.3, -1.2), dict(sub_pixel_res=2))):
        _, a, b = check(g, o, ic.light_frame(*RES, light, **kw), ("tight", on_device, light))
        fast += a
        generic += b
    assert fast > 0 and generic > 0, (fast, generic)                   # lists with and without an extremal triangle exist


@pytest.mark.parametrize("on_device", [True, False])
def test_box_smaller_than_the_model(on_device):
    """A band of triangles sticks out through every face of the root box and the light lies beyond it: sample rays cross the protruding
    parts outside the box, where the reference ignores them (tests/test_interior_cases.py counts such segments on the oracle).  A
    shortcut that trusted a wrong bit would darken pixels.  The oracle has no tree for such a box: its nearest-hit mode is the BVH's rule."""
    v9, argb = ic.soup()
    lo, hi = ic.small_box()
    g, o = scenes(v9, argb, lo, hi, on_device, tree=False)
    for light in (ic.LIGHT_OUTSIDE, (0.9, 0.9, -0.9)):
        _, fast, generic = check(g, o, ic.light_frame(*RES, light, mode=orc.MODE_NEAREST), ("small", on_device, light))
        assert generic > 0 and fast > 0, (fast, generic)


def test_roomy_box():
    """The benchmark's situation, a box clearly larger than the soup: every list is interior, no hit point computes a box exit."""
    v9, argb = ic.soup()
    lo, hi = ic.roomy_box()
    g, o = scenes(v9, argb, lo, hi, None)
    for light, kw in ((ic.LIGHT_OUTSIDE, {}), ((0.2, 0.3, -1.2), dict(yaw_deg=20.0, pitch_deg=35.0))):
        items, fast, generic = check(g, o, ic.light_frame(*RES, light, **kw), ("roomy", light))
        assert generic == 0 and fast == items, (items, fast, generic)
    # short lists: the hit points go on to the later rounds (k_shadow_cls, lists of several chunks), which take the shortcut too
    g.debug_set(sa._lib.DBG_ROUND_CAP0, 5)
    items, fast, generic = check(g, o, ic.light_frame(*RES, ic.LIGHT_OUTSIDE), ("roomy, round 2", ic.LIGHT_OUTSIDE))
    g.debug_set(sa._lib.DBG_ROUND_CAP0, -1)
    assert generic == 0 and fast == items, (items, fast, generic)


def test_light_inside_and_vertices_on_the_margin():
    """A light inside the box, and triangles with one vertex exactly on a face of the shrunk box (the margin's boundary) and one ulp of the
    FP64 coordinate to either side of it: whichever way such a record's byte falls, the pixels are the oracle's."""
    v9, argb = ic.soup()
    lo, hi = ic.roomy_box()
    delta = ic.DELTA_REL * float((hi - lo).max())
    extra = []
    for axis in range(3):
        for face, sign in ((hi[axis] - delta, 1.0), (lo[axis] + delta, -1.0)):
            for k, coord in enumerate((np.nextafter(face, -np.inf), face, np.nextafter(face, np.inf))):
                a = np.array([0.1 * k - 0.15, 0.05 * k - 0.1, 0.12 - 0.1 * k])
                t = np.stack([a, a + [0.09, 0.02, 0.0], a + [0.01, 0.03, 0.08]])
                t[:, axis] = face - sign * np.array([0.0, 0.07, 0.05])          # first vertex on the boundary, the others inside
                t[0, axis] = coord
                extra.append(t)
                extra.append(t[::-1].copy())                                     # (both windings: one of them faces the light)
    tv = np.concatenate([np.asarray(v9).reshape(-1, 3, 3), np.array(extra)])
    ta = np.concatenate([argb, np.full(len(extra), 0xFFE0E0E0, dtype=np.uint32)])
    for box in ((lo, hi), ic.tight_box(tv)):                                     # (the margin's faces belong to the first box; the second: light inside a tight box)
        g, o = scenes(tv, ta, box[0], box[1], None)
        for light in (ic.LIGHT_INSIDE, (0.3, 0.45, 0.2), ic.LIGHT_OUTSIDE):
            check(g, o, ic.light_frame(*RES, light), ("margin", tuple(box[0]), light))
