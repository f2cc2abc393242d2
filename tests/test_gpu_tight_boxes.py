"""The boxes of the camera- / light-ordered node copies, fitted to the records their rays can hit (k_tight_level / k_tight_top,
softray_amd/csrc/sr_tight_boxes.h).  Only boxes of the per-pose copies change, so every frame must equal the frame with
SR_DBG_KERNEL_SWITCH 72 (copies with the base tree's boxes) pixel for pixel, and the small frames the CPU oracle as well.

Scenes: a closed lat-long sphere over a floor, seen from outside -- its whole far side is camera-dead and the side away from the light
light-dead, so whole subtrees and leaves go absent -- and the unit-cube soup.  Frames are 200 x 160 (partial tiles, one workgroup per
tile) and 640 x 480 in one pipeline (SR_F_NO_SPLIT), the smallest grid that takes the persistent tile feed without another value of the
same hook; sr_debug_counters [6] says that it did."""
import math
import os

import numpy as np
import pytest
import torch

import softray_amd as sa
from helpers import make_frame, orc, unit_cube_scene

pytestmark = pytest.mark.gpu
NCPU = min(16, os.cpu_count() or 8)
DBG = sa._lib
OFF = 72                                                             # SR_DBG_KERNEL_SWITCH: the copies keep the base boxes
SMALL, BIG = (200, 160), (640, 480)
SAMPLES = 5
LO, HI = np.array([-0.5] * 3), np.array([0.5] * 3)


def sphere_scene(rings=40, segments=64, radius=0.3):
    """A closed sphere (outward normals: edge1 x edge2 points away from the centre) above a floor of two triangles that face +y."""
    tris = []

    def p(i, j):
        th, ph = math.pi * i / rings, 2.0 * math.pi * j / segments
        return np.array([radius * math.sin(th) * math.cos(ph), 0.05 + radius * math.cos(th), radius * math.sin(th) * math.sin(ph)])

    centre = np.array([0.0, 0.05, 0.0])
    for i in range(rings):
        for j in range(segments):
            quad = (p(i, j), p(i + 1, j), p(i + 1, j + 1), p(i, j + 1))
            for t in ((quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])):
                n = np.cross(t[1] - t[0], t[2] - t[0])
                if np.linalg.norm(n) < 1e-12:
                    continue                                           # the poles' degenerate halves
                tris.append(t if np.dot(n, (t[0] + t[1] + t[2]) / 3.0 - centre) > 0 else (t[0], t[2], t[1]))
    h, y = 0.45, -0.35
    floor = [(np.array([-h, y, -h]), np.array([h, y, h]), np.array([h, y, -h])), (np.array([-h, y, -h]), np.array([-h, y, h]), np.array([h, y, h]))]
    for t in floor:
        tris.append(t if np.cross(t[1] - t[0], t[2] - t[0])[1] > 0 else (t[0], t[2], t[1]))
    v9 = np.ascontiguousarray(np.array(tris, dtype=np.float64))
    rnd = np.random.default_rng(7)
    argb = (rnd.integers(0x404040, 0xFFFFFF, size=len(tris)).astype(np.uint32)) | np.uint32(0xFF000000)
    assert 4000 < len(tris) < 6000 and np.abs(v9).max() < 0.5
    return v9, argb, LO, HI


def frame(res=SMALL, yaw=135.0, pitch=-22.0, depth=1.5, light=None, samples=SAMPLES, shadows=True):
    f = make_frame(res[0], res[1], yaw_deg=yaw, pitch_deg=pitch, depth=depth, shadows=shadows, shadow_samples=samples if shadows else 0)
    if light is not None:                                              # a model-space light position
        t = [f.transform[i] for i in range(12)]
        for r in range(3):
            f.light_pos_view[r] = t[4 * r] * light[0] + t[4 * r + 1] * light[1] + t[4 * r + 2] * light[2] + t[4 * r + 3]
    return f


def as_sr(f, res=None, **fields):
    sf = sa.Frame.from_buffer_copy(bytes(f))
    sf.trace_mode = sa.MODE_BVH
    if res == BIG:
        sf.flags |= DBG.F_NO_SPLIT
    for k, v in fields.items():
        setattr(sf, k, v)
    return sf


class World:
    def __init__(self, model):
        self.model = model
        self.o = orc.Scene()
        self.o.set_triangles(*model)
        assert self.o.build_tree() == 0
        self.wanted = {}

    def want(self, **kw):
        key = tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple, np.ndarray)) else v) for k, v in kw.items()))
        if key not in self.wanted:
            self.wanted[key] = self.o.render(frame(**kw), threads=NCPU)[0].copy()
        return self.wanted[key]

    def gpu(self, off=False, on_device=None, model=None):
        g = sa.GpuScene(0)
        g.set_triangles(*(model or self.model))
        g.build((sa.MODE_BVH,), on_device=on_device)
        if off:
            g.debug_set(DBG.DBG_KERNEL_SWITCH, OFF)
        return g


_WORLDS = {}


def world(name):
    if name not in _WORLDS:
        _WORLDS[name] = World(sphere_scene() if name == "sphere" else unit_cube_scene(int(name)))
    return _WORLDS[name]


def both(w, label, oracle=True, pair=None, **kw):
    """The frame with the step and without it (on two scenes, or the given pair): equal pixels; and the oracle's."""
    on, off = pair or (w.gpu(), w.gpu(off=True))
    sf = as_sr(frame(**kw), kw.get("res"))
    a, b = on.render(sf)[0].copy(), off.render(sf)[0].copy()
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, "%s: %d pixels differ between the fitted and the base boxes (first %s)" % (label, bad.size, bad[:5])
    if oracle:
        bad = np.flatnonzero(a != w.want(**kw))
        assert bad.size == 0, "%s: %d pixels differ from the oracle (first %s)" % (label, bad.size, bad[:5])
    return a


# ---- 1. a closed mesh from outside: dead subtrees, empty leaves ----
def test_closed_mesh_from_outside():
    w = world("sphere")
    on, off = w.gpu(), w.gpu(off=True)
    for g in (on, off):
        g.debug_set(DBG.DBG_KERNEL_TIMING, 1)
    img = both(w, "sphere 200 x 160", pair=(on, off))
    assert (img != np.uint32(0xFFFF00FF)).sum() > 5000
    assert "k_tight_boxes" in on.kernel_times() and on.kernel_times()["k_tight_boxes"][1] == 2       # the camera copy and the light copy
    assert "k_tight_boxes" not in off.kernel_times()
    both(w, "sphere 640 x 480, persistent feed", oracle=False, pair=(on, off), res=BIG)
    assert on.debug_counters()[6] > 0 and off.debug_counters()[6] > 0
    # the same handle, the switch thrown between frames: the copies are re-made either way
    sf = as_sr(frame())
    want = w.want()
    on.debug_set(DBG.DBG_KERNEL_SWITCH, OFF)
    assert np.array_equal(on.render(sf)[0], want)
    on.debug_set(DBG.DBG_KERNEL_SWITCH, -1)
    assert np.array_equal(on.render(sf)[0], want)
    assert on.kernel_times()["k_tight_boxes"][1] == 4                  # the larger frame had the same pose: its copies stood; the last frame made both again


# ---- 2. camera and light inside the root box; the light outside on one axis ----
LIGHTS = {"inside": (0.1, 0.2, -0.1), "+x": (0.9, 0.1, 0.1), "-x": (-0.9, 0.1, 0.1), "+y": (0.1, 0.9, 0.1), "-y": (0.1, -0.9, 0.1), "+z": (0.1, 0.1, 0.9),
          "-z": (0.1, 0.1, -0.9)}


@pytest.mark.parametrize("where", sorted(LIGHTS))
def test_light_inside_and_beside_the_box(where):
    both(world("3000"), "light " + where, light=LIGHTS[where])


def test_camera_inside_the_box():
    w = world("3000")
    both(w, "camera inside", depth=0.3)
    both(w, "camera and light inside", depth=0.3, light=LIGHTS["inside"])


# ---- 3. A, B, A on one scene and scratch set ----
def test_pose_sequence_on_one_scene():
    w = world("sphere")
    pair = (w.gpu(), w.gpu(off=True))
    a = dict(yaw=135.0)
    b = dict(yaw=20.0, pitch=-40.0, light=(-0.6, 0.8, 0.3))
    for turn, kw in enumerate((a, b, a, a)):
        both(w, "turn %d" % turn, pair=pair, **kw)
    for turn, kw in enumerate((a, b, a)):
        both(w, "640 x 480, turn %d" % turn, oracle=False, pair=pair, res=BIG, **kw)
    assert pair[0].debug_counters()[6] > 0


# ---- 4. a refit moves the boxes ----
def test_boxes_follow_a_refit():
    w = world("sphere")
    pair = (w.gpu(on_device=True), w.gpu(off=True, on_device=True))
    both(w, "before the refit", pair=pair)
    v9, argb, lo, hi = w.model
    moved = v9.copy()
    moved[:-2] = (moved[:-2] - [0.0, 0.05, 0.0]) * [1.3, 0.7, 1.1] + [0.05, 0.02, -0.04]      # the sphere, squashed and shifted; the floor stays
    assert np.abs(moved).max() < 0.5
    m = World((moved, argb, lo, hi))
    assert not np.array_equal(m.want(), w.want())
    for g in pair:
        g.refit_triangles_device(torch.from_numpy(moved).to(torch.device("cuda", 0)), None, lo, hi)
    both(m, "after the refit", pair=pair)
    both(m, "after the refit, again", pair=pair)


# ---- 5. truncated lists; the other readers of the copies ----
@pytest.mark.parametrize("cap", [2, 40])
def test_list_caps(cap):
    w = world("3000")
    pair = (w.gpu(), w.gpu(off=True))
    for g in pair:
        g.debug_set(DBG.DBG_ROUND_CAP0, cap)
    both(w, "list cap %d" % cap, pair=pair)
    if cap == 2:
        assert pair[0].debug_counters()[2] > 0                         # hit points went on to the second round


def test_hits_and_coherent_points_read_the_same_copies():
    w = world("sphere")
    on, off = w.gpu(), w.gpu(off=True)
    sf = as_sr(frame())
    ha, hb = on.render_hits(sf), off.render_hits(sf)
    for k in ha:
        assert np.array_equal(ha[k], hb[k]), "sr_render_hits: %s differs" % k
    hit = ha["hit"].astype(bool)
    assert hit.sum() > 5000
    pos, nrm, col = ha["pos"][hit], ha["normal"][hit], ha["color"][hit]
    pa, pb = on.shadow_points(sf, pos, nrm, col, coherent=True), off.shadow_points(sf, pos, nrm, col, coherent=True)
    assert np.array_equal(pa, pb), "sr_shadow_points (coherent) differs"
    assert np.array_equal(pa, on.shadow_points(sf, pos, nrm, col, coherent=False))
    assert len(np.unique(pa)) > 10


# ---- 6. the walks do no more than before ----
def test_counters_do_not_grow():
    w = world("20000")
    sf = as_sr(frame(res=(256, 192)))
    stats = []
    for off in (False, True):
        g = w.gpu(off=off)
        g.render(sf, stats=True)
        stats.append([int(x) for x in g.ray_stats()])
    on, base = stats
    print("counters [1], [2], [6], [7], [10]: fitted %s, base boxes %s" % ([on[i] for i in (1, 2, 6, 7, 10)], [base[i] for i in (1, 2, 6, 7, 10)]))
    for i in (1, 2, 6, 7, 10):
        assert base[i] > 0 and on[i] <= base[i], "counter [%d]: %d with the fitted boxes, %d with the base boxes" % (i, on[i], base[i])
