"""Umbra hints of the persistent packet shaft walk (k_shaft_pkt4, softray_amd/csrc/sr_umbra_hint.h): every 8x8 tile
leaves the leaf run whose triangle put lanes into umbra, and the next launch with the same tile grid tries the runs of the tile's 16x16
parent before it walks.  A hint is only ever a record to ask first -- the umbra test is the walk's own -- so every frame below must
equal the CPU oracle pixel for pixel, whatever the words left by the frame before it say.

Scene: a soup of small triangles over one half of a floor of two large triangles that face the camera and the light, and over the
other half one "roof" triangle, parallel to the floor and much closer to it than to the light (the umbra test needs the crossing in
the nearer half of a shaft); the light stands to the side, so the roof's shadow falls beside it on the clear floor, in sight of the
camera.  The area-light table is the test's own, radius 0.01.  The oracle's image must hold at least 50 aligned 8x8 tiles whose hit
pixels are all black: that is asserted on the oracle's image.

Frames are 512 x 384 with hook 831 (one workgroup per CU: the persistent walk at that size, as tests/test_gpu_placement.py reaches
it).  Switches 97 / 98 / 99 are values of the same hook, so their frames are 640 x 480 in one pipeline (SR_F_NO_SPLIT), the smallest
grid that is persistent without it on 256 CUs; sr_debug_counters [6] says that the persistent walk ran."""
import math
import os

import numpy as np
import pytest
import torch

import softray_amd as sa
from helpers import make_frame, orc, random_triangles

pytestmark = pytest.mark.gpu
NCPU = min(16, os.cpu_count() or 8)
DBG = sa._lib
RES, BIG = (512, 384), (640, 480)
SAMPLES = 5
RADIUS = 0.01
POSE = (135.0, -22.0)
BLACK = 0xFF000000

# ---- the scene, in the unit cube ----
N_AXIS = np.array([-0.5, 0.75, 0.45]) / math.sqrt(0.5 * 0.5 + 0.75 * 0.75 + 0.45 * 0.45)    # the floor's normal: towards camera and light
T1 = np.cross(N_AXIS, [0.0, 0.0, 1.0])
T1 /= np.linalg.norm(T1)
T2 = np.cross(N_AXIS, T1)
FLOOR_AT, ROOF_UP = -0.2, 0.22                                   # n.x of the floor; the roof's height above it


def plane_point(a, b, up=0.0):
    return N_AXIS * (FLOOR_AT + up) + T1 * a + T2 * b


def facing(v):
    """The triangle with the winding whose normal (edge1 x edge2) points along N_AXIS."""
    v = np.asarray(v, dtype=np.float64)
    return v if np.dot(np.cross(v[1] - v[0], v[2] - v[0]), N_AXIS) > 0 else v[[0, 2, 1]]


def scene(soup=3000, seed=12345):
    """(v9, argb, box_min, box_max): floor (2), roof (1), then `soup` small triangles above the floor's a < -0.1 half."""
    h = 0.36
    tris = [facing([plane_point(-h, -h), plane_point(h, -h), plane_point(h, h)]), facing([plane_point(-h, -h), plane_point(h, h), plane_point(-h, h)]),
            facing([plane_point(0.0, -0.3, ROOF_UP), plane_point(0.34, -0.3, ROOF_UP), plane_point(0.17, 0.32, ROOF_UP)])]
    colors = [0xFFD0D0D0, 0xFFD0D0D0, 0xFF40C040]
    u, argb, _ = random_triangles(soup, seed, space=1.0, extent=0.04, origin=0.0, mask_color=True)
    u = np.asarray(u, dtype=np.float64).reshape(-1, 3, 3)
    first = u[:, 0, :]                                                # v1 in [0, 1)^3 -> (a, b, height) over the floor's other half
    base = (plane_point(0.0, 0.0)[None, :] + T1[None, :] * (-0.35 + 0.12 * first[:, 0:1]) + T2[None, :] * (-0.33 + 0.62 * first[:, 1:2]) +
            N_AXIS[None, :] * (0.02 + 0.25 * first[:, 2:3]))
    soup_v = base[:, None, :] + (u - first[:, None, :])
    v9 = np.ascontiguousarray(np.concatenate([np.stack(tris), soup_v]))
    assert np.abs(v9).max() < 0.5
    return v9, np.concatenate([np.array(colors, dtype=np.uint32), np.asarray(argb, dtype=np.uint32)]), np.array([-0.5] * 3), np.array([0.5] * 3)


LIGHT = tuple(plane_point(1.1, 0.1, 0.9))                          # model space: to the side of the roof, 0.9 above the floor
LIGHT_MOVED = tuple(plane_point(1.0, 0.25, 0.95))


def table(radius=RADIUS, samples=SAMPLES):
    t = orc.area_light_offsets(1234567890, samples)
    return np.ascontiguousarray(t * (radius / np.sqrt((t * t).sum(axis=1)).max()))


def frame(res=RES, yaw=POSE[0], light=LIGHT):
    f = make_frame(res[0], res[1], yaw_deg=yaw, pitch_deg=POSE[1], depth=1.5, shadows=True, shadow_samples=SAMPLES)
    t = [f.transform[i] for i in range(12)]
    for r in range(3):
        f.light_pos_view[r] = t[4 * r] * light[0] + t[4 * r + 1] * light[1] + t[4 * r + 2] * light[2] + t[4 * r + 3]
    return f


def all_black_tiles(img, res, background=0xFFFF00FF):
    """Aligned 8x8 tiles with at least one hit pixel whose hit pixels are all opaque black."""
    w, h = res
    p = np.asarray(img).reshape(h, w)[: h // 8 * 8, : w // 8 * 8].reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(h // 8, w // 8, 64)
    hit = p != np.uint32(background)
    return int((hit.any(axis=2) & ((p == np.uint32(BLACK)) | ~hit).all(axis=2)).sum())


class World:
    """One geometry on the oracle, the oracle's frames (each rendered once) and the offset tables they point at."""

    def __init__(self, v9, argb, lo, hi):
        self.model = (v9, argb, lo, hi)
        self.o = orc.Scene()
        self.o.set_triangles(v9, argb, lo, hi)
        assert self.o.build_tree() == 0
        self.tables, self.wanted = {}, {}

    def frame(self, res=RES, yaw=POSE[0], light=LIGHT, radius=RADIUS):
        f = frame(res, yaw, light)
        f.area_light_offsets = self.tables.setdefault(radius, table(radius)).ctypes.data
        return f

    def want(self, **kw):
        key = tuple(sorted(kw.items()))
        if key not in self.wanted:
            self.wanted[key] = self.o.render(self.frame(**kw), threads=NCPU)[0].copy()
        return self.wanted[key]

    def gpu(self, hook=831, on_device=None):
        g = sa.GpuScene(0)
        g.set_triangles(*self.model)
        g.build((sa.MODE_BVH,), on_device=on_device)
        if hook is not None:
            g.debug_set(DBG.DBG_KERNEL_SWITCH, hook)
        return g

    def check(self, g, label, stats=False, **kw):
        sf = sa.Frame.from_buffer_copy(bytes(self.frame(**kw)))
        sf.trace_mode = sa.MODE_BVH
        if kw.get("res") == BIG:
            sf.flags |= DBG.F_NO_SPLIT                                 # one pipeline for the whole frame: 2048 tiles of 16 x 16
        got, _ = g.render(sf, stats=stats)
        want = self.want(**kw)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: %d of %d pixels differ from the oracle (first %s)" % (label, bad.size, want.size, bad[:5])
        return got


_WORLD = {}


def world(soup=3000):
    if soup not in _WORLD:
        _WORLD[soup] = World(*scene(soup))
    return _WORLD[soup]


def test_the_scene_has_tiles_in_full_umbra():
    w = world()
    for res in (RES, BIG):
        img = w.want(res=res)
        black = all_black_tiles(img, res)
        print("%d x %d: %d aligned 8x8 tiles with every hit pixel black, %d black pixels" % (res[0], res[1], black, int((img == np.uint32(BLACK)).sum())))
        assert black >= 50
    assert not np.array_equal(w.want(), w.want(light=LIGHT_MOVED)) and not np.array_equal(w.want(), w.want(radius=3 * RADIUS))
    assert not np.array_equal(w.want(), w.want(yaw=POSE[0] + 0.25))


def test_frame_sequence_equals_the_oracle():
    w = world()
    g = w.gpu()
    w.check(g, "1. frame A")
    w.check(g, "2. A again (hints of 1)")
    ctr = g.debug_counters()
    assert ctr[6] > 0 and ctr[7] > 0, ctr                              # the persistent walk, on the previous frame's tile lists (and so its hints)
    w.check(g, "3. object yawed 0.25 degrees", yaw=POSE[0] + 0.25)
    w.check(g, "4. light moved", light=LIGHT_MOVED)
    w.check(g, "5. light radius x 3", radius=3 * RADIUS)
    w.check(g, "A after 5")
    # 6. A on a second stream
    f = sa.Frame.from_buffer_copy(bytes(w.frame()))
    f.trace_mode = sa.MODE_BVH
    buf = torch.empty(RES[0] * RES[1], dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g.render_device(f, buf.data_ptr(), side.cuda_stream)
    side.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), w.want()), "6. A on a second stream"
    # 7. another tile grid, then A again
    w.check(g, "7. 384 x 512", res=(384, 512))
    w.check(g, "7. A after another grid")
    w.check(g, "7. A again")
    # ---- stale words: a model of a tenth as many triangles on the same handle ----
    small = world(soup=300)
    g.set_triangles(*small.model)
    g.build((sa.MODE_BVH,))
    small.check(g, "a tenth of the triangles, words of the larger model left behind")
    small.check(g, "... again")


def test_refit_with_moved_vertices():
    w = world()
    g = w.gpu(on_device=True)
    assert g.bvh_stats()[3] == 1
    w.check(g, "A")
    w.check(g, "A again")
    v9, argb, lo, hi = w.model
    moved = v9.copy()
    moved[2] += N_AXIS * 0.05 + T2 * 0.1                               # the roof: higher and to the side -- its shadow moves
    moved[3:] += T2 * 0.02
    assert np.abs(moved).max() < 0.5
    dev = torch.device("cuda", 0)
    g.refit_triangles_device(torch.from_numpy(moved).to(dev), None, lo, hi)
    m = World(moved, argb, lo, hi)
    assert not np.array_equal(m.want(), w.want())
    m.check(g, "refit")
    m.check(g, "refit, again")


def test_list_length_two():
    w = world()
    g = w.gpu()
    g.debug_set(DBG.DBG_ROUND_CAP0, 2)
    for turn in range(3):
        w.check(g, "list length 2, frame %d" % turn)
    w.check(g, "list length 2, yawed", yaw=POSE[0] + 0.25)
    assert g.debug_counters()[2] > 0                                   # hit points went on to the second round


def test_switches_97_and_99_give_the_same_frames():
    w = world()
    for hook in (97, 99):
        g = w.gpu(hook=hook)
        for turn in range(3):
            w.check(g, "switch %d, frame %d" % (hook, turn), res=BIG)
        assert g.debug_counters()[6] > 0                               # persistent without hook 831 at this size
        w.check(g, "switch %d, yawed" % hook, res=BIG, yaw=POSE[0] + 0.25)


def test_switch_98_counts_the_tiles_that_never_walk():
    """Statistics [22]: tiles that entered the walk with a lane finished by a hint, [23]: tiles that never took a node step; [20] / [21]: the
    walk length of all tiles / of the tiles that ended with every valid lane in umbra.  The first frame has no words to try."""
    w = world()
    g = w.gpu(hook=98)
    w.check(g, "switch 98, first frame", stats=True, res=BIG)
    first = g.ray_stats()
    assert g.debug_counters()[6] > 0
    w.check(g, "switch 98, second frame", stats=True, res=BIG)
    second = g.ray_stats()
    print("switch 98: first frame [20..23] %s, second frame %s" % ([int(x) for x in first[20:24]], [int(x) for x in second[20:24]]))
    assert first[22] == 0 and first[23] == 0, first
    assert second[22] > 0 and second[23] > 0, second
    assert first[20] > 0 and 0 < first[21] < first[20]
    assert second[20] < first[20]                                      # the tiles that never walked cost their hint's filters only
