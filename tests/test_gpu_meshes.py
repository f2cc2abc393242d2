"""Frames, ray batches and point calls on structured meshes (tests/mesh_cases.py): the HIP path against the oracle on connected surfaces
with shared vertices, bit for bit -- every comparison is np.array_equal, there is no tolerance anywhere.  Per scene: every frame kind
(shaded, soft shadows, a light inside the box, a directional light, a row range, sub-pixel sampling with focal blur, mirror bounces,
path tracing) on every structure (device-built LBVH, host SAH, the reference tree with and without statistics, brute force); every
schedule of the soft-shadow frame on the device LBVH, per scene and per light of `edge_on`; the persistent shaft walk with a light
sequence; the G-buffer; ray batches at mesh vertices and edge midpoints; the point calls on the mesh's vertices; a refit height field.
The ray statistics say that the stage under test ran: [12] pairs classified in fp32, [13] pairs handed to the FP64 test, [22] / [23] hit
points on the interior shortcut / the generic block (hook 94), debug counters [2] / [3] the second round and the exact fallback,
[6] / [7] the persistent walk and its longest-first order.

tests/test_mesh_cases.py shows on the oracle alone that no scene is vacuous.

Figures of the default schedule, 117 x 91, 17 samples, device LBVH, on an MI355X (shadow rays [4], hit points [9], fp32 pairs [12],
FP64 pairs [13]):
    terrain             9690   574   125970    32    census [22] / [23] 574 / 0
    torus               9257   561    90812    57    census [22] / [23] 561 / 0
    fine               27721  1819   285277   172    census [22] / [23] 1819 / 0
    room              117771  7104  1460041   715    census [22] / [23] 7104 / 0
    room_flush        115204  6953  1464876   697    census [22] / [23] 1923 / 5030
    slivers            24329  1502  1042773    82    census [22] / [23] 1502 / 0
    edge_on            51141  3088   316205   110    census [22] / [23] 3088 / 0
    edge_on:in_plane  102832  7597  3443358   762    census [22] / [23] 7597 / 0
    edge_on:pierced   116344  7851  4248295  2391    census [22] / [23] 7851 / 0
    edge_on:straddle  119961  8072  4121853   812    census [22] / [23] 8072 / 0
(one run: the pair counts move by a fraction of a percent between runs, the pixels do not.)"""
import os

import numpy as np
import pytest
import torch

import ao_points_model as apm
import gbuffer_model as gbm
import mesh_cases as mc
import path_points_model as ppm
import pathtrace_model as ptm
import shadow_points_model as spm
import softray_amd as sa
import static_shadow_points_model as ssm
from helpers import make_frame, orc

pytestmark = pytest.mark.gpu
NCPU = min(16, os.cpu_count() or 8)
DBG = sa._lib
DEV = torch.device("cuda", 0)
RES, ODD, BLUR_RES, BIG = (96, 80), (117, 91), (72, 56), (512, 384)        # 117 x 91: partial 8 x 8 tiles on both axes
SAMPLES = 17
KEYS = gbm.KEYS
ITEM = dict(hit=(np.uint8, 1), ray_frac=(np.float64, 1), pos=(np.float64, 3), normal=(np.float64, 3), color=(np.uint32, 1), tri_index=(np.int32, 1))
SEED = mc.SEED
LIGHT_CASES = tuple(mc.NAMES) + tuple("edge_on:" + k for k in sorted(mc.EDGE_ON_LIGHTS))
_CASES = {}


class Case:
    """One scene: its arrays, the oracle's scene (with the tree, and without for brute force) and its frames (each rendered once), the
    library's scenes by structure."""

    def __init__(self, name, model=None):
        self.name = name
        self.v9, self.argb, self.lo, self.hi = model or mc.scene(name)
        self.o, self.brute = orc.Scene(), orc.Scene()
        for s in (self.o, self.brute):
            s.set_triangles(self.v9, self.argb, self.lo, self.hi)
        assert self.o.build_tree() == 0
        self.tables = {n: mc.offset_table(name, n) for n in (SAMPLES, 33)}          # kept alive: frames point at them
        self.scenes, self.wanted, self.points = {}, {}, None

    def scene(self, structure):
        """"lbvh" / "sah": the own BVH, device- / host-built; "tree": the reference tree (and the own BVH its shadow rays may use)."""
        if structure not in self.scenes:
            g = sa.GpuScene(0)
            g.set_triangles(self.v9, self.argb, self.lo, self.hi)
            if structure == "tree":
                g.build((sa.MODE_REF_TREE, sa.MODE_BVH))
            else:
                g.build((sa.MODE_BVH,), on_device=structure == "lbvh")
                assert g.bvh_stats()[3] == (1 if structure == "lbvh" else 0)
            self.scenes[structure] = g
        return self.scenes[structure]

    def frame(self, kind, w=RES[0], h=RES[1], light=None, omode=orc.MODE_NEAREST, **more):
        soft = dict(shadows=True, shadow_samples=SAMPLES, table=self.tables[SAMPLES])
        kw = {"shaded": dict(),
              "soft": soft,
              "blur": dict(shadows=True, shadow_samples=33, table=self.tables[33], sub_pixel_res=2, focal_blur=True),
              "inside": dict(soft, light_model=mc.light_inside(self.lo, self.hi)),
              "directional": dict(shadows=True, point_light=False),
              "mirror1": dict(), "mirror3": dict(),
              "rows": dict(soft, start_row=11, end_row=h - 23)}[kind]
        if light is not None:
            kw = dict(kw, light_model=np.asarray(light, dtype=np.float64))
        f = mc.frame(self.name, w, h, mode=omode, **dict(kw, **more))
        if kind.startswith("mirror"):
            f.max_bounces, f.reflectivity = int(kind[-1]), 0.5
        return f

    def want(self, kind, w=RES[0], h=RES[1], light=None, omode=orc.MODE_NEAREST):
        """The oracle's frame in its trace mode `omode`, rendered once.  On a mesh the reference's three ways to find a hit are three
        yardsticks: a camera ray through a shared edge or a border of coplanar neighbours has two hits at (nearly) one rayFrac, and brute
        force (the first of the nearest in index order), the tree (the first leaf's) and the nearest hit inside the box choose differently
        on a few pixels of `torus` and `edge_on` -- in the oracle itself.  SR_MODE_BVH is held to the nearest hit."""
        key = (kind, w, h, None if light is None else tuple(light), omode)
        if key not in self.wanted:
            self.wanted[key] = self.o.render(self.frame(kind, w, h, light, omode), threads=NCPU)[0]
            self.wanted[key].setflags(write=False)
        return self.wanted[key]

    def vertex_points(self, limit):
        """(pos, normal, colour) of the mesh's vertices, evenly thinned to `limit`."""
        if self.points is None:
            self.points = mc.vertex_points(self.name)
        pos, nrm, col = self.points
        idx = (np.arange(min(limit, len(pos))) * len(pos)) // min(limit, len(pos))
        return np.ascontiguousarray(pos[idx]), np.ascontiguousarray(nrm[idx]), np.ascontiguousarray(col[idx])

    def geometry(self, mode, shadows=False):
        """(oracle scene, Scene.trace target) that answers a ray as the frame's root geometry in `mode` does; shadows: a sample is blocked
        iff something is hit, whichever walk finds it."""
        if mode == sa.MODE_BRUTE:
            return self.brute, ptm.TRACE_ROOT_TREE
        if mode == sa.MODE_REF_TREE or shadows:
            return self.o, ptm.TRACE_ROOT_TREE
        return self.o, ptm.TRACE_NEAREST


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def as_sr(frame, mode, flags=0):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = mode
    f.flags |= flags
    return f


OMODE = {sa.MODE_BVH: orc.MODE_NEAREST, sa.MODE_BRUTE: orc.MODE_BRUTE, sa.MODE_REF_TREE: orc.MODE_REF_TREE}       # the oracle's mode for the library's


def structures(c):
    """(tag, scene, trace mode, stats) of every structure.  (stats=False: the shadow rays of a reference-tree frame run on the own BVH)"""
    return [("lbvh", c.scene("lbvh"), sa.MODE_BVH, True), ("sah", c.scene("sah"), sa.MODE_BVH, True), ("brute", c.scene("lbvh"), sa.MODE_BRUTE, True),
            ("tree", c.scene("tree"), sa.MODE_REF_TREE, True), ("tree, no statistics", c.scene("tree"), sa.MODE_REF_TREE, False)]


def check_kinds(c, kinds, size=RES, skip_brute=()):
    for kind in kinds:
        for tag, g, mode, stats in structures(c):
            if tag == "brute" and kind in skip_brute:
                continue
            want = c.want(kind, *size, omode=OMODE[mode])
            got, _ = g.render(as_sr(c.frame(kind, *size), mode), stats=stats)
            assert np.array_equal(got, want), (c.name, kind, tag, int((got != want).sum()))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, want):
    want = np.asarray(want).reshape(np.asarray(got).shape)
    return np.array_equal(bits(got), bits(want))


def same_hits(got, want, keys=KEYS):
    return all(same(got[k], want[k]) for k in keys)


# ---- 1. every frame kind on every structure ----
@pytest.mark.parametrize("name", mc.NAMES)
def test_shaded_and_shadow_frames(name):
    c = case(name)
    check_kinds(c, ("shaded", "soft", "inside", "directional", "rows"))
    check_kinds(c, ("soft",), size=ODD)
    assert not np.array_equal(c.want("soft"), c.want("shaded")) and not np.array_equal(c.want("inside"), c.want("soft"))


@pytest.mark.parametrize("name", mc.NAMES)
def test_sub_pixel_sampling_with_focal_blur(name):
    c = case(name)
    check_kinds(c, ("blur",), size=BLUR_RES, skip_brute=("blur",))     # (33 samples x 4 sub-pixels x every triangle: the own BVH and the tree only)


@pytest.mark.parametrize("name", mc.NAMES)
def test_mirror_bounces(name):
    c = case(name)
    check_kinds(c, ("mirror1", "mirror3"))
    assert not np.array_equal(c.want("mirror1"), c.want("shaded"))


@pytest.mark.parametrize("name", mc.NAMES)
def test_path_tracing(name):
    """Set up as tests/test_gpu_placement.py does: the CPU model of tests/pathtrace_model.py on the oracle's ray batches."""
    c = case(name)
    f = mc.frame(name, 80, 60, shading=True)
    f.flags |= ptm.F_PATH_TRACING
    want = ptm.render(c.o, f, ptm.TRACE_NEAREST)
    for structure in ("lbvh", "sah"):
        got, _ = c.scene(structure).render(as_sr(f, sa.MODE_BVH))
        assert np.array_equal(got.reshape(want.shape), want), (name, structure)
    for mode, scene in ((sa.MODE_REF_TREE, c.o), (sa.MODE_BRUTE, c.brute)):
        want = ptm.render(scene, f, ptm.TRACE_ROOT_TREE)
        got, _ = c.scene("tree").render(as_sr(f, mode))
        assert np.array_equal(got.reshape(want.shape), want), (name, mode)
    plain, _ = c.scene("lbvh").render(as_sr(mc.frame(name, 80, 60), sa.MODE_BVH))
    assert np.count_nonzero(plain.reshape(want.shape) != want) > 0                       # the second ray changed the image


# ---- 2. the schedules of the soft-shadow frame, and what the statistics say about them ----
def elsewhere(c, g):
    """A small frame from another camera and another light: the per-pose node copies and per-light records are made anew by the next
    frame, under whatever hook is set by then (some hooks speak only when a copy is made)."""
    f = c.frame("soft", 24, 16, light=mc.light_inside(c.lo, c.hi) * np.array([1.0, -1.0, 1.0]) + 0.05 * (c.hi - c.lo), yaw_deg=mc.SCENES[c.name]["pose"]["yaw_deg"] + 37.0)
    g.render(as_sr(f, sa.MODE_BVH), stats=False)


@pytest.mark.parametrize("which", LIGHT_CASES)
def test_soft_shadow_schedules(which):
    """Every schedule of the 117 x 91, 17-sample frame on the device LBVH equals the oracle.  At scale 1 pairs must be classified in fp32
    and a part of them, not none and not all, decided in FP64; for `fine` no expectation is fixed, as for the small placements.  The census of hook 94: every hit point is counted once; on `room_flush`, whose walls lie on the root box, hit points take
    the generic block; on `torus`, no triangle of which is near the box, all take the interior shortcut."""
    name, _, light_name = which.partition(":")
    light = mc.EDGE_ON_LIGHTS[light_name] if light_name else None
    c = case(name)
    g = c.scene("lbvh")
    want = c.want("soft", *ODD, light)
    f = as_sr(c.frame("soft", *ODD, light), sa.MODE_BVH)
    elsewhere(c, g)
    got, _ = g.render(f)
    st = g.ray_stats()
    print("mesh %-18s shadow rays [4] %d hit points [9] %d fp32 pairs [12] %d FP64 pairs [13] %d" % (which, st[4], st[9], st[12], st[13]))
    assert np.array_equal(got, want), (which, "default", int((got != want).sum()))
    assert np.array_equal(g.render(f, stats=False)[0], want), (which, "default, no statistics")
    assert st[4] > 0 and st[9] > 0
    if name in mc.SCALE_ONE:                                            # the fp32 classification ran, and handed the FP64 test a part of its pairs
        assert st[12] > 0 and 0 < st[13] < st[12], (which, st)
    assert np.array_equal(c.scene("sah").render(f)[0], want), (which, "sah")
    got, _ = g.render(as_sr(c.frame("soft", *ODD, light), sa.MODE_BVH, DBG.F_PER_LANE_SHADOWS))
    assert np.array_equal(got, want), (which, "SR_F_PER_LANE_SHADOWS", int((got != want).sum()))
    schedules = [((DBG.DBG_EXACT_SHADOW_TESTS, 1),), ((DBG.DBG_BVH2_PACKETS, 1),), ((DBG.DBG_LITERAL_SHADOWS, 1),)]
    schedules += [((DBG.DBG_PER_LANE_SHAFT, v),) for v in (0, 1, 2, 3)]
    schedules += [((DBG.DBG_PER_LANE_PRIMARY, v),) for v in (0, 1)]
    schedules += [((DBG.DBG_KERNEL_SWITCH, v),) for v in (93, 94, 96, 72, 61, 62, 97, 99)]
    schedules += [((DBG.DBG_ROUND_CAP0, 2), (DBG.DBG_ROUND_CAP1, 3))]
    for sched in schedules:
        try:
            for key, value in sched:
                g.debug_set(key, value)
            elsewhere(c, g)
            got, _ = g.render(f)
            st2, ctr = g.ray_stats(), g.debug_counters()
        finally:
            for key, _ in sched:
                g.debug_set(key, -1)
        assert np.array_equal(got, want), (which, sched, int((got != want).sum()))
        if sched[0] == (DBG.DBG_EXACT_SHADOW_TESTS, 1):
            assert st2[12] == 0
        if sched[0][0] == DBG.DBG_ROUND_CAP0:
            assert ctr[2] > 0 and ctr[3] > 0, (which, ctr)             # the second round and the exact fallback really ran
        if sched[0] == (DBG.DBG_KERNEL_SWITCH, 94):
            print("mesh %-18s census: hit points [9] %d shortcut [22] %d generic [23] %d" % (which, st2[9], st2[22], st2[23]))
            assert st2[9] > 0 and st2[22] + st2[23] == st2[9], (which, st2)
            if name == "room_flush":
                assert st2[23] > 0, (which, st2)
            if name == "torus":
                assert st2[22] == st2[9], (which, st2)
    elsewhere(c, g)
    assert np.array_equal(g.render(f)[0], want), (which, "default, after the hooks")


# ---- 3. the persistent shaft walk ----
@pytest.mark.parametrize("name", ["terrain", "room"])
def test_large_frame_on_the_persistent_shaft_walk(name):
    """512 x 384 under hook 831: the persistent form of the shaft walk; from the second frame on the tiles are walked longest first and
    try the umbra leaves the frame before left."""
    c = case(name)
    g = sa.GpuScene(0)                                                  # a scene of its own: the hook and the hints stay here
    g.set_triangles(c.v9, c.argb, c.lo, c.hi)
    g.build((sa.MODE_BVH,), on_device=True)
    want = c.want("soft", *BIG)
    f = as_sr(c.frame("soft", *BIG), sa.MODE_BVH)
    g.debug_set(DBG.DBG_KERNEL_SWITCH, 831)
    for turn in range(3):
        got, _ = g.render(f, stats=False)
        assert np.array_equal(got, want), (name, turn, int((got != want).sum()))
    ctr = g.debug_counters()
    assert ctr[6] > 0 and ctr[7] > 0, ctr                              # the persistent walk, in the longest-first order


_SEQUENCE = {}
LIGHT_SEQUENCE = ("in_plane", "straddle", "pierced", "in_plane")


@pytest.mark.parametrize("turn", range(len(LIGHT_SEQUENCE)), ids=["%d-%s" % t for t in enumerate(LIGHT_SEQUENCE)])
def test_light_sequence_on_the_persistent_shaft_walk(turn):
    """in_plane -> straddle -> pierced -> in_plane on ONE scene, a case per turn in pytest's order (each 512 x 384, 17-sample frame costs the
    oracle a few seconds): the per-light records, the light-ordered copy and the umbra hints of the frame before belong to another light
    each time.  A turn run alone is the first frame of a new scene: it equals the oracle too."""
    c = case("edge_on")
    if "scene" not in _SEQUENCE:
        g = sa.GpuScene(0)
        g.set_triangles(c.v9, c.argb, c.lo, c.hi)
        g.build((sa.MODE_BVH,), on_device=True)
        g.debug_set(DBG.DBG_KERNEL_SWITCH, 831)
        _SEQUENCE["scene"], _SEQUENCE["frames"] = g, 0
    g = _SEQUENCE["scene"]
    light = mc.EDGE_ON_LIGHTS[LIGHT_SEQUENCE[turn]]
    got, _ = g.render(as_sr(c.frame("soft", *BIG, light), sa.MODE_BVH), stats=False)
    _SEQUENCE["frames"] += 1
    want = c.want("soft", *BIG, light)
    assert np.array_equal(got, want), (turn, LIGHT_SEQUENCE[turn], int((got != want).sum()))
    ctr = g.debug_counters()
    assert ctr[6] > 0, ctr                                              # the persistent walk
    if _SEQUENCE["frames"] == len(LIGHT_SEQUENCE):
        assert ctr[7] > 0, ctr                                          # ... in the longest-first order an earlier frame left


# ---- 4. the G-buffer and ray batches at vertices and edge midpoints ----
@pytest.mark.parametrize("name", ["terrain", "edge_on"])
def test_gbuffer(name):
    """sr_render_hits: rays and hits of every camera sample, tri_index above all -- on edge_on the central pixel column and row travel in
    the planes of the central plates, and the plates' borders are ties between coplanar neighbours."""
    c = case(name)
    for size, sub in ((RES, 1), (BLUR_RES, 2)):
        f = c.frame("shaded", *size, sub_pixel_res=sub)
        for tag, g, mode, _ in structures(c)[:4]:
            scene, target = c.geometry(mode)
            starts, dirs, want = gbm.hits(scene, f, target)
            got = g.render_hits(as_sr(f, mode), rays=True)
            assert same(got["starts"], starts) and same(got["dirs"], dirs), (name, tag, sub)
            for k in KEYS:
                assert same(got[k], want[k]), (name, tag, sub, k, int((bits(got[k]).reshape(len(starts), -1) != bits(want[k]).reshape(len(starts), -1)).any(axis=1).sum()))
            assert 0.1 * len(starts) < got["hit"].sum() < 0.9 * len(starts)


def origin_device(g, target, origin, dirs, coherent):
    """sr_trace_origin_rays_device into torch buffers, read back."""
    n = dirs.shape[0]
    d_dirs = torch.from_numpy(dirs).to(DEV)
    bufs = {k: torch.zeros(n * ITEM[k][1] * np.dtype(ITEM[k][0]).itemsize, dtype=torch.uint8, device=DEV) for k in KEYS}
    torch.cuda.synchronize(DEV)
    g.trace_origin_device(target, origin, n, d_dirs.data_ptr(), coherent=coherent, **{"d_" + k: v.data_ptr() for k, v in bufs.items()})
    torch.cuda.synchronize(DEV)
    out = {}
    for k, b in bufs.items():
        a = b.cpu().numpy().view(ITEM[k][0])
        out[k] = a.reshape(-1, 3) if ITEM[k][1] == 3 else a
    return out


@pytest.mark.parametrize("name", sorted(mc.VERTEX_RAY_CASES))
def test_rays_at_vertices_and_edge_midpoints(name):
    """A ray at a mesh vertex ties every incident triangle at one rayFrac, a ray at an edge midpoint two: the lowest index wins, and
    where the reference's edge tests reject them all the ray goes through the crack -- on the device as in the oracle."""
    c = case(name)
    count = mc.VERTEX_RAY_CASES[name]
    for origin in mc.outside_origin(name):
        dirs, _ = mc.vertex_rays(name, origin, count)
        assert dirs.shape[0] == 2 * count
        starts = np.ascontiguousarray(np.tile(origin, (dirs.shape[0], 1)))
        for structure, mode, otarget in (("lbvh", sa.MODE_BVH, mc.TRACE_NEAREST), ("sah", sa.MODE_BVH, mc.TRACE_NEAREST),
                                         ("tree", sa.MODE_REF_TREE, mc.TRACE_TREE), ("tree", sa.MODE_BRUTE, mc.TRACE_BRUTE)):
            g = c.scene(structure)
            want = c.o.trace(otarget, starts, dirs)
            assert same_hits(g.trace(mode, starts, dirs), want), (name, structure, mode, "sr_trace_rays")
            for coherent in (False, True):
                assert same_hits(g.trace_origin(mode, origin, dirs, coherent=coherent), want), (name, structure, mode, coherent, "sr_trace_origin_rays")
                assert same_hits(origin_device(g, mode, origin, dirs, coherent), want), (name, structure, mode, coherent, "sr_trace_origin_rays_device")
        assert 0.5 * len(dirs) <= want["hit"].sum()


# ---- 5. the point calls on the mesh's vertices ----
POINT_SCENES = ("terrain", "torus", "fine", "room")
POINT_MODES = (("bvh", sa.MODE_BVH, 1536), ("tree", sa.MODE_REF_TREE, 1536), ("brute", sa.MODE_BRUTE, 384))


@pytest.mark.parametrize("name", POINT_SCENES)
def test_shadow_points_on_vertices(name):
    """sr_shadow_points and sr_static_shadow_points: a vertex's probe point pos + 0.001 n lies over every incident triangle's edge."""
    c = case(name)
    f = c.frame("soft")
    for tag, mode, limit in POINT_MODES:
        pos, nrm, col = c.vertex_points(limit)
        scene, target = c.geometry(mode, shadows=True)
        g = c.scene("tree")
        want = spm.shadowed(scene, f, pos, nrm, col, target)
        assert len(np.unique(want)) > 10
        for coherent in (False, True):
            assert same(g.shadow_points(as_sr(f, mode), pos, nrm, col, coherent=coherent), want), (name, tag, coherent)
        h = len(pos) // 2 + 3
        parts = [g.shadow_points(as_sr(f, mode), pos[a:b], nrm[a:b], col[a:b]) for a, b in ((0, h), (h, len(pos)))]
        assert same(np.concatenate(parts), want), (name, tag, "two calls")
        if tag == "bvh":
            assert same(c.scene("lbvh").shadow_points(as_sr(f, mode), pos, nrm, col), want), (name, "lbvh")
        cache = np.zeros(ssm.CELLS, dtype=np.uint8)
        w_amount, w_out, w_made = ssm.static_shadow_points(scene, f, pos, nrm, target, cache, col)
        for coherent in (False, True):
            g.reset_shadow_cache()
            out, amount, made = g.static_shadow_points(as_sr(f, mode), pos, nrm, col, coherent=coherent)
            assert made == w_made and same(amount, w_amount) and same(out, w_out), (name, tag, coherent, "static")
            assert same(g.get_shadow_cache().reshape(-1), cache)
        g.reset_shadow_cache()
        a = g.static_shadow_points(as_sr(f, mode), pos[:h], nrm[:h], col[:h])
        b = g.static_shadow_points(as_sr(f, mode), pos[h:], nrm[h:], col[h:])
        assert a[2] + b[2] == w_made and same(np.concatenate([a[0], b[0]]), w_out) and same(np.concatenate([a[1], b[1]]), w_amount), (name, tag, "static, two calls")
        g.reset_shadow_cache()


def points_frame(mode, flags=0, shading=False):
    f = sa.Frame.from_buffer_copy(bytes(make_frame(16, shading=shading)))
    f.trace_mode = mode
    f.random_seed = SEED
    f.flags |= flags
    return f


@pytest.mark.parametrize("name", POINT_SCENES)
def test_ao_points_on_vertices(name):
    """sr_ao_points, cached and with SR_F_AO_UNCACHED: 100 probes from pos + 0.001 n of every generator."""
    c = case(name)
    g = c.scene("tree")
    for tag, mode, limit in POINT_MODES:
        pos, nrm, col = c.vertex_points(limit // 3)
        scene, target = c.geometry(mode)
        for uncached in (False, True):
            cache = np.zeros(ssm.CELLS, dtype=np.uint8)
            w_amount, w_out, w_gen = apm.ao_points(scene, target, pos, nrm, SEED, cache, uncached=uncached, color=col)
            f = points_frame(mode, DBG.F_AO_UNCACHED if uncached else 0)
            g.reset_ao_cache()
            out, amount, gens = g.ao_points(f, pos, nrm, col)
            assert gens == w_gen and same(amount, w_amount) and same(out, w_out), (name, tag, uncached)
            if not uncached:
                assert same(g.get_ao_cache().reshape(-1), cache)
            g.reset_ao_cache()
            h = len(pos) // 2 + 3
            a = g.ao_points(f, pos[:h], nrm[:h], col[:h])
            b = g.ao_points(f, pos[h:], nrm[h:], col[h:], first_generator=a[2])
            assert a[2] + b[2] == w_gen and same(np.concatenate([a[0], b[0]]), w_out) and same(np.concatenate([a[1], b[1]]), w_amount), (name, tag, uncached, "two calls")
    g.reset_ao_cache()


@pytest.mark.parametrize("name", POINT_SCENES)
def test_path_points_on_vertices(name):
    """sr_path_points: the bounce ray starts at pos + 0.001 n, over the edges of the vertex's triangles."""
    c = case(name)
    g = c.scene("tree")
    for tag, mode, limit in POINT_MODES:
        pos, nrm, col = c.vertex_points(limit)
        scene, target = c.geometry(mode)
        for shading in (False, True):
            f = points_frame(mode, shading=shading)
            info = {}
            want = ppm.path_points(scene, target, f, pos, nrm, col, info=info)
            got = g.path_points(f, pos, nrm, col)
            assert all(same(a, b) for a, b in zip(got, want)), (name, tag, shading)
            h = len(pos) // 2 + 3
            a = g.path_points(f, pos[:h], nrm[:h], col[:h])
            b = g.path_points(f, pos[h:], nrm[h:], col[h:], first_sample=h)
            assert all(same(np.concatenate([x, y]), w) for x, y, w in zip(a, b, want)), (name, tag, shading, "two calls")
        assert info["hit"].any()
        if tag == "bvh":
            assert all(same(a, b) for a, b in zip(c.scene("lbvh").path_points(f, pos, nrm, col), want)), (name, "lbvh")


# ---- 6. dynamic geometry: the height field moves ----
def test_refit_height_field():
    """terrain fed through sr_set_triangles_device, then refit to the heights of a second function (x and z stay): the soft frame and the
    vertex-ray batch equal a scene built from scratch on the moved mesh, and the oracle."""
    c = case("terrain")
    moved = Case("terrain", mc.terrain(second=True))
    assert np.array_equal(moved.v9[:, :, (0, 2)], c.v9[:, :, (0, 2)]) and not np.array_equal(moved.v9[:, :, 1], c.v9[:, :, 1])
    g = sa.GpuScene(0)
    g.set_triangles_device(torch.from_numpy(c.v9.copy()).to(DEV), torch.from_numpy(c.argb.view(np.int32).copy()).to(DEV), c.lo, c.hi)
    g.build((sa.MODE_BVH,), on_device=True)
    f = c.frame("soft", *ODD)
    assert np.array_equal(g.render(as_sr(f, sa.MODE_BVH))[0], c.want("soft", *ODD))
    g.refit_triangles_device(torch.from_numpy(moved.v9).to(DEV), None, c.lo, c.hi)
    torch.cuda.synchronize(DEV)
    want = moved.want("soft", *ODD)
    assert not np.array_equal(want, c.want("soft", *ODD))
    scratch = moved.scene("lbvh")
    for turn in range(2):
        got, _ = g.render(as_sr(f, sa.MODE_BVH))
        assert np.array_equal(got, want), ("refit", turn, int((got != want).sum()))
    assert np.array_equal(scratch.render(as_sr(f, sa.MODE_BVH))[0], want)
    origin = mc.outside_origin("terrain")[0]
    verts, idx = mc.mesh_vertices(moved.v9)
    pick = (np.arange(2048) * len(verts)) // 2048
    corners = moved.v9.reshape(-1, 3)
    mids = 0.5 * (corners[0::3] + corners[1::3])[(np.arange(2048) * len(moved.v9)) // 2048]
    dirs = np.ascontiguousarray(np.concatenate([verts[pick] - origin, mids - origin]))
    starts = np.ascontiguousarray(np.tile(origin, (dirs.shape[0], 1)))
    model = moved.o.trace(mc.TRACE_NEAREST, starts, dirs)
    for coherent in (False, True):
        got = g.trace_origin(sa.MODE_BVH, origin, dirs, coherent=coherent)
        assert same_hits(got, model) and same_hits(got, scratch.trace_origin(sa.MODE_BVH, origin, dirs, coherent=coherent)), coherent
    assert same_hits(g.trace(sa.MODE_BVH, starts, dirs), model)
    assert model["hit"].sum() > len(dirs) // 2
