"""Frames on models away from the origin-centred unit cube (tests/placement_cases.py): the HIP path against the oracle run on the same
PLACED arrays, bit for bit -- every comparison is np.array_equal on whole frames.  Per placement: every frame kind (shaded, soft
shadows, sub-pixel sampling with focal blur, a light inside the box, a directional light, mirror bounces, path tracing, a row range)
on every structure (device-built LBVH, host SAH, the reference tree with and without statistics, brute force), the schedules of the
soft-shadow frame, scenes fed from device memory, and extra geometry.  The ray statistics say that the fp32 classification really ran
([12] pairs classified in fp32, [13] pairs it handed to the FP64 test) and which block of it took the hit points ([22] / [23]).

tests/test_placement_cases.py shows on the oracle alone that no placement is vacuous."""
import os

import numpy as np
import pytest
import torch

import pathtrace_model as ptm
import placement_cases as pc
import softray_amd as sa
from helpers import orc

pytestmark = pytest.mark.gpu
NCPU = min(16, os.cpu_count() or 8)
DBG = sa._lib
RES, ODD, BLUR_RES = (96, 80), (117, 91), (72, 56)        # 117 x 91: partial 8 x 8 tiles on both axes
SAMPLES = 17
_CASES = {}


class Case:
    """One placement: the placed arrays, the oracle's scene and its frames (each rendered once), the library's scenes by structure."""

    def __init__(self, name):
        self.name = name
        self.v9, self.argb, self.lo, self.hi = pc.placed(name)
        self.o = orc.Scene()
        self.o.set_triangles(self.v9, self.argb, self.lo, self.hi)
        self.tree = name in pc.HAS_TREE
        assert self.o.build_tree() == (0 if self.tree else -2)
        self.omode = orc.MODE_REF_TREE if self.tree else orc.MODE_NEAREST
        self.tables = {n: pc.offset_table(name, n) for n in (SAMPLES, 33)}          # kept alive: frames point at them
        self.scenes, self.wanted = {}, {}

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

    def frame(self, kind, w=RES[0], h=RES[1], omode=None):
        soft = dict(shadows=True, shadow_samples=SAMPLES, table=self.tables[SAMPLES])
        kw = {"shaded": dict(),
              "soft": soft,
              "blur": dict(shadows=True, shadow_samples=33, table=self.tables[33], sub_pixel_res=2, focal_blur=True),
              "inside": dict(soft, light_model=pc.light_inside(self.lo, self.hi)),
              "directional": dict(shadows=True, point_light=False),
              "directional_lit": dict(point_light=False),
              "mirror1": dict(), "mirror3": dict(),
              "rows": dict(soft, start_row=11, end_row=h - 23)}[kind]
        f = pc.frame(self.name, w, h, mode=self.omode if omode is None else omode, **kw)
        if kind.startswith("mirror"):
            f.max_bounces, f.reflectivity = int(kind[-1]), 0.5
        return f

    def want(self, kind, w=RES[0], h=RES[1], omode=None):
        """The oracle's frame; omode: its trace mode when not the placement's (brute force where the two differ)."""
        if (kind, w, h, omode) not in self.wanted:
            self.wanted[kind, w, h, omode] = self.o.render(self.frame(kind, w, h, omode), threads=NCPU)[0]
        return self.wanted[kind, w, h, omode]


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def as_sr(frame, mode):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = mode
    return f


def structures(c):
    """(tag, scene, trace mode, stats) of every structure the placement has."""
    out = [("lbvh", c.scene("lbvh"), sa.MODE_BVH, True), ("sah", c.scene("sah"), sa.MODE_BVH, True), ("brute", c.scene("lbvh"), sa.MODE_BRUTE, True)]
    if c.tree:                                                          # stats=False: the shadow rays of a reference-tree frame run on the own BVH
        out += [("tree", c.scene("tree"), sa.MODE_REF_TREE, True), ("tree, no statistics", c.scene("tree"), sa.MODE_REF_TREE, False)]
    return out


def check_kinds(c, kinds, size=RES, skip_brute=()):
    """Brute force tests every triangle wherever it lies, the own BVH and the oracle's nearest-hit mode only inside the root box: where
    triangles leave the box (`cut`) brute force has the oracle's brute-force frame as its yardstick, which costs the oracle 6000 tests
    per ray -- there its shadow frames are a quarter of the size."""
    for kind in kinds:
        for tag, g, mode, stats in structures(c):
            if tag == "brute" and kind in skip_brute:
                continue
            omode, sz = None, size
            if tag == "brute" and not c.tree:
                omode = orc.MODE_BRUTE
                if kind in ("soft", "inside", "rows"):
                    sz = (size[0] // 2, size[1] // 2)
            want = c.want(kind, *sz, omode)
            got, _ = g.render(as_sr(c.frame(kind, *sz), mode), stats=stats)
            assert np.array_equal(got, want), (c.name, kind, tag, int((got != want).sum()))


# ---- 1. every frame kind on every structure ----
@pytest.mark.parametrize("name", pc.NAMES)
def test_shaded_and_shadow_frames(name):
    c = case(name)
    check_kinds(c, ("shaded", "soft", "inside", "directional", "rows"))
    check_kinds(c, ("soft",), size=ODD)
    if name in pc.BLUR_AT:
        check_kinds(c, ("blur",), size=BLUR_RES, skip_brute=("blur",))  # (33 samples x 4 sub-pixels x every triangle: the own BVH and the tree only)
    if name == "big":                                                   # the directional light's 1000-unit start lies within the model's reach:
        assert not np.array_equal(c.want("directional"), c.want("directional_lit"))       # its samples do not all escape


@pytest.mark.parametrize("name", pc.NAMES)
def test_mirror_bounces(name):
    c = case(name)
    check_kinds(c, ("mirror1", "mirror3"))
    assert not np.array_equal(c.want("mirror1"), c.want("shaded")) and not np.array_equal(c.want("mirror3"), c.want("mirror1"))


@pytest.mark.parametrize("name", pc.NAMES)
def test_path_tracing(name):
    """Set up as tests/test_gpu_pathtrace.py does: the CPU model of tests/pathtrace_model.py on the oracle's ray batches."""
    c = case(name)
    f = pc.frame(name, 80, 60, shading=True)
    f.flags |= ptm.F_PATH_TRACING
    want = ptm.render(c.o, f, ptm.TRACE_NEAREST)
    for structure in ("lbvh", "sah"):
        got, _ = c.scene(structure).render(as_sr(f, sa.MODE_BVH))
        assert np.array_equal(got.reshape(want.shape), want), (name, structure)
    if c.tree:
        want = ptm.render(c.o, f, ptm.TRACE_ROOT_TREE)
        for mode in (sa.MODE_REF_TREE, sa.MODE_BRUTE):
            got, _ = c.scene("tree").render(as_sr(f, mode))
            assert np.array_equal(got.reshape(want.shape), want), (name, mode)
    plain, _ = c.scene("lbvh").render(as_sr(pc.frame(name, 80, 60), sa.MODE_BVH))
    assert np.count_nonzero(plain.reshape(want.shape) != want) > 0                       # the second ray changed the image


def test_the_reference_tree_refuses_the_cut_box():
    c = case("cut")
    g = sa.GpuScene(0)
    g.set_triangles(c.v9, c.argb, c.lo, c.hi)
    with pytest.raises(sa.SoftrayError) as e:
        g.build((sa.MODE_REF_TREE,))
    assert e.value.code == DBG.SR_ERR_OUT_OF_RANGE
    g.build((sa.MODE_BVH,))
    assert np.array_equal(g.render(as_sr(c.frame("soft"), sa.MODE_BVH))[0], c.want("soft"))
    brute = c.want("shaded", *RES, orc.MODE_BRUTE)                      # brute force ignores the box: the protruding parts show
    assert np.array_equal(g.render(as_sr(c.frame("shaded"), sa.MODE_BRUTE))[0], brute)
    assert not np.array_equal(brute, c.want("shaded"))


# ---- 2. the schedules of the soft-shadow frame, and what the statistics say about them ----
@pytest.mark.parametrize("name", pc.NAMES + pc.EXTRA)
def test_soft_shadow_schedules(name):
    """Every schedule of the 117 x 91, 17-sample frame on the device LBVH equals the oracle.  Where the scale is 1 or more and the box
    holds the model, pairs must be classified in fp32 and only a part of them decided in FP64.  At `small` and `tiny` no expectation is
    fixed: most / all probe points lie outside the box, where no pair is BLOCKED in fp32.  Figures of the default schedule on an MI355X
    (shadow rays [4], hit points [9], fp32 pairs [12], FP64 pairs [13]):
        origin     77009  5140   901335     54        near       79292  5088  1106280    115        far       132639  9065  1734101    187
        far_scaled 86736  5722  1679222    200        big        93935  6147   972869  46045        small       7492   522   166938   5728
        flat       20621  1213    17655     28        loose      77479  5170   901178    117        cut        31171  2053   516056   8894
        far_probe  77335  5170  1011538     56        far_limit  77300  5167  1010571     56        tiny        2686   171    64461  10478
    (`big`: the absolute 0.001 of the probe offset is 1e-6 of the box, so many more crossings lie within the margin of the surface point.)"""
    c = case(name)
    g = c.scene("lbvh")
    want = c.want("soft", *ODD)
    f = as_sr(c.frame("soft", *ODD), sa.MODE_BVH)
    got, _ = g.render(f)
    st = g.ray_stats()
    print("placement %-10s shadow rays [4] %d hit points [9] %d fp32 pairs [12] %d FP64 pairs [13] %d" % (name, st[4], st[9], st[12], st[13]))
    assert np.array_equal(got, want), (name, "default", int((got != want).sum()))
    assert np.array_equal(g.render(f, stats=False)[0], want), (name, "default, no statistics")
    if name in pc.FP32_MUST_RUN and st[4] > 0:
        assert st[12] > 0 and st[13] < st[12], (name, st)
    if name != "far" and name in pc.NAMES:                              # (the host's SAH tree: the same lists up to order)
        assert np.array_equal(c.scene("sah").render(f)[0], want), (name, "sah")
    schedules = [((DBG.DBG_EXACT_SHADOW_TESTS, 1),)]
    schedules += [((DBG.DBG_PER_LANE_SHAFT, v),) for v in (0, 1, 2, 3)]
    schedules += [((DBG.DBG_PER_LANE_PRIMARY, v),) for v in (0, 1)]
    schedules += [((DBG.DBG_BVH2_PACKETS, 1),), ((DBG.DBG_KERNEL_SWITCH, 93),), ((DBG.DBG_ROUND_CAP0, 2), (DBG.DBG_ROUND_CAP1, 3))]
    for sched in schedules:
        try:
            for key, value in sched:
                g.debug_set(key, value)
            got, _ = g.render(f)
            st2, ctr = g.ray_stats(), g.debug_counters()
        finally:
            for key, _ in sched:
                g.debug_set(key, -1)
        assert np.array_equal(got, want), (name, sched, int((got != want).sum()))
        if sched[0] == (DBG.DBG_EXACT_SHADOW_TESTS, 1):
            assert st2[12] == 0
        if sched[0][0] == DBG.DBG_ROUND_CAP0:
            assert ctr[2] > 0 and ctr[3] > 0, (name, ctr)              # the second round and the exact fallback really ran


@pytest.mark.parametrize("name", ["origin", "loose", "cut"])
def test_interior_shortcut_census(name):
    """SR_DBG_KERNEL_SWITCH 94: [22] hit points classified with the interior shortcut, [23] with the per-sample box exits.  In the loose
    box every triangle lies 0.6 or more inside every face (the margin is 1e-5 x 3): no list takes the generic block.  In the cut box
    4689 of the 6000 triangles have a vertex outside: lists with such a triangle take the generic block."""
    c = case(name)
    g = c.scene("lbvh")
    f = as_sr(c.frame("soft", *ODD), sa.MODE_BVH)
    try:
        g.debug_set(DBG.DBG_KERNEL_SWITCH, 94)
        got, _ = g.render(f)
        st = g.ray_stats()
    finally:
        g.debug_set(DBG.DBG_KERNEL_SWITCH, -1)
    print("placement %-10s census: hit points [9] %d shortcut [22] %d generic [23] %d" % (name, st[9], st[22], st[23]))
    assert np.array_equal(got, c.want("soft", *ODD))
    assert st[9] > 0 and st[22] + st[23] == st[9], (name, st)
    if name == "loose":
        assert st[22] == st[9] and st[23] == 0, (name, st)
    elif name == "cut":
        assert st[23] > 0, (name, st)
    else:
        assert st[22] > 0, (name, st)


@pytest.mark.parametrize("name", pc.BIG_FRAME_AT)
def test_large_frame_on_the_persistent_shaft_walk(name):
    """512 x 384: large enough for the persistent form of the shaft walk once its grid is one workgroup per CU (hook 831); from the
    second frame on the tiles are walked longest first."""
    v9, argb, lo, hi = pc.placed(name, 3000)
    g, o = sa.GpuScene(0), orc.Scene()
    for s in (g, o):
        s.set_triangles(v9, argb, lo, hi)
    g.build((sa.MODE_BVH,))
    assert o.build_tree() == 0
    table = pc.offset_table(name, SAMPLES)
    f = pc.frame(name, 512, 384, shadows=True, shadow_samples=SAMPLES, table=table)
    want, _ = o.render(f, threads=NCPU)
    g.debug_set(DBG.DBG_KERNEL_SWITCH, 831)
    for turn in range(3):
        got, _ = g.render(as_sr(f, sa.MODE_BVH))
        assert np.array_equal(got, want), (name, turn, int((got != want).sum()))
    ctr = g.debug_counters()
    assert ctr[6] > 0 and ctr[7] > 0, ctr                              # the persistent walk, in the longest-first order


# ---- 3. geometry fed from device memory ----
@pytest.mark.parametrize("name", pc.DEVICE_FED_AT)
def test_device_fed_geometry(name):
    """sr_set_triangles_device with the box passed as given.  The library offers no read-back of the vertex bounds its two reduction
    kernels make; what reads them is the directional light's "every sample escapes" proof (sr_api.cpp render_common), so a directional
    frame is compared too, as tests/test_gpu_device_geometry.py does."""
    c = case(name)
    dev = torch.device("cuda", 0)
    g = sa.GpuScene(0)
    g.set_triangles_device(torch.from_numpy(c.v9).to(dev), torch.from_numpy(c.argb.view(np.int32)).to(dev), c.lo, c.hi)
    g.build((sa.MODE_BVH,))
    for kind in ("soft", "directional", "inside"):
        got, _ = g.render(as_sr(c.frame(kind), sa.MODE_BVH))
        assert np.array_equal(got, c.want(kind)), (name, kind)
    r_v9, r_argb, r_lo, r_hi = g.get_triangles()
    assert np.array_equal(r_lo, c.lo) and np.array_equal(r_hi, c.hi)
    assert np.array_equal(r_v9.view(np.uint64), c.v9.view(np.uint64)) and np.array_equal(r_argb, c.argb)
    p = r_v9.reshape(-1, 3)
    inside = (p.min(axis=0) >= c.lo).all() and (p.max(axis=0) <= c.hi).all()
    assert inside == (name != "cut")                                    # cut: the vertex bounds are not the box
    if c.tree:
        g.build((sa.MODE_REF_TREE, sa.MODE_BVH))                        # (the reference tree reads the host copy fetched from the device)
        assert np.array_equal(g.render(as_sr(c.frame("soft"), sa.MODE_REF_TREE))[0], c.want("soft")), name


# ---- 4. extra geometry, mapped like the vertices ----
@pytest.mark.parametrize("name", pc.SPHERES_AT)
def test_extra_geometry(name):
    c = case(name)
    prims = pc.placed_spheres(name, 5)
    g, o = sa.GpuScene(0), orc.Scene()
    for s in (g, o):
        s.set_triangles(c.v9, c.argb, c.lo, c.hi)
        s.set_extra(prims)
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH))
    assert o.build_tree() == 0
    f = c.frame("soft")
    want, _ = o.render(f, threads=NCPU)
    assert not np.array_equal(want, c.want("soft"))                     # the spheres show
    for mode in (sa.MODE_BVH, sa.MODE_REF_TREE):
        got, _ = g.render(as_sr(f, mode))
        assert np.array_equal(got, want), (name, mode, int((got != want).sum()))
