"""The colour light field with dynamic soft shadows (sr_set_light_field_shadows + SR_F_LIGHT_FIELD | SR_F_SHADOWS) on the device, frames and
bakes, against the golden of the reference's active test RaytraceLightField_Colors and the CPU model (tests/lightfield_shadow_model.py) --
bit for bit: every comparison is an exact equality over every pixel and every table entry.  The frames are those of
lightfield_shadow_model.gpu_frames(), whose input conditions tests/test_lightfield_shadow_model.py checks on the CPU."""
import os
import subprocess

import numpy as np
import pytest

import lightfield_bake as lfb
import lightfield_model as lfm
import lightfield_shadow_model as lsm
import softray_amd as sa
from helpers import GOLDEN, ROOT, load_obj3ds, orc, read_bmp_rgb, unit_cube_scene

pytestmark = pytest.mark.gpu
MODES = {"tree": sa.MODE_REF_TREE, "brute": sa.MODE_BRUTE, "bvh": sa.MODE_BVH}
UNTOUCHED = 0x01020304
FRAMES = lsm.gpu_frames()


def target_of(mode):
    return lfm.TRACE_NEAREST if mode == "bvh" else lfm.TRACE_ROOT_TREE


def as_sr(frame, mode, extra_flags=0):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = MODES[mode]
    f.flags |= extra_flags
    return f


def gpu_rows(g, frame, mode, extra_flags=0):
    """The frame's rows start_row..end_row as the library renders them and the four statistics; the other rows must stay untouched."""
    f = as_sr(frame, mode, extra_flags)
    out = np.full(f.width * f.height, UNTOUCHED, dtype=np.uint32)
    _, stats = g.render(f, out=out, stats=True)
    a = min(max(0, f.start_row), f.height - 1)
    b = min(max(0, f.end_row), f.height - 1)
    px = out.reshape(f.height, f.width)
    assert np.all(px[:a] == UNTOUCHED) and np.all(px[b + 1:] == UNTOUCHED)
    return px[a:b + 1].copy(), stats


def pair(model, prims=(), modes=(sa.MODE_REF_TREE, sa.MODE_BVH), on_device=None, devices=None):
    g, o = (sa.GpuScene(devices=devices) if devices else sa.GpuScene(0)), orc.Scene()
    for s in (g, o):
        s.set_triangles(*(unit_cube_scene(2000) if model == "unit_cube_2000" else load_obj3ds(model)))
        if prims:
            s.set_extra(list(prims))
    g.build(tuple(modes), on_device=on_device)
    assert o.build_tree() == 0
    g.light_field_shadows = True
    return g, o


@pytest.fixture(scope="module")
def obj_pair():
    g, o = pair("obj.3ds")
    assert g.bvh_stats()[3] == 1
    return g, o


@pytest.fixture(scope="module")
def obj_host_bvh():
    g, _ = pair("obj.3ds", modes=(sa.MODE_BVH,), on_device=False)
    assert g.bvh_stats()[3] == 0
    return g


@pytest.fixture(scope="module")
def tables(obj_pair):
    """The model's whole shadowed tables of obj.3ds, each computed once: (N, frame key, target) -> uint32 [4 N^4], read-only."""
    made = {}

    def get(n, frame, target, key=None):
        key = (n, key if key is not None else bytes(frame), target)
        if key not in made:
            m = lsm.LightFieldShadowModel(n)
            index = np.arange(lfm.cache_entries(n), dtype=np.int64)
            m.fill(obj_pair[1], frame, index, target)
            t = m.entries(index)
            t.setflags(write=False)
            made[key] = t
        return made[key]
    return get


def bake_frame(shading=True, **kw):
    return lsm.shadow_frame(lfb.bake_frame(shading, **kw))


def same_cache(g, model):
    got = g.get_light_field()
    assert got.size == lfm.cache_entries(model.n)
    filled = np.flatnonzero(got)
    want = np.array(sorted(model.cache), dtype=np.int64)
    return filled.size == want.size and np.array_equal(filled, want) and np.array_equal(got[filled], model.entries(want))


def start(g, n):
    g.light_field_res = n
    g.reset_light_field()
    return lsm.LightFieldShadowModel(n)


def check(g, o, model, frame, mode, extra_flags=0, whole_cache=True):
    """One frame on the scene's and the model's running caches: pixels, the four statistics, the canonical rays and the whole cache."""
    want = model.render(o, frame, target_of(mode))
    assert model.coord_margin > lfm.MARGIN and model.term_margin > lfm.MARGIN
    got, stats = gpu_rows(g, frame, mode, extra_flags)
    assert got.shape == want.shape and int(np.count_nonzero(got != want)) == 0
    assert [int(x) for x in stats] == [want.size * frame.sub_pixel_res ** 2, 0, 0, 0]
    rs = g.ray_stats()
    assert int(rs[4]) >= model.filled.size                                       # the canonical rays + what the shadow stage counts
    if model.filled.size == 0:
        assert not rs[4:8].any()
    if whole_cache:
        assert same_cache(g, model)
    return got


def bake(g, frame, mode, first=0, count=None, extra_flags=0):
    filled = g.bake_light_field(as_sr(frame, mode, extra_flags), first, count)
    return filled, [int(x) for x in g.ray_stats()[:8]]


# ---- 1. the reference's active golden, from an empty table ----
@pytest.mark.parametrize("mode", ["tree", "brute", "bvh"])
def test_golden_from_an_empty_table(obj_pair, mode):
    g, o = obj_pair
    _, _, n, f = FRAMES["golden"]
    model = start(g, n)
    got = check(g, o, model, f, mode)
    want = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", lsm.GOLDEN_NAME + ".bmp"))
    assert int(np.count_nonzero((got & 0xFFFFFF) != want)) == 0
    assert model.filled.size == 14937


# ---- 2. ... and from a table baked with shadows: the frame fills nothing ----
def test_golden_from_a_baked_table(obj_pair):
    g, o = obj_pair
    _, _, n, f = FRAMES["golden"]
    start(g, n)
    total = lfm.cache_entries(n)
    filled, rs = bake(g, f, "bvh")
    assert filled == total and rs[:4] == [0, 0, 0, 0] and rs[4] > total
    got, _ = gpu_rows(g, f, "bvh")
    want = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", lsm.GOLDEN_NAME + ".bmp"))
    assert int(np.count_nonzero((got & 0xFFFFFF) != want)) == 0
    assert not g.ray_stats()[4:8].any()                                          # no cell was filled
    # the entries the golden's samples read are the model's
    model = lsm.LightFieldShadowModel(n)
    model.render(o, f, lfm.TRACE_NEAREST)
    cells = np.array(sorted(model.cache), dtype=np.int64)
    table = g.get_light_field()
    assert np.array_equal(table[cells], model.entries(cells)) and np.all(table != 0)
    g.reset_light_field()


def test_cpp_mirror_reproduces_the_golden(tmp_path):
    exe = str(tmp_path / "lightfield_shadow_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "lightfield_shadow_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL OK" in r.stdout
    for line in ("empty table: %s diff=0" % lsm.GOLDEN_NAME, "baked table: %s diff=0" % lsm.GOLDEN_NAME, "second bake fills 0 ok",
                 "switch off, Render refused ok", "switch on, static shadows refused ok"):
        assert line in r.stdout


# ---- 3. the frames of tests/test_gpu_lightfield.py, with shadows ----
FRAME_CASES = [("view0_n8", "tree"), ("view0_n8", "brute"), ("view0_n8", "bvh"), ("small_blur", "tree"), ("small_blur", "bvh"),
               ("far_primitives", "tree"), ("far_primitives", "brute"),     # (the oracle's nearest-hit target has no extra geometry)
               ("unit_cube", "tree"), ("unit_cube", "bvh"), ("inside_sphere", "tree"), ("inside_sphere", "bvh")]
_pairs = {}


@pytest.mark.parametrize("name,mode", FRAME_CASES)
def test_frame(name, mode):
    model_file, prims, n, f = FRAMES[name]
    key = (model_file, bool(prims))
    if key not in _pairs:
        _pairs[key] = pair(model_file, prims=prims, modes=(sa.MODE_REF_TREE,) if prims else (sa.MODE_REF_TREE, sa.MODE_BVH))
    g, o = _pairs[key]
    model = start(g, n)
    got = check(g, o, model, f, mode)
    assert model.filled.size > 20
    plain = lfm.LightFieldModel(n)
    assert int(np.count_nonzero(plain.render(o, f, target_of(mode)) != got)) > 0     # the shadows are in it
    if name == "far_primitives":
        assert got.shape == (13, 37)


# ---- 4. two and more row bands ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_row_bands(obj_pair, mode):
    g, o = obj_pair
    _, _, n, f = FRAMES["view1_n8"]
    model = start(g, n)
    try:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, 64 * 4 * 16)                      # 16 rows per band: three bands
        check(g, o, model, f, mode)
    finally:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, -1)
    assert model.filled.size > 10


# ---- 5. a warm table: the second view fills only its new cells; 6. the claim bits are clear afterwards ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_warm_second_view_and_clear_claim_bits(obj_pair, mode):
    g, o = obj_pair
    _, _, n, f0 = FRAMES["view0_n8"]
    model = start(g, n)
    first = check(g, o, model, f0, mode)
    cells0 = model.filled.copy()
    again = check(g, o, model, f0, mode)                                         # identical frame: nothing is claimed, nothing is filled
    assert model.filled.size == 0 and np.array_equal(first, again)
    check(g, o, model, FRAMES["view2_n8"][3], mode)
    assert 0 < model.filled.size and not np.intersect1d(model.filled, cells0).size
    g.reset_light_field()                                                        # a reset, then the frame: the same cells again
    model.reset()
    check(g, o, model, f0, mode)
    assert np.array_equal(model.filled, cells0)


# ---- 7. whole baked tables ----
@pytest.mark.parametrize("shading", [False, True], ids=["noShading", "shading"])
@pytest.mark.parametrize("mode", ["tree", "brute", "bvh_host", "bvh_device"])
@pytest.mark.parametrize("n", [1, 2, 4, 8, 12])
def test_whole_table(obj_pair, obj_host_bvh, tables, n, mode, shading):
    g = obj_host_bvh if mode == "bvh_host" else obj_pair[0]
    mode = "bvh" if mode.startswith("bvh") else mode
    start(g, n)
    total = lfm.cache_entries(n)
    f = bake_frame(shading)
    filled, rs = bake(g, f, mode)
    assert filled == total and rs[:4] == [0, 0, 0, 0]
    want = tables(n, f, target_of(mode), key=("bake", shading))
    got = g.get_light_field()
    assert got.size == total and int(np.count_nonzero(got != want)) == 0
    if n == 1:
        assert got.tolist() == [lfb.BACKGROUND] * 4 and rs[4:8] == [0, 0, 0, 0]
    else:
        hits = lfb.NON_BACKGROUND[("obj.3ds", n)][0]
        assert int(np.count_nonzero(got != lfb.BACKGROUND)) == hits and rs[4] >= total
        plain = lfb.model_table(obj_pair[1], lfb.bake_frame(shading), n, target_of(mode))
        assert int(np.count_nonzero(got != plain)) == hits                       # every hit's colour is shadowed
    assert bake(g, f, mode) == (0, [0] * 8)                                      # nothing left


# ---- 8. ranges; entries that are there already survive and cost nothing ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_ranges_and_existing_entries(obj_pair, tables, mode):
    g, n = obj_pair[0], 8
    total = lfm.cache_entries(n)
    f = bake_frame(True)
    want = tables(n, f, target_of(mode), key=("bake", True))
    start(g, n)
    done = np.zeros(total, dtype=bool)
    for first, last in ((5001, 11000), (0, 5001), (11000, total)):
        filled, _ = bake(g, f, mode, first, last - first)
        assert filled == last - first
        done[first:last] = True
        got = g.get_light_field()
        assert not got[~done].any() and np.array_equal(got[done], want[done])
    assert np.array_equal(g.get_light_field(), want)
    g.reset_light_field()
    where = (np.arange(1000, dtype=np.int64) * 16381 + 7) % total
    mine = (np.arange(1000, dtype=np.uint32) + np.uint32(0x00010001))
    table = np.zeros(total, dtype=np.uint32)
    table[where] = mine
    g.set_light_field(table)
    filled, _ = bake(g, f, mode)
    assert filled == total - 1000
    mixed = want.copy()
    mixed[where] = mine
    assert np.array_equal(g.get_light_field(), mixed)
    assert bake(g, f, mode) == (0, [0] * 8)


# ---- 9. pass boundaries: the hook shrinks a pass to 7 origin patches (896 cells), 19 passes for N = 8 ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_bake_pass_boundaries(obj_pair, tables, mode):
    g, n = obj_pair[0], 8
    f = bake_frame(True)
    start(g, n)
    try:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, 1000)
        filled, rs = bake(g, f, mode, 3, lfm.cache_entries(n) - 5)
    finally:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, -1)
    assert filled == lfm.cache_entries(n) - 5
    want = tables(n, f, target_of(mode), key=("bake", True)).copy()
    want[:3] = 0
    want[-2:] = 0
    assert np.array_equal(g.get_light_field(), want)


# ---- 10. the shadow stage's schedules give the same bytes ----
def test_shadow_schedules(obj_pair, tables):
    g, n = obj_pair[0], 8
    f = bake_frame(True)
    lib = sa._lib
    cases = [("bvh", 0, None), ("bvh", lib.F_PER_LANE_SHADOWS, None), ("tree", 0, None), ("tree", lib.F_LITERAL_SECONDARY, None),
             ("tree", lib.F_PER_LANE_SHADOWS, None), ("bvh", 0, lib.DBG_EXACT_SHADOW_TESTS), ("bvh", lib.F_NO_SPLIT, None), ("bvh", 0, lib.DBG_PER_LANE_SHAFT)]
    for mode, flags, hook in cases:
        start(g, n)
        try:
            if hook is not None:
                g.debug_set(hook, 3 if hook == lib.DBG_PER_LANE_SHAFT else 1)
            filled, _ = bake(g, f, mode, extra_flags=flags)
        finally:
            if hook is not None:
                g.debug_set(hook, -1)
        assert filled == lfm.cache_entries(n)
        assert np.array_equal(g.get_light_field(), tables(n, f, target_of(mode), key=("bake", True))), (mode, flags, hook)
    # and a frame under each flag
    o = obj_pair[1]
    for mode, flags in (("bvh", lib.F_PER_LANE_SHADOWS), ("tree", lib.F_LITERAL_SECONDARY), ("bvh", lib.F_NO_SPLIT)):
        check(g, o, start(g, n), FRAMES["view0_n8"][3], mode, extra_flags=flags)
    try:                                                                         # the fill's shadow stage with the packet shaft walk (hook 36)
        g.debug_set(lib.DBG_KERNEL_SWITCH, 36)
        for mode in ("tree", "bvh"):
            check(g, o, start(g, 64), FRAMES["golden"][3], mode)
    finally:
        g.debug_set(lib.DBG_KERNEL_SWITCH, -1)


# ---- 11. sample counts (130: the accum chunks) and a directional light ----
@pytest.mark.parametrize("name", ["samples_1", "samples_17", "samples_100", "samples_130", "directional"])
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_sample_counts_and_directional_light(obj_pair, name, mode):
    g, o = obj_pair
    _, _, n, f = FRAMES[name]
    check(g, o, start(g, n), f, mode)
    # the whole table too: thousands of hit points, not the frame's 22 cells
    start(g, n)
    filled, _ = bake(g, f, mode)
    m = lsm.LightFieldShadowModel(n)
    index = np.arange(lfm.cache_entries(n), dtype=np.int64)
    m.fill(o, f, index, target_of(mode))
    assert filled == index.size and np.array_equal(g.get_light_field(), m.entries(index))


# ---- 12. refusals with the switch on leave the surface and the table untouched; switch off: the old refusal ----
def test_refusals_leave_surface_and_table_untouched(obj_pair):
    g, n = obj_pair[0], 8
    start(g, n)
    good = bake_frame(True)
    assert bake(g, good, "tree", 0, 6000)[0] == 6000
    before = g.get_light_field()

    def refused(f, text):
        out = np.full(f.width * f.height, UNTOUCHED, dtype=np.uint32)
        for call in (lambda: g.render(f, out=out), lambda: g.bake_light_field(f)):
            with pytest.raises(sa.SoftrayError) as e:
                call()
            assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED and text in str(e.value)
        assert np.all(out == UNTOUCHED) and np.array_equal(g.get_light_field(), before)

    for change in lfm.REFUSED[1:]:
        refused(lfm.apply_change(as_sr(good, "tree"), change), "light field")
    try:
        g.light_field_shadows = False
        refused(as_sr(good, "tree"), "light field together with shadows (dynamic or static) is not supported")
    finally:
        g.light_field_shadows = True
    assert np.array_equal(g.get_light_field(), before)                           # the switch does not touch the table


# ---- 13. a multi-device scene renders and bakes on its first device ----
def test_multi_device_scene(obj_pair, tables):
    g, o = obj_pair
    n = 8
    gm, _ = pair("obj.3ds", devices=[0, 0])
    assert gm.light_field_shadows is True
    gm.light_field_res = n
    model = lsm.LightFieldShadowModel(n)
    check(gm, o, model, FRAMES["view0_n8"][3], "bvh")
    assert gm.last_frame_parts() == 1
    gm.reset_light_field()
    f = bake_frame(True)
    assert gm.bake_light_field(as_sr(f, "bvh")) == lfm.cache_entries(n)
    assert np.array_equal(gm.get_light_field(), tables(n, f, lfm.TRACE_NEAREST, key=("bake", True)))


# ---- 14. statistics ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_primary_stats_only_leaves_the_secondary_counters_zero(obj_pair, tables, mode):
    g, o = obj_pair
    n = 8
    _, _, _, f = FRAMES["view0_n8"]
    model = start(g, n)
    check(g, o, model, f, mode)
    loud = [int(x) for x in g.ray_stats()[:8]]
    assert loud[4] >= model.filled.size > 0 and loud[5] > 0                     # canonical rays + what the shadow stage counts
    table = g.get_light_field()
    g.reset_light_field()
    got, stats = gpu_rows(g, f, mode, sa._lib.F_PRIMARY_STATS_ONLY)
    assert [int(x) for x in g.ray_stats()[:8]] == [got.size * 4, 0, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(g.get_light_field(), table)
    g.reset_light_field()
    bf = bake_frame(True)
    filled, rs = bake(g, bf, mode, extra_flags=sa._lib.F_PRIMARY_STATS_ONLY)
    assert filled == lfm.cache_entries(n) and rs == [0] * 8
    assert np.array_equal(g.get_light_field(), tables(n, bf, target_of(mode), key=("bake", True)))


def test_switch_without_the_flag_runs_the_plain_light_field(obj_pair):
    """Switch on, no SR_F_SHADOWS: the frame and the bake are the unshadowed ones."""
    g, o = obj_pair
    _, _, n, f = lfm.gpu_frame("view0_n8")
    g.light_field_res = n
    g.reset_light_field()
    model = lfm.LightFieldModel(n)
    want = model.render(o, f, lfm.TRACE_NEAREST)
    got, _ = gpu_rows(g, f, "bvh")
    assert np.array_equal(got, want) and int(g.ray_stats()[4]) == model.filled.size
    g.reset_light_field()
    assert bake(g, lfb.bake_frame(True), "bvh")[1][4] == lfm.cache_entries(n)
    assert np.array_equal(g.get_light_field(), lfb.model_table(o, lfb.bake_frame(True), n, lfm.TRACE_NEAREST))
