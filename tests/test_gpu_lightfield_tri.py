"""The triangle-index light field (sr_set_light_field_triangles: rayTraceLightField with LightFieldStoresTriangles = true) on the device against the
CPU model (tests/lightfield_tri_model.py) -- bit for bit: every comparison is an exact equality over every pixel, every table entry and every
pinned statistic.  The frames are lightfield_tri_model.GPU_FRAMES_TRI, whose input conditions tests/test_lightfield_tri_model.py checks on the CPU.
The reference ignores its own test of this method (RendererTests.cs:217-220) and the model does not reproduce the stale goldens,
so the model is the yardstick."""
import os
import subprocess

import numpy as np
import pytest

import lightfield_model as lfm
import lightfield_tri_model as ltm
import softray_amd as sa
from helpers import GOLDEN, ROOT, orc

pytestmark = pytest.mark.gpu
MODES = {"tree": sa.MODE_REF_TREE, "brute": sa.MODE_BRUTE, "bvh": sa.MODE_BVH}
TARGET = {"tree": ltm.TRACE_TREE, "bvh": ltm.TRACE_NEAREST}
UNTOUCHED = 0x01020304
SPLIT = 43                                   # SR_DBG_KERNEL_SWITCH: stage 3 as a compact list for k_lft_trace instead of inside k_lft_hit


def as_sr(frame, mode):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = MODES[mode]
    return f


def gpu_rows(g, f):
    out = np.full(f.width * f.height, UNTOUCHED, dtype=np.uint32)
    _, stats = g.render(f, out=out, stats=True)
    a = min(max(0, f.start_row), f.height - 1)
    b = min(max(0, f.end_row), f.height - 1)
    px = out.reshape(f.height, f.width)
    assert np.all(px[:a] == UNTOUCHED) and np.all(px[b + 1:] == UNTOUCHED)
    return px[a:b + 1].copy(), [int(x) for x in stats]


@pytest.fixture(scope="module")
def scenes():
    """(model file, with extra geometry?) -> GpuScene with the reference tree and the own BVH, the triangle switch on; made once."""
    made = {}

    def get(model, prims=()):
        key = (model, bool(prims))
        if key not in made:
            g = sa.GpuScene(0)
            g.set_triangles(*ltm.model_data(model))
            if prims:
                g.set_extra(list(prims))
            g.build((sa.MODE_REF_TREE, sa.MODE_BVH))
            g.light_field_triangles = True
            made[key] = g
        return made[key]
    return get


@pytest.fixture(scope="module")
def oracles():
    made = {}
    return lambda model: made.setdefault(model, ltm.oracle_scene(model))


@pytest.fixture(scope="module")
def expected(oracles):
    """(frame name, mode) -> (pixels, table, statistics) of the model from an empty table; computed once, read-only."""
    made = {}

    def get(name, mode):
        if (name, mode) not in made:
            model, _, n, f = lfm.gpu_frame(name)
            m = ltm.LightFieldTriModel(*oracles(model), n=n)
            px = m.render(f, TARGET[mode])
            table = m.dense()
            px.setflags(write=False)
            table.setflags(write=False)
            made[(name, mode)] = (px, table, list(m.stats))
        return made[(name, mode)]
    return get


def fresh(g, n):
    g.light_field_res = n
    g.reset_light_field()


def pinned(stats, mode):
    """The statistics that are pinned in this mode: all of [0..7] and the census on the reference tree; on the own BVH the walks count what they fetch."""
    return stats[0:8] + stats[20:24] if mode == "tree" else [stats[0], stats[4]] + stats[20:24]


# ---- 1. every frame: from an empty table, again warm, and with stage 3 in a kernel of its own ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
@pytest.mark.parametrize("name", ltm.GPU_FRAMES_TRI)
def test_frames(scenes, expected, name, mode):
    model, prims, n, frame = lfm.gpu_frame(name)
    g = scenes(model, prims)                                 # (far_primitives: the extra geometry is there and must have no effect)
    want_px, want_table, want_stats = expected(name, mode)
    f = as_sr(frame, mode)
    for hook in (-1, SPLIT):
        fresh(g, n)
        try:
            g.debug_set(sa._lib.DBG_KERNEL_SWITCH, hook)
            got, stats4 = gpu_rows(g, f)
            rs = [int(x) for x in g.ray_stats()]
            assert np.array_equal(got, want_px)
            assert stats4 == rs[:4] and pinned(rs, mode) == pinned(want_stats, mode)
            assert np.array_equal(g.get_light_field_tris(), want_table)
            # warm: nothing is filled, the same samples take the same stages
            got, _ = gpu_rows(g, f)
            rs = [int(x) for x in g.ray_stats()]
            assert np.array_equal(got, want_px) and rs[4:8] == [0, 0, 0, 0]
            assert rs[0:4] + rs[20:24] == (want_stats[0:4] + want_stats[20:24] if mode == "tree" else rs[0:4] + want_stats[20:24])
            assert np.array_equal(g.get_light_field_tris(), want_table)
        finally:
            g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
    assert not g.get_light_field().any()                     # the colour table is never touched


def test_primary_stats_only(scenes, expected):
    model, prims, n, frame = lfm.gpu_frame("view0_n8")
    g = scenes(model)
    want_px, want_table, want_stats = expected("view0_n8", "tree")
    fresh(g, n)
    f = as_sr(frame, "tree")
    f.flags |= sa._lib.F_PRIMARY_STATS_ONLY
    got, _ = gpu_rows(g, f)
    rs = [int(x) for x in g.ray_stats()]
    assert np.array_equal(got, want_px) and rs[0:4] == want_stats[0:4] and not any(rs[4:8]) and not any(rs[20:24])
    assert np.array_equal(g.get_light_field_tris(), want_table)


# ---- 2. row bands and a row range ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_three_bands_and_a_row_range(scenes, oracles, expected, mode):
    model, prims, n, frame = lfm.gpu_frame("view1_n8")       # 64 x 48, 2 x 2 samples: bands of 16 rows
    g = scenes(model)
    want_px, want_table, want_stats = expected("view1_n8", mode)
    for hook in (-1, SPLIT):
        fresh(g, n)
        try:
            g.debug_set(sa._lib.DBG_BAND_SAMPLES, 1)
            g.debug_set(sa._lib.DBG_KERNEL_TIMING, 1)
            g.debug_set(sa._lib.DBG_KERNEL_SWITCH, hook)
            g.reset_kernel_times()
            got, _ = gpu_rows(g, as_sr(frame, mode))
            launches = {k: v[1] for k, v in g.kernel_times().items()}
        finally:
            g.debug_set(sa._lib.DBG_BAND_SAMPLES, -1)
            g.debug_set(sa._lib.DBG_KERNEL_TIMING, -1)
            g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
        assert launches["k_lf_lookup"] == launches["k_lft_fill"] == launches["k_lft_hit"] == 3
        assert launches.get("k_lft_trace", 0) == (3 if hook == SPLIT else 0)
        rs = [int(x) for x in g.ray_stats()]
        assert np.array_equal(got, want_px) and pinned(rs, mode) == pinned(want_stats, mode)
        assert np.array_equal(g.get_light_field_tris(), want_table)
    # a row range, from an empty table: the model's rows
    ranged = lfm.gpu_frame("view1_n8")[3]
    ranged.start_row, ranged.end_row = 7, 37
    m = ltm.LightFieldTriModel(*oracles(model), n=n)
    want = m.render(ranged, TARGET[mode])
    fresh(g, n)
    got, _ = gpu_rows(g, as_sr(ranged, mode))
    assert got.shape[0] == 31 and np.array_equal(got, want) and np.array_equal(g.get_light_field_tris(), m.dense())


# ---- 3. the bake ----
@pytest.fixture(scope="module")
def baked(oracles):
    """(N, mode) -> the model's whole table of obj.3ds; once."""
    made = {}

    def get(n, mode):
        if (n, mode) not in made:
            m = ltm.LightFieldTriModel(*oracles("obj.3ds"), n=n)
            m.bake(TARGET[mode])
            made[(n, mode)] = (m.dense(), list(m.stats))
            made[(n, mode)][0].setflags(write=False)
        return made[(n, mode)]
    return get


@pytest.mark.parametrize("mode", ["tree", "bvh"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_bake_whole_table(scenes, baked, n, mode):
    g = scenes("obj.3ds")
    want, want_stats = baked(n, mode)
    fresh(g, n)
    f = as_sr(lfm.gpu_frame("view0_n8")[3], mode)
    total = lfm.cache_entries(n)
    assert g.bake_light_field(f) == total
    rs = [int(x) for x in g.ray_stats()]
    assert rs[0:4] == [0, 0, 0, 0] and rs[4] == (0 if n == 1 else total) == want_stats[4]
    if mode == "tree":
        assert rs[5:8] == want_stats[5:8]
    got = g.get_light_field_tris()
    assert np.array_equal(got, want) and got.min() >= 1
    if n == 1:
        assert got.tolist() == [1] * 4
    assert g.bake_light_field(f) == 0                        # nothing is empty any more
    assert not g.get_light_field().any()


@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_bake_clipped_range_keeps_existing_entries(scenes, oracles, mode):
    n, first, count = 16, 70001, 4099                        # inside one origin patch row and across tile borders
    g = scenes("obj.3ds")
    fresh(g, n)
    keep = np.array([5, 0, 77, 0, 0, 9], dtype=np.uint32)    # non-zero entries survive, whatever they say
    g.set_light_field_tris(keep, first=first + 10)
    f = as_sr(lfm.gpu_frame("far_n16")[3], mode)
    assert g.bake_light_field(f, first, count) == count - 3
    m = ltm.LightFieldTriModel(*oracles("obj.3ds"), n=n)
    m.bake(TARGET[mode], first, count)
    want = m.dense()
    at = first + 10 + np.flatnonzero(keep)
    want[at] = keep[keep != 0]
    assert np.array_equal(g.get_light_field_tris(), want)
    assert not want[:first].any() and not want[first + count:].any()


@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_frame_from_the_baked_table_equals_the_lazy_frame(scenes, expected, mode):
    model, prims, n, frame = lfm.gpu_frame("view2_n8")
    g = scenes(model)
    want_px, _, want_stats = expected("view2_n8", mode)
    fresh(g, n)
    f = as_sr(frame, mode)
    assert g.bake_light_field(f) == lfm.cache_entries(n)
    table = g.get_light_field_tris()
    got, _ = gpu_rows(g, f)
    rs = [int(x) for x in g.ray_stats()]
    assert np.array_equal(got, want_px) and rs[4] == 0 and rs[20:24] == want_stats[20:24]
    assert np.array_equal(g.get_light_field_tris(), table)


# ---- 4. switch off: the colour light field is what it was, and the two tables do not touch each other ----
def test_switch_off_is_the_colour_light_field(scenes):
    model, prims, n, frame = lfm.gpu_frame("view0_n8")
    g = scenes(model)
    o = orc.Scene()
    o.set_triangles(*ltm.model_data(model))
    assert o.build_tree() == 0
    fresh(g, n)
    f = as_sr(frame, "tree")
    gpu_rows(g, f)                                           # the triangle table gets entries ...
    tris = g.get_light_field_tris()
    assert tris.any() and not g.get_light_field().any()
    try:
        g.light_field_triangles = False
        cm = lfm.LightFieldModel(n)
        want = cm.render(o, frame, lfm.TRACE_ROOT_TREE)
        got, stats4 = gpu_rows(g, f)
        assert np.array_equal(got, want) and stats4 == [want.size * 4, 0, 0, 0]
        assert np.array_equal(g.get_light_field(), cm.dense())
        assert np.array_equal(g.get_light_field_tris(), tris)      # ... which a colour frame leaves alone
    finally:
        g.light_field_triangles = True
    colours = g.get_light_field()
    gpu_rows(g, f)
    assert np.array_equal(g.get_light_field(), colours) and np.array_equal(g.get_light_field_tris(), tris)
    g.reset_light_field()                                    # both tables
    assert not g.get_light_field().any() and not g.get_light_field_tris().any()


# ---- 5. refusals ----
def test_refusals(scenes):
    g = scenes("obj.3ds")
    base = lfm.gpu_frame("contention")[3]

    def code(frame, call):
        with pytest.raises(sa.SoftrayError) as e:
            call(frame)
        return e.value.code

    try:
        g.light_field_shadows = True                         # the colour method's opt-in does not let shadows through the triangle method
        for call in (g.render, g.bake_light_field):
            for change in lfm.REFUSED:
                for mode in ("tree", "bvh"):
                    assert code(lfm.apply_change(as_sr(base, mode), change), call) == sa._lib.SR_ERR_UNSUPPORTED, (change, mode)
            assert code(as_sr(base, "brute"), call) == sa._lib.SR_ERR_UNSUPPORTED
    finally:
        g.light_field_shadows = False
    h = sa.GpuScene(0)
    h.set_triangles(*ltm.model_data("obj.3ds"))
    h.build((sa.MODE_BVH,))
    h.light_field_triangles = True
    for call in (h.render, h.bake_light_field):
        assert code(as_sr(base, "bvh"), call) == sa._lib.SR_ERR_NOT_BUILT        # the own BVH alone: stages 1 and 2 need the reference tree
        assert code(as_sr(base, "tree"), call) == sa._lib.SR_ERR_NOT_BUILT
    h.light_field_triangles = False
    h.light_field_res = 4
    h.render(as_sr(base, "bvh"))                             # switch off: the colour frame needs no reference tree


# ---- 6. what drops the table ----
def test_drops(scenes):
    import torch
    data = ltm.model_data("obj.3ds")
    g = sa.GpuScene(0)
    g.set_triangles(*data)
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=True)
    g.light_field_triangles = True
    g.light_field_res = 4
    f = as_sr(lfm.gpu_frame("contention")[3], "bvh")

    def filled():
        g.render(f)
        assert g.get_light_field_tris().any()

    filled()
    g.reset_light_field()
    assert not g.get_light_field_tris().any()
    filled()
    g.light_field_res = 5
    assert not g.get_light_field_tris().any() and g.get_light_field_tris().size == lfm.cache_entries(5)
    g.light_field_res = 4
    filled()
    g.build((sa.MODE_REF_TREE,), 9, 6)                       # another reference tree: the table stays
    assert g.get_light_field_tris().any()
    v9 = torch.tensor(np.asarray(data[0]).reshape(-1, 3, 3), dtype=torch.float64, device="cuda:0")
    g.refit_triangles_device(v9, None, data[2], data[3])
    torch.cuda.synchronize()
    assert not g.get_light_field_tris().any() and g.light_field_triangles is True
    with pytest.raises(sa.SoftrayError) as e:                # a refit drops the reference tree: nothing names handle leaves of the old one
        g.render(f)
    assert e.value.code == sa._lib.SR_ERR_NOT_BUILT
    g.build((sa.MODE_REF_TREE,))
    filled()
    g.set_triangles(*data)
    assert not g.get_light_field_tris().any() and g.light_field_triangles is True


# ---- 7. sr_render_device on a caller's stream ----
def test_render_device_on_a_caller_stream(scenes, expected):
    import torch
    model, prims, n, frame = lfm.gpu_frame("view2_n8")
    g = scenes(model)
    want_px, want_table, want_stats = expected("view2_n8", "bvh")
    fresh(g, n)
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        px = torch.full((frame.width * frame.height,), 0x01020304, dtype=torch.int32, device="cuda:0")
        st = torch.zeros(24, dtype=torch.int64, device="cuda:0")
        g.render_device(as_sr(frame, "bvh"), px.data_ptr(), stream.cuda_stream, st.data_ptr())
    stream.synchronize()
    assert np.array_equal(px.cpu().numpy().view(np.uint32).reshape(frame.height, frame.width), want_px)
    rs = [int(x) for x in st.cpu().numpy()]
    assert pinned(rs, "bvh") == pinned(want_stats, "bvh")
    assert np.array_equal(g.get_light_field_tris(), want_table)


# ---- 8. the C++ mirror ----
def test_cpp_mirror_opt_in(tmp_path):
    exe = str(tmp_path / "lightfield_tri_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "lightfield_tri_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL OK" in r.stdout
    for line in ("without the opt-in Render() names the switch ok", "without the opt-in BakeLightField() names the switch ok",
                 "triangle frame equals sr_render with the switch on: diff=0", "BakeLightField() equals sr_bake_light_field: filled equal, tables equal ok",
                 "frame from the baked table identical ok"):
        assert line in r.stdout
