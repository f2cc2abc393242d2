"""The colour light field (SR_F_LIGHT_FIELD, rayTraceLightField with LightFieldStoresTriangles = false) on the device against the reference's
goldens and the CPU model (tests/lightfield_model.py) -- bit for bit: every comparison is an exact equality over every pixel and every cache
entry.  Every frame rendered here is listed in lightfield_model.GPU_FRAMES, whose input conditions (no sample on a cell boundary or on the
sphere test's threshold) tests/test_lightfield_model.py checks on the CPU."""
import os
import subprocess

import numpy as np
import pytest

import lightfield_model as lfm
import softray_amd as sa
from helpers import GOLDEN, ROOT, load_obj3ds, make_frame, orc, read_bmp_rgb, unit_cube_scene

pytestmark = pytest.mark.gpu
MODES = {"tree": sa.MODE_REF_TREE, "brute": sa.MODE_BRUTE, "bvh": sa.MODE_BVH}
UNTOUCHED = 0x01020304
BACKGROUND = 0xFFFF00FF


def target_of(mode):
    return lfm.TRACE_NEAREST if mode == "bvh" else lfm.TRACE_ROOT_TREE


def as_sr(frame, mode):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = MODES[mode]
    return f


def gpu_rows(g, frame, mode, extra_flags=0):
    """The frame's rows start_row..end_row as the library renders them, [rows, width], and the four statistics; the other rows must stay untouched."""
    f = as_sr(frame, mode)
    f.flags |= extra_flags
    out = np.full(f.width * f.height, UNTOUCHED, dtype=np.uint32)
    _, stats = g.render(f, out=out, stats=True)
    a = min(max(0, f.start_row), f.height - 1)
    b = min(max(0, f.end_row), f.height - 1)
    px = out.reshape(f.height, f.width)
    assert np.all(px[:a] == UNTOUCHED) and np.all(px[b + 1:] == UNTOUCHED)
    return px[a:b + 1].copy(), stats


def triangles(model):
    return unit_cube_scene(2000) if model == "unit_cube_2000" else load_obj3ds(model)


def pair(model, prims=(), modes=(sa.MODE_REF_TREE, sa.MODE_BVH), on_device=None, devices=None):
    g, o = (sa.GpuScene(devices=devices) if devices else sa.GpuScene(0)), orc.Scene()
    for s in (g, o):
        s.set_triangles(*triangles(model))
        if prims:
            s.set_extra(list(prims))
    g.build(tuple(modes), on_device=on_device)
    assert o.build_tree() == 0
    return g, o


@pytest.fixture(scope="module")
def obj_pair():
    return pair("obj.3ds")


@pytest.fixture(scope="module")
def obj2_pair():
    return pair("obj2.3DS")


def same_cache(g, model):
    """The device's whole table against the model's: the same entries are filled, with the same colours."""
    got = g.get_light_field()
    assert got.size == lfm.cache_entries(model.n)
    filled = np.flatnonzero(got)
    want = np.array(sorted(model.cache), dtype=np.int64)
    return filled.size == want.size and np.array_equal(filled, want) and np.array_equal(got[filled], model.entries(want))


def check(g, o, model, frame, mode, extra_flags=0, whole_cache=True):
    """One frame on the scene's and the model's running caches: pixels, the four statistics, the fill count and the whole cache."""
    want = model.render(o, frame, target_of(mode))
    assert model.coord_margin > lfm.MARGIN and model.term_margin > lfm.MARGIN       # (the frame's input conditions)
    got, stats = gpu_rows(g, frame, mode, extra_flags)
    assert got.shape == want.shape and int(np.count_nonzero(got != want)) == 0
    samples = want.size * frame.sub_pixel_res ** 2
    assert [int(x) for x in stats] == [samples, 0, 0, 0]
    rs = g.ray_stats()
    assert int(rs[4]) == model.filled.size
    if whole_cache:
        assert same_cache(g, model)
    return got


def start(g, n):
    """The scene as a new Renderer with resolution n has it, and a model to match."""
    g.light_field_res = n
    g.reset_light_field()
    return lfm.LightFieldModel(n)


# ---- 1. the reference's goldens ----
GOLDEN_CASES = [(name, mode) for name, _ in lfm.GOLDENS for mode in ("tree", "bvh")] + \
               [(name, "brute") for name in ("noShading_lightFieldColor", "shading_lightFieldColor")]


@pytest.mark.parametrize("name,mode", GOLDEN_CASES)
def test_golden(obj_pair, name, mode):
    g, o = obj_pair
    _, _, n, f = lfm.gpu_frame(name)
    model = start(g, n)
    got = check(g, o, model, f, mode)
    want = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))
    assert int(np.count_nonzero((got & 0xFFFFFF) != want)) == 0
    assert model.filled.size > 1000


# ---- 2. many samples, few cells ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_contention_for_seven_cells(obj_pair, mode):
    g, o = obj_pair
    _, _, n, f = lfm.gpu_frame("contention")
    model = start(g, n)
    check(g, o, model, f, mode)
    assert model.filled.size == 7 and f.width * f.height * f.sub_pixel_res ** 2 == 49152
    check(g, o, model, f, mode)                                                  # and again: nothing left to claim
    assert model.filled.size == 0


@pytest.mark.parametrize("mode", ["tree", "brute", "bvh"])
def test_small_cache_with_focal_blur(obj2_pair, mode):
    g, o = obj2_pair
    _, _, n, f = lfm.gpu_frame("small_blur")
    model = start(g, n)
    check(g, o, model, f, mode)
    assert model.filled.size == 36


# ---- 3. rays that miss the sphere, a ragged width, a row range, extra geometry ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_samples_that_miss_the_sphere(obj_pair, mode):
    g, o = obj_pair
    _, _, n, f = lfm.gpu_frame("far")
    model = start(g, n)
    got = check(g, o, model, f, mode)
    idx, _, _ = lfm.sample_cells(*lfm.ptm.camera_samples(f), n)
    assert idx.size == 1073 and int((idx >= 0).sum()) == 560 == model.filled.size
    assert np.all(got.reshape(-1)[idx < 0] == BACKGROUND)


@pytest.mark.parametrize("mode", ["tree", "brute"])
def test_extra_geometry_and_a_row_range(mode):
    """(the oracle's nearest-hit target has no extra geometry: tree and brute force)"""
    model_file, prims, n, f = lfm.gpu_frame("far_primitives")
    g, o = pair(model_file, prims=prims, modes=(sa.MODE_REF_TREE,))
    model = start(g, n)
    got = check(g, o, model, f, mode)                                            # (gpu_rows: the rows outside 5..17 stay untouched)
    assert got.shape == (13, 37) and model.filled.size > 100
    plain = lfm.LightFieldModel(n)
    plain.render(orc_scene_without_extra(), f)
    assert plain.cache != model.cache                                            # the canonical rays see the spheres


def orc_scene_without_extra():
    o = orc.Scene()
    o.set_triangles(*load_obj3ds("obj.3ds"))
    assert o.build_tree() == 0
    return o


# ---- 4. the camera inside the sphere: no refusal, the arithmetic as written ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_start_inside_the_sphere(obj_pair, mode):
    g, o = obj_pair
    _, _, n, f = lfm.gpu_frame("inside_sphere")
    assert f.position_z < lfm.RADIUS
    model = start(g, n)
    check(g, o, model, f, mode)
    assert model.filled.size > 500


# ---- 5. the largest table: 4 GiB, indices up to 2^30 ----
def test_resolution_128(obj_pair):
    g, o = obj_pair
    _, _, n, f = lfm.gpu_frame("res128")
    model = start(g, n)
    try:
        check(g, o, model, f, "bvh", whole_cache=False)
        check(g, o, model, lfm.gpu_frame("res128_high")[3], "tree", whole_cache=False)
        filled = np.array(sorted(model.cache), dtype=np.int64)
        assert filled.size == 5000 and int(filled.max()) > 2 ** 29              # byte offsets beyond 2^31
        got = np.array([int(g.get_light_field(int(i), 1)[0]) for i in filled], dtype=np.uint32)
        assert np.array_equal(got, model.entries(filled))
        # a strided sample of the rest: 256 windows of 64 Ki entries hold exactly the model's entries
        total, window = lfm.cache_entries(n), 1 << 16
        for first in np.linspace(0, total - window, 256).astype(np.int64):
            part = g.get_light_field(int(first), window)
            inside = filled[(filled >= first) & (filled < first + window)]
            want = np.zeros(window, dtype=np.uint32)
            want[inside - first] = model.entries(inside)
            assert np.array_equal(part, want)
    finally:
        g.light_field_res = 64                                                   # (drops the 4 GiB)


# ---- 6. a warm cache and other views ----
@pytest.mark.parametrize("size", ["n64", "n8"])
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_warm_cache_and_second_view(obj_pair, mode, size):
    g, o = obj_pair
    frames = [lfm.gpu_frame("view%d_%s" % (i, size)) for i in range(3)]
    model = start(g, frames[0][2])
    total = 0
    for _, _, _, f in frames:
        first = check(g, o, model, f, mode)
        assert model.filled.size > 0
        total += model.filled.size
        again = check(g, o, model, f, mode)                                      # the same pose again: 0 cells, the same frame
        assert model.filled.size == 0 and np.array_equal(first, again)
    assert len(model.cache) == total
    check(g, o, model, frames[0][3], mode)                                       # back to the first view: its cells are still there
    assert model.filled.size == 0


# ---- 7. the cache is read, not recomputed ----
def test_loaded_cache_is_what_the_frame_shows(obj_pair):
    g, o = obj_pair
    _, _, n, f = lfm.gpu_frame("far_n16")
    start(g, n)
    colour = 0xFF123456
    g.set_light_field(np.full(lfm.cache_entries(n), colour, dtype=np.uint32))
    idx, _, _ = lfm.sample_cells(*lfm.ptm.camera_samples(f), n)
    assert 0 < int((idx >= 0).sum()) < idx.size
    for mode in ("tree", "bvh"):
        got, stats = gpu_rows(g, f, mode)
        assert np.array_equal(got.reshape(-1), np.where(idx >= 0, colour, BACKGROUND).astype(np.uint32))
        assert [int(x) for x in stats] == [idx.size, 0, 0, 0] and not g.ray_stats()[4:8].any()     # geometry is never traced
    assert np.all(g.get_light_field() == colour)
    g.reset_light_field()


# ---- 8. round trip and what drops the cache ----
def test_cache_round_trip_and_drops():
    g, o = pair("obj.3ds")
    _, _, n, f = lfm.gpu_frame("view0_n8")
    total = lfm.cache_entries(n)
    g.light_field_res = n
    assert g.light_field_res == n and not g.get_light_field().any()              # never rendered: zeros
    model = lfm.LightFieldModel(n)
    check(g, o, model, f, "tree")
    cache = g.get_light_field()
    assert np.count_nonzero(cache) == model.filled.size
    data = (np.arange(3000, dtype=np.uint32) * np.uint32(2654435761)) | np.uint32(1)
    g.set_light_field(data, first=total - 3000)
    assert np.array_equal(g.get_light_field(total - 3000, 3000), data)
    assert np.array_equal(g.get_light_field(0, total - 3000), cache[:total - 3000])       # the rest is untouched
    g.set_light_field(cache)
    assert np.array_equal(g.get_light_field(), cache)
    g.reset_light_field()
    assert not g.get_light_field().any()
    check(g, o, lfm.LightFieldModel(n), f, "tree")
    g.set_triangles(*load_obj3ds("obj.3ds"))                                     # a new model
    assert not g.get_light_field().any()
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH))
    check(g, o, lfm.LightFieldModel(n), f, "bvh")
    g.light_field_res = n + 1                                                    # another N
    assert g.get_light_field().size == lfm.cache_entries(n + 1) and not g.get_light_field().any()
    g.light_field_res = n
    assert not g.get_light_field().any()
    for bad in (0, 129):
        with pytest.raises(sa.SoftrayError) as e:
            g.light_field_res = bad
        assert e.value.code == sa._lib.SR_ERR_INVALID_ARG
    assert g.light_field_res == n
    # a table that was loaded before the first frame
    g.reset_light_field()
    g.set_light_field(data, first=100)
    want = np.zeros(total, dtype=np.uint32)
    want[100:3100] = data
    assert np.array_equal(g.get_light_field(), want)


# ---- 9. a frame of two row bands ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_two_row_bands(obj2_pair, mode):
    g, o = obj2_pair
    _, _, n, f = lfm.gpu_frame("small_blur")
    model = start(g, n)
    try:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, 8192)                              # 64 columns x 4 samples: bands of 32 rows, the frame has 48
        check(g, o, model, f, mode)
    finally:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, -1)
    assert model.filled.size == 36


# ---- 10. the unit-cube scene on both BVH builds ----
def test_unit_cube_scene_on_both_bvh_builds():
    model_file, _, n, f = lfm.gpu_frame("unit_cube")
    frames = []
    for on_device in (True, False):
        g, o = pair(model_file, modes=(sa.MODE_BVH,), on_device=on_device)
        assert g.bvh_stats()[3] == (1 if on_device else 0)
        model = start(g, n)
        frames.append(check(g, o, model, f, "bvh"))
        assert model.filled.size > 300
    assert np.array_equal(frames[0], frames[1])


# ---- 11. statistics ----
def test_statistics(obj_pair):
    g, o = obj_pair
    _, _, n, f = lfm.gpu_frame("view1_n64")
    for mode in ("tree", "brute", "bvh"):
        model = start(g, n)
        check(g, o, model, f, mode)
        rs = g.ray_stats().copy()
        assert int(rs[4]) == model.filled.size and rs[5] > 0
        if mode != "brute":
            assert rs[6] > 0 and rs[7] > 0                                       # the canonical rays' walks are counted
        g.reset_light_field()
        got, stats = gpu_rows(g, f, mode, sa._lib.F_PRIMARY_STATS_ONLY)
        assert [int(x) for x in stats] == [got.size, 0, 0, 0] and not g.ray_stats()[4:8].any()
        assert same_cache(g, model)


# ---- 12. refusals ----
def test_refused_combinations_leave_everything_untouched(obj_pair):
    g, o = obj_pair
    _, _, n, f = lfm.gpu_frame("view0_n8")
    model = start(g, n)
    check(g, o, model, f, "tree")
    before = g.get_light_field()
    for change in lfm.REFUSED:
        bad = lfm.apply_change(as_sr(f, "tree"), change)
        out = np.full(bad.width * bad.height, UNTOUCHED, dtype=np.uint32)
        with pytest.raises(sa.SoftrayError) as e:
            g.render(bad, out=out)
        assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED and "light field" in str(e.value), change
        assert np.all(out == UNTOUCHED) and np.array_equal(g.get_light_field(), before), change
    check(g, o, model, f, "tree")                                                # and the scene still renders
    assert model.filled.size == 0


def test_rccl_render_refuses_the_light_field():
    """sr_rccl_render refuses a light-field frame in its own right, before it makes strips of it: a one-rank communicator on one GPU."""
    import torch
    g, o = pair("obj.3ds")
    g.rccl_init(sa.rccl_unique_id(), 1, 0)
    _, _, n, f = lfm.gpu_frame("view0_n8")
    model = start(g, n)
    check(g, o, model, f, "tree")
    before = g.get_light_field()
    surface = torch.zeros(f.width * f.height, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(sa.SoftrayError) as e:
        g.rccl_render(as_sr(lfm.gpu_frame("view1_n8")[3], "tree"), surface.data_ptr(), stream)
    assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED and "light field" in str(e.value) and "sr_rccl_render" in str(e.value)
    torch.cuda.synchronize()
    assert not surface.any().item() and np.array_equal(g.get_light_field(), before)


def test_multi_device_scene_renders_on_the_first_device(obj_pair):
    g1, o = obj_pair
    gm = pair("obj.3ds", devices=[0, 0])[0]
    _, _, n, f = lfm.gpu_frame("view2_n8")
    model = lfm.LightFieldModel(n)
    gm.light_field_res = n
    check(gm, o, model, f, "bvh")
    assert gm.last_frame_parts() == 1
    check(gm, o, model, f, "bvh")
    assert model.filled.size == 0


# ---- 13. the C++ host mirror ----
def test_cpp_mirror_reproduces_the_goldens(tmp_path):
    exe = str(tmp_path / "lightfield_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "lightfield_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL OK" in r.stdout
    for line in ("shading_lightFieldColor", "noShading_lightFieldColor_4xAA", "LightFieldStoresTriangles = true refused ok"):
        assert line in r.stdout
