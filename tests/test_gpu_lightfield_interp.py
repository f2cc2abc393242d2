"""Quad-linear interpolation of the colour light field on the device (sr_set_light_field_interpolation, sr_light_field_coords) against the CPU
model (tests/lightfield_interp_model.py) -- bit for bit: every frame comparison is an exact equality over every pixel and every table entry.

The model takes the DEVICE's coordinates (sr_light_field_coords of the oracle's camera rays): where the 16 entries are equal the blend lands
within rounding of an integer, and one ulp of atan2 / asin flips a byte.  The coordinates themselves are checked against numpy's (test 1).
The frames are lightfield_interp_model.gpu_frames(), whose input conditions and wrap counts tests/test_lightfield_interp_model.py checks on
the CPU.  (far_primitives runs in tree and brute-force mode: the oracle's nearest-hit target, the reference of SR_MODE_BVH, has no extra
geometry -- as in tests/test_gpu_lightfield.py.)"""
import os
import subprocess

import numpy as np
import pytest

import lightfield_interp_model as lim
import lightfield_model as lfm
import lightfield_shadow_model as lsm
import pathtrace_model as ptm
import softray_amd as sa
from helpers import GOLDEN, ROOT, load_obj3ds, orc, unit_cube_scene

pytestmark = pytest.mark.gpu
MODES = {"tree": sa.MODE_REF_TREE, "brute": sa.MODE_BRUTE, "bvh": sa.MODE_BVH}
UNTOUCHED = 0x01020304
FRAMES = lim.gpu_frames()
COORD_TOLERANCE = 1e-11          # a few ulp of an angle <= pi, scaled by at most 256: about 3e-13; nine orders below one cell
TERM_MARGIN = 1e-9


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


_pairs = {}


def pair(model, prims=(), devices=None):
    key = (model, bool(prims), tuple(devices or ()))
    if key not in _pairs:
        g, o = (sa.GpuScene(devices=devices) if devices else sa.GpuScene(0)), orc.Scene()
        for s in (g, o):
            s.set_triangles(*(unit_cube_scene(2000) if model == "unit_cube_2000" else load_obj3ds(model)))
            if prims:
                s.set_extra(list(prims))
        g.build((sa.MODE_REF_TREE,) if prims else (sa.MODE_REF_TREE, sa.MODE_BVH))
        assert o.build_tree() == 0
        _pairs[key] = (g, o)
    return _pairs[key]


_coords = {}


def device_coords(g, name):
    """sr_light_field_coords of the frame's camera samples at the frame's N, once per frame (read-only)."""
    _, _, n, f = FRAMES[name]
    if name not in _coords:
        g.light_field_res = n
        coords, inside = g.light_field_coords(*ptm.camera_samples(f))
        coords.setflags(write=False)
        inside.setflags(write=False)
        _coords[name] = (coords, inside)
    return _coords[name]


def start(g, n, table=lfm.LightFieldModel, on=True):
    g.light_field_res = n
    g.reset_light_field()
    g.light_field_interpolation = on
    return lim.LightFieldInterpModel(table(n))


def same_cache(g, table):
    got = g.get_light_field()
    assert got.size == lfm.cache_entries(table.n)
    filled = np.flatnonzero(got)
    want = np.array(sorted(table.cache), dtype=np.int64)
    return filled.size == want.size and np.array_equal(filled, want) and np.array_equal(got[filled], table.entries(want))


def check(g, o, model, name, mode, extra_flags=0, shadowed=False):
    """One frame on the scene's and the model's running tables: pixels, statistics, the canonical rays and the whole table."""
    f = FRAMES[name][3] if not shadowed else lsm.shadow_frame(orc.Frame.from_buffer_copy(bytes(FRAMES[name][3])))
    coords, inside = device_coords(g, name)
    want = model.render(o, f, coords, inside, target_of(mode))
    assert model.conditions_hold()
    got, stats = gpu_rows(g, f, mode, extra_flags)
    diff = int(np.count_nonzero(got != want)) if got.shape == want.shape else -1
    print("%s %s: %d of %d pixels differ, %d cells read, %d filled" % (name, mode, diff, want.size, model.touched.size, model.filled.size))
    assert diff == 0
    assert [int(x) for x in stats] == [want.size * f.sub_pixel_res ** 2, 0, 0, 0]
    rs = g.ray_stats()
    if shadowed:
        assert int(rs[4]) >= model.filled.size
    else:
        assert int(rs[4]) == model.filled.size                                  # one canonical ray per cell filled
    if model.filled.size == 0:
        assert not rs[4:8].any()
    assert same_cache(g, model.table)
    return got


# ---- 1. the coordinates: sr_light_field_coords against numpy's RayToFloat4D ----
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_coordinates_against_numpy(name):
    model_file, prims, n, f = FRAMES[name]
    g, _ = pair(model_file, prims)
    coords, inside = device_coords(g, name)
    want, want_inside, term = lim.float4d(*ptm.camera_samples(f), n)
    clear = np.abs(term - lfm.EPSILON) > TERM_MARGIN
    err = float(np.abs(coords - want).max())
    print("%s: %d samples, %d inside, largest coordinate error %.3g" % (name, inside.size, int(inside.sum()), err))
    assert clear.all() and np.array_equal(inside[clear], want_inside[clear])
    assert err <= COORD_TOLERANCE
    assert not coords[~inside].any()
    assert lim.wrap_counts(coords, inside, n) == lim.frame_figures(name)[3]       # the device's base cells wrap where numpy's do


def test_coordinates_of_special_lines():
    g, _ = pair("obj.3ds")
    g.light_field_res = 4
    starts = np.array([[0.0, 0.0, 2.0], [0.0, 2.0, 2.0], [0.0, 0.0, 2.0]])
    dirs = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [0.0, 0.0, -7.5]])
    coords, inside = g.light_field_coords(starts, dirs)
    assert inside.tolist() == [True, False, True]
    assert np.abs(coords[0] - np.array([4.0, 2.0, 8.0, 2.0])).max() <= COORD_TOLERANCE and coords[0, 2] <= 8.0    # s = 1: F_s = 2N
    assert coords[1].tolist() == [0.0] * 4 and np.array_equal(coords[2], coords[0])                              # dir is normalised
    g.light_field_res = 64
    assert np.abs(g.light_field_coords(starts[:1], dirs[:1])[0][0] - np.array([64.0, 32.0, 128.0, 32.0])).max() <= COORD_TOLERANCE * 16
    empty, none = g.light_field_coords(np.zeros((0, 3)), np.zeros((0, 3)))
    assert empty.shape == (0, 4) and none.shape == (0,)


# ---- 2. frame == model(device coordinates), table == model's table, in every trace mode ----
FRAME_CASES = [(name, mode) for name in ("contention", "unit_cube", "pose_up", "pose_down", "blur_x2") for mode in ("tree", "brute", "bvh")] + \
              [("far_primitives", "tree"), ("far_primitives", "brute")]


@pytest.mark.parametrize("name,mode", FRAME_CASES)
def test_frame(name, mode):
    model_file, prims, n, f = FRAMES[name]
    g, o = pair(model_file, prims)
    device_coords(g, name)
    model = start(g, n)
    got = check(g, o, model, name, mode)
    assert model.filled.size == model.touched.size > 16
    nearest = lfm.LightFieldModel(n).render(o, f, target_of(mode))
    assert int(np.count_nonzero(nearest != got)) > 0                             # not the nearest lookup
    if name == "far_primitives":
        assert got.shape == (13, 37) and not device_coords(g, name)[1].all()
    g.reset_light_field()


def test_every_axis_wraps_on_the_device():
    total = np.zeros(4, dtype=np.int64)
    for name in sorted(FRAMES):
        model_file, prims, n, _ = FRAMES[name]
        coords, inside = device_coords(pair(model_file, prims)[0], name)
        wraps = lim.wrap_counts(coords, inside, n)
        for got, want in zip(wraps, lim.REQUIRED[name].get("wraps", (None,) * 4)):
            assert want is None or got == want
        total += np.array(wraps)
    assert np.all(total > 0)


@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_two_row_bands(mode):
    g, o = pair("obj.3ds")
    _, _, n, f = FRAMES["contention"]
    model = start(g, n)
    try:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, 64 * 16 * 32)                      # 32 rows per band: two bands for 48 rows
        check(g, o, model, "contention", mode)
    finally:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, -1)
    g.reset_light_field()


@pytest.mark.parametrize("name", ["pose_up", "blur_x2"])
def test_recomputing_variant_gives_the_same_frame(name):
    """Hook 39: the apply kernel computes base cell and fractions again instead of taking them from the lookup."""
    model_file, prims, n, _ = FRAMES[name]
    g, o = pair(model_file, prims)
    model = start(g, n)
    try:
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, 39)
        check(g, o, model, name, "bvh")
        check(g, o, model, name, "bvh")                                          # warm
    finally:
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
    g.reset_light_field()


# ---- 3. from a baked table: identical frames, no cell filled; a second frame on the warm table fills none ----
@pytest.mark.parametrize("name,mode", [("contention", "tree"), ("contention", "bvh"), ("pose_up", "bvh"), ("pose_down", "tree"), ("blur_x2", "bvh"),
                                       ("unit_cube", "bvh")])
def test_baked_and_warm_tables(name, mode):
    model_file, prims, n, f = FRAMES[name]
    g, o = pair(model_file, prims)
    model = start(g, n)
    lazy = check(g, o, model, name, mode)
    assert model.filled.size > 0
    again = check(g, o, model, name, mode)                                       # warm: nothing is claimed, nothing is filled
    assert model.filled.size == 0 and np.array_equal(lazy, again)
    g.reset_light_field()
    total = lfm.cache_entries(n)
    assert g.bake_light_field(as_sr(f, mode)) == total                          # the bake is unaffected by the switch
    baked, stats = gpu_rows(g, f, mode)
    assert np.array_equal(baked, lazy)
    assert not g.ray_stats()[4:8].any()                                          # no cell was filled
    table = g.get_light_field()
    assert np.all(table != 0) and np.array_equal(table[model.touched], model.table.entries(model.touched))
    g.reset_light_field()


# ---- 4. with shadows in the table: the lazily filled neighbours equal the shadowed bake's entries ----
@pytest.mark.parametrize("name,mode", [("pose_up", "tree"), ("pose_up", "bvh"), ("contention", "bvh")])
def test_shadowed_lazy_fill_equals_the_shadowed_bake(name, mode):
    model_file, prims, n, f = FRAMES[name]
    g, o = pair(model_file, prims)
    fs = lsm.shadow_frame(orc.Frame.from_buffer_copy(bytes(f)))
    try:
        g.light_field_shadows = True
        model = start(g, n, table=lsm.LightFieldShadowModel)
        check(g, o, model, name, mode, shadowed=True)
        lazy = g.get_light_field()
        touched = np.flatnonzero(lazy)
        assert np.array_equal(touched, model.touched) and touched.size > 16
        g.reset_light_field()
        assert g.bake_light_field(as_sr(fs, mode)) == lfm.cache_entries(n)
        baked = g.get_light_field()
        assert np.array_equal(baked[touched], lazy[touched])
        plain = lfm.LightFieldModel(n)
        plain.fill(o, f, touched, target_of(mode))
        assert int(np.count_nonzero(plain.entries(touched) != lazy[touched])) > 0    # the shadows are in it
    finally:
        g.light_field_shadows = False
        g.reset_light_field()


def test_shadowed_frame_in_two_bands():
    g, o = pair("obj.3ds")
    n = FRAMES["contention"][2]
    try:
        g.light_field_shadows = True
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, 64 * 16 * 32 * 16)                 # the shadowed band is 1/16 of the budget: 32 rows, two bands
        model = start(g, n, table=lsm.LightFieldShadowModel)
        check(g, o, model, "contention", "bvh", shadowed=True)
    finally:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, -1)
        g.light_field_shadows = False
        g.reset_light_field()


# ---- 5. the switch ----
def test_switch_off_after_on_is_the_nearest_lookup():
    g, o = pair("obj.3ds")
    _, _, n, f = FRAMES["pose_up"]
    start(g, n)
    gpu_rows(g, f, "bvh")
    g.light_field_interpolation = False
    g.reset_light_field()
    off, _ = gpu_rows(g, f, "bvh")
    off_table = g.get_light_field()
    never = sa.GpuScene(0)
    never.set_triangles(*load_obj3ds("obj.3ds"))
    never.build((sa.MODE_BVH,))
    never.light_field_res = n
    assert never.light_field_interpolation is False
    want, _ = gpu_rows(never, f, "bvh")
    assert off.tobytes() == want.tobytes() and off_table.tobytes() == never.get_light_field().tobytes()
    model = lfm.LightFieldModel(n)
    assert np.array_equal(model.render(o, f, lfm.TRACE_NEAREST), off)
    never.close()
    g.reset_light_field()


def test_setter_getter_and_refusals():
    g, _ = pair("obj.3ds")
    lib, h = sa._lib.lib(), g._h
    g.light_field_interpolation = True
    for bad in (2, -1, 1 << 20):
        assert lib.sr_set_light_field_interpolation(h, bad) == sa._lib.SR_ERR_INVALID_ARG
        assert "sr_set_light_field_interpolation" in lib.sr_last_error().decode()
    assert lib.sr_get_light_field_interpolation(h) == 1
    g.set_triangles(*load_obj3ds("obj.3ds"))                                     # survives sr_set_triangles
    assert g.light_field_interpolation is True
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH))
    # the switch does not touch the table, and every refusal of a light-field frame stays
    _, _, n, f = FRAMES["pose_up"]
    g.light_field_res = n
    g.reset_light_field()
    table = np.zeros(lfm.cache_entries(n), dtype=np.uint32)
    table[5:50] = 0xFF102030
    g.set_light_field(table)
    g.light_field_interpolation = False
    g.light_field_interpolation = True
    assert np.array_equal(g.get_light_field(), table)
    out = np.full(f.width * f.height, UNTOUCHED, dtype=np.uint32)
    for change in lfm.REFUSED:
        bad = lfm.apply_change(as_sr(f, "tree"), change)
        with pytest.raises(sa.SoftrayError) as e:
            g.render(bad, out=out)
        assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED
    assert np.all(out == UNTOUCHED) and np.array_equal(g.get_light_field(), table)
    one, out4, out1 = np.zeros(3), np.zeros(4), np.zeros(1, dtype=np.uint8)
    assert lib.sr_light_field_coords(h, 1, None, one.ctypes.data, out4.ctypes.data, out1.ctypes.data) == sa._lib.SR_ERR_INVALID_ARG
    assert lib.sr_light_field_coords(h, -1, one.ctypes.data, one.ctypes.data, out4.ctypes.data, out1.ctypes.data) == sa._lib.SR_ERR_INVALID_ARG
    host = sa.GpuScene(-1)
    host.light_field_interpolation = True
    assert host.light_field_interpolation is True
    assert lib.sr_light_field_coords(host._h, 1, one.ctypes.data, one.ctypes.data, out4.ctypes.data, out1.ctypes.data) == sa._lib.SR_ERR_NO_DEVICE
    host.close()
    g.light_field_interpolation = False
    g.reset_light_field()


def test_multi_device_scene_interpolates_on_its_first_device():
    g, o = pair("obj.3ds")
    gm, _ = pair("obj.3ds", devices=[0, 0])
    _, _, n, f = FRAMES["pose_up"]
    device_coords(g, "pose_up")
    model = start(gm, n)
    assert gm.light_field_interpolation is True
    check(gm, o, model, "pose_up", "bvh")
    assert gm.last_frame_parts() == 1
    gm.light_field_interpolation = False
    gm.reset_light_field()


def test_render_device_interpolates():
    import torch
    g, o = pair("obj.3ds")
    _, _, n, f = FRAMES["pose_up"]
    model = start(g, n)
    coords, inside = device_coords(g, "pose_up")
    want = model.render(o, f, coords, inside, lfm.TRACE_NEAREST)
    px = torch.zeros(f.width * f.height, dtype=torch.int32, device="cuda:0")
    g.render_device(as_sr(f, "bvh"), px.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(px.cpu().numpy().view(np.uint32).reshape(f.height, f.width), want)
    g.light_field_interpolation = False
    g.reset_light_field()


def test_cpp_mirror_passes_the_switch_on(tmp_path):
    exe = str(tmp_path / "lightfield_interp_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "lightfield_interp_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL OK" in r.stdout
    for line in ("switch defaults to off ok", "interpolated frame differs from the nearest lookup ok", "interpolated frame equals sr_render with the switch on: diff=0",
                 "warm frame identical ok", "switch off: the nearest lookup again ok"):
        assert line in r.stdout
