"""Voxel grids of any resolution from 1 to 256 (sr_set_voxel_res) on the device: the device voxeliser against the host loop and the CPU
model (tests/voxel_model_n.py, pinned by tests/test_voxel_res_model.py) for every size class, frames and SR_TARGET_VOXELS ray batches
against the model for the three walks (N < 64: the run-time grid with its occupancy bits in LDS; N = 64: the compile-time grid; N > 64:
the two-level walk), the two cross-check hooks, a change of N between frames, a multi-device scene and the C++ mirror.  Every comparison
is an exact equality: colours as uint32, normals as bit patterns.

What the sizes exercise: 5 -- N^3 is no multiple of 64 (the mask's tail); 63 / 65 -- either side of the kernel choice; 98 -- bricks clipped
on every axis; 256 -- 24-bit sort keys and 1.24 M (cell, triangle) pairs.

NOT YET RUN ON A GPU: no GPU could be obtained while this file was written; it has been collected and its model side (the frames'
background share, the ray batches' hit counts, the CRCs of the C++ program) checked on the CPU only."""
import os
import zlib

import numpy as np
import pytest

import softray_amd as sa
import voxel_model_n as vn
from helpers import GOLDEN, ROOT, load_obj3ds, make_frame

pytestmark = pytest.mark.gpu

W, H, DEPTH = 64, 48, 3.0
_cache = {}


def obj():
    if "obj" not in _cache:
        _cache["obj"] = load_obj3ds("obj.3ds")
    return _cache["obj"]


def model_grid(n):
    """The model's grid of obj.3ds at n, computed once."""
    if ("grid", n) not in _cache:
        v9, argb, _, _ = obj()
        _cache[("grid", n)] = vn.voxelise(v9, argb, n)
    return _cache[("grid", n)][:2]


def dev_scene(n):
    """One device scene of obj.3ds per n (no sr_build: a voxel frame needs triangles only)."""
    if ("scene", n) not in _cache:
        g = sa.GpuScene(0)
        g.set_triangles(*obj())
        g.voxel_res = n
        _cache[("scene", n)] = g
    return _cache[("scene", n)]


def voxel_frame(w=W, h=H, **kw):
    kw.setdefault("depth", DEPTH)
    f = make_frame(w, h, **kw)
    f.flags |= vn.F_VOXELS
    return f


def as_sr(frame):
    return sa.Frame.from_buffer_copy(bytes(frame))


def gpu_rows(g, frame, stats=False):
    """The frame's rows start_row..end_row as the library renders them, [rows, width]; the other rows must stay untouched."""
    f = as_sr(frame)
    out = np.full(f.width * f.height, 0x01020304, dtype=np.uint32)
    _, st = g.render(f, out=out, stats=stats)
    a = min(max(0, f.start_row), f.height - 1)
    b = min(max(0, f.end_row), f.height - 1)
    px = out.reshape(f.height, f.width)
    assert np.all(px[:a] == 0x01020304) and np.all(px[b + 1:] == 0x01020304)
    return (px[a:b + 1].copy(), st) if stats else px[a:b + 1].copy()


def model_image(grid, f):
    """The model's image of the frame; at least a quarter of its samples are background (long empty walks) and a quarter hits."""
    col = vn.sample_colors(grid, f)
    background = (f.background_argb | 0xFF000000) & 0xFFFFFFFF
    share = np.count_nonzero(col == background) / col.size
    assert 0.25 <= share <= 0.75, "background share %.2f" % share
    return vn.render(grid, f)


def assert_same_grid(got, want, what):
    assert got[0].shape == want[0].shape
    assert np.array_equal(got[0], want[0]), "%s: colours differ in %d cells" % (what, int(np.count_nonzero(got[0] != want[0])))
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), what + ": normals differ"


def grids_of(v9, argb, n):
    box = (np.array([-0.5] * 3), np.array([0.5] * 3))
    host = sa.GpuScene(device=-1)
    dev = sa.GpuScene(0)
    try:
        for s in (host, dev):
            s.set_triangles(v9, argb, *box)
            s.voxel_res = n
            with pytest.raises(sa.SoftrayError) as e:
                s.get_voxels()
            assert e.value.code == sa._lib.SR_ERR_NOT_BUILT
            s.build_voxels()
            s.build_voxels()                                         # idempotent
        return host.get_voxels(), dev.get_voxels()
    finally:
        host.close(); dev.close()


# ---- 1. the grid: device voxeliser == host loop == model ----
@pytest.mark.parametrize("n", [1, 2, 5, 32, 63, 65, 98, 128, 256])
def test_device_grid_equals_host_grid_equals_model(n):
    v9, argb, _, _ = obj()
    want = model_grid(n)
    host, dev = grids_of(v9, argb, n)
    assert dev[0].shape == (n, n, n) and dev[1].shape == (n, n, n, 3)
    assert_same_grid(host, want, "host at %d" % n)
    assert_same_grid(dev, want, "device at %d" % n)
    assert int(np.count_nonzero(dev[0])) >= 1


@pytest.mark.parametrize("n", [5, 98])
def test_device_grid_of_triangles_on_the_planes(n):
    v9, argb = vn.boundary_triangles(n)
    want = vn.voxelise(v9, argb, n)
    host, dev = grids_of(v9, argb, n)
    assert_same_grid(host, want, "host at %d" % n)
    assert_same_grid(dev, want, "device at %d" % n)


# ---- 2. frames against the model ----
@pytest.mark.parametrize("n", [5, 32, 65, 98, 256])
def test_frames_equal_the_model(n):
    f = voxel_frame()
    want = model_image(model_grid(n), f)
    got, st = gpu_rows(dev_scene(n), f, stats=True)
    assert got.shape == want.shape and int(np.count_nonzero(got != want)) == 0
    assert [int(x) for x in st] == [W * H, W * H, 0, 0]


CASES_98 = {
    "no_shading": dict(shading=False),
    "sub2": dict(sub_pixel_res=2),
    "focal_blur": dict(sub_pixel_res=2, focal_blur=True, focal_depth=3.0),
    "row_range": dict(start_row=7, end_row=39),
}


@pytest.mark.parametrize("case", list(CASES_98), ids=list(CASES_98))
def test_frames_at_98(case):
    f = voxel_frame(**CASES_98[case])
    want = model_image(model_grid(98), f)
    got, st = gpu_rows(dev_scene(98), f, stats=True)
    assert got.shape == want.shape and int(np.count_nonzero(got != want)) == 0
    samples = want.size * f.sub_pixel_res ** 2
    assert [int(x) for x in st] == [samples, samples, 0, 0]          # NumRaysFired, NumGeometryTests (NumRayTests == 1), no nodes, no leaves


def test_strips_at_98():
    g = dev_scene(98)
    want = model_image(model_grid(98), voxel_frame())
    got = np.zeros_like(want)
    for k in range(3):
        f = as_sr(voxel_frame(strips=(16, 3, k)))
        rows = [r for r in range(H) if (r // 16) % 3 == k]
        px, st = g.render(f, stats=True)
        assert px.size == len(rows) * W and int(st[0]) == int(st[1]) == len(rows) * W
        got[rows] = px.reshape(len(rows), W)
    assert int(np.count_nonzero(got != want)) == 0


def test_row_bands_at_98():
    g = dev_scene(98)
    f = voxel_frame(sub_pixel_res=2)
    want = model_image(model_grid(98), f)
    try:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, W * 4 * 32)            # 32-row bands: two of them
        got, st = gpu_rows(g, f, stats=True)
    finally:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, -1)
    assert int(np.count_nonzero(got != want)) == 0
    assert [int(x) for x in st] == [W * H * 4, W * H * 4, 0, 0]


# ---- 3. SR_TARGET_VOXELS ----
def kat_batches():
    """20 000 rays each on the reference's single-triangle grid: from z in [-1, -0.5] along +z with x, y in [-1, 1] (the walk maps the box
    (-1, -1, -1)..(1, 1, 1) onto the grid, so every one of these crosses the filled layer: the model says 20 000 hits); the same starts with
    random directions (3393 hits); and along +z with x, y in [-1.5, 1.5], where the rays beside the box miss (8942 hits)."""
    rng = np.random.default_rng(32)
    n = 20000
    starts = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, -0.5, n)], axis=-1)
    along = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
    anywhere = rng.uniform(-1, 1, (n, 3))
    wide = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(-1, -0.5, n)], axis=-1)     # some start beside the box
    return [("along_z", starts, along), ("random_directions", starts, anywhere), ("beside_the_box", wide, along)]


def check_batch(g, grid, starts, dirs):
    want = vn.walk(grid[0], grid[1], starts, dirs)
    got = g.trace(sa.TARGET_VOXELS, starts, dirs, counters=True)
    assert np.array_equal(got["hit"], want["hit"])
    assert np.array_equal(got["color"], want["color"])
    assert np.array_equal(got["normal"].view(np.uint64), want["normal"].view(np.uint64))
    assert not got["ray_frac"].any() and not got["pos"].any() and np.all(got["tri_index"] == -1)
    assert np.all(got["counters"] == np.array([1, 0, 0], dtype=np.int32))
    return want, got


def test_target_voxels_on_the_reference_kat_grid_at_32():
    grid = vn.voxelise(vn.KAT_TRIANGLE, vn.KAT_COLOR, 32)
    assert grid[2]["filled"] == 32 * 32
    g = sa.GpuScene(0)
    try:
        g.set_triangles(vn.KAT_TRIANGLE, vn.KAT_COLOR, np.array([-0.5] * 3), np.array([0.5] * 3))
        g.voxel_res = 32
        hits = {}
        for name, starts, dirs in kat_batches():
            want, _ = check_batch(g, grid, starts, dirs)
            hits[name] = int(want["hit"].sum())
        dc, dn = g.get_voxels()
        assert_same_grid((dc, dn), grid, "KAT")
    finally:
        g.close()
    assert hits == dict(along_z=20000, random_directions=3393, beside_the_box=8942)


# ---- 4. the cross-check hooks ----
def frame_and_batch(g):
    rng = np.random.default_rng(5)
    d = rng.normal(size=(6000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = rng.uniform(-0.5, 0.5, (6000, 3))
    starts, dirs = t - d * 3.0, d * rng.uniform(0.2, 1.0, (6000, 1))   # from outside towards the model
    px = gpu_rows(g, voxel_frame())
    sub = gpu_rows(g, voxel_frame(sub_pixel_res=2))
    r = g.trace(sa.TARGET_VOXELS, starts, dirs, counters=True)
    return px, sub, r


def same_results(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for k in ("hit", "color", "tri_index", "counters"):
        assert np.array_equal(a[2][k], b[2][k]), k
    for k in ("normal", "ray_frac", "pos"):
        assert np.array_equal(a[2][k].view(np.uint64), b[2][k].view(np.uint64)), k


@pytest.mark.parametrize("n,hook", [(65, 42), (98, 42), (256, 42), (32, 41)])
def test_hooks_give_the_same_results(n, hook):
    g = dev_scene(n)
    default = frame_and_batch(g)
    try:
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, hook)
        other = frame_and_batch(g)
    finally:
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
    same_results(default, other)
    assert np.array_equal(default[0], model_image(model_grid(n), voxel_frame()))
    assert 0 < int(default[2]["hit"].sum()) < 6000


# ---- 5. another N on the same scene, several devices, the C++ mirror ----
def test_changing_the_resolution_between_frames():
    g = sa.GpuScene(0)
    try:
        g.set_triangles(*obj())
        f = voxel_frame()
        frames = []
        for n in (64, 98, 64):
            g.voxel_res = n
            assert g.voxel_res == n
            with pytest.raises(sa.SoftrayError) as e:
                g.get_voxels()
            assert e.value.code == sa._lib.SR_ERR_NOT_BUILT
            got = gpu_rows(g, f)                                     # the frame builds the grid
            assert np.array_equal(got, model_image(model_grid(n), f)), n
            assert_same_grid(g.get_voxels(), model_grid(n), "grid at %d" % n)
            frames.append(got)
        assert np.array_equal(frames[0], frames[2]) and not np.array_equal(frames[0], frames[1])
        g.voxel_res = 64                                             # the same value keeps the grid
        assert_same_grid(g.get_voxels(), model_grid(64), "kept")
    finally:
        g.close()


@pytest.mark.parametrize("n", [32, 98])
def test_multi_device_scene_honours_voxel_res(n):
    g = sa.GpuScene(devices=[0, 0])
    try:
        g.set_triangles(*obj())
        assert g.voxel_res == 64
        g.voxel_res = n
        assert g.voxel_res == n
        for kw in (dict(), dict(sub_pixel_res=2)):
            f = voxel_frame(**kw)
            want = model_image(model_grid(n), f)
            got, st = gpu_rows(g, f, stats=True)
            assert int(np.count_nonzero(got != want)) == 0, kw
            assert g.last_frame_parts() == 2
            samples = want.size * f.sub_pixel_res ** 2
            assert [int(x) for x in st] == [samples, samples, 0, 0]
        assert_same_grid(g.get_voxels(), model_grid(n), "multi-device grid")
        with pytest.raises(sa.SoftrayError) as e:
            g.voxel_res = 257
        assert e.value.code == sa._lib.SR_ERR_INVALID_ARG and g.voxel_res == n
    finally:
        g.close()


CPP_TEST = os.path.join(ROOT, "tests", "cpp", "voxel_res_tests.cpp")


def test_cpp_constants_are_the_models_crcs():
    """The expected pixels of tests/cpp/voxel_res_tests.cpp are CRC-32s of the frames the model renders."""
    import re
    src = open(CPP_TEST).read()
    crc = {k: int(v, 16) for k, v in re.findall(r"static const uint32_t kCrc(\w+) = 0x([0-9a-f]{8})u;", src)}
    kat = vn.voxelise(vn.KAT_TRIANGLE, vn.KAT_COLOR, 32)[:2]
    f = voxel_frame()
    assert zlib.crc32(model_image(kat, f).astype("<u4").tobytes()) & 0xFFFFFFFF == crc["Kat32"]
    assert zlib.crc32(model_image(model_grid(98), f).astype("<u4").tobytes()) & 0xFFFFFFFF == crc["Obj98"]


def test_cpp_mirror_renders_other_resolutions(tmp_path):
    import subprocess
    exe = str(tmp_path / "voxel_res_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, CPP_TEST,
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL OK" in r.stdout
    assert r.stdout.count("crc ok") == 2 and "range refused ok" in r.stdout
