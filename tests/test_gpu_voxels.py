"""Voxel-grid rendering (SR_F_VOXELS, rayTraceVoxels) on the device: the reference's two goldens through the C ABI and through the C++
mirror, the device voxeliser against the host loop and the CPU model (tests/voxel_model.py, pinned to the goldens by
tests/test_voxel_model.py), SR_TARGET_VOXELS ray batches and frames without a golden against the model -- bit for bit, every
comparison an exact equality.

NOT YET RUN ON A GPU: no GPU could be obtained while this file was written; it has been collected and its model side (the frames' coverage,
the ray batch's hit share) checked on the CPU only."""
import os

import numpy as np
import pytest

import softray_amd as sa
import voxel_model as vm
from helpers import GOLDEN, ROOT, c1_spheres, load_obj3ds, make_frame, orc, read_bmp_rgb, unit_cube_scene

pytestmark = pytest.mark.gpu


def golden_rgb(name):
    return read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))


def voxel_frame(w=100, h=None, **kw):
    f = make_frame(w, h, **kw)
    f.flags |= vm.F_VOXELS
    return f


def as_sr(frame, mode=sa.MODE_REF_TREE):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = mode
    return f


def gpu_rows(g, frame, stats=False, mode=sa.MODE_REF_TREE):
    """The frame's rows start_row..end_row as the library renders them, [rows, width]; the other rows must stay untouched."""
    f = as_sr(frame, mode)
    out = np.full(f.width * f.height, 0x01020304, dtype=np.uint32)
    _, st = g.render(f, out=out, stats=stats)
    a = min(max(0, f.start_row), f.height - 1)
    b = min(max(0, f.end_row), f.height - 1)
    px = out.reshape(f.height, f.width)
    assert np.all(px[:a] == 0x01020304) and np.all(px[b + 1:] == 0x01020304)
    return (px[a:b + 1].copy(), st) if stats else px[a:b + 1].copy()


def model_image(grid, f):
    """The model's image of the frame, which must show the model: an empty frame cannot pass a comparison."""
    want = vm.render(grid, f)
    background = (f.background_argb | 0xFF000000) & 0xFFFFFFFF
    assert np.count_nonzero(want != background) >= 0.10 * want.size, "the model's frame is (nearly) empty"
    return want


SCENES = {"obj": lambda: load_obj3ds("obj.3ds"), "obj2": lambda: load_obj3ds("obj2.3DS"), "cube20k": lambda: unit_cube_scene(20000),
          "cube200k": lambda: unit_cube_scene(200000)}
_cache = {}


def scene(name, devices=None):
    """(GpuScene without any sr_build, the model's grid) of a named scene."""
    key = (name, tuple(devices) if devices else None)
    if key not in _cache:
        v9, argb, bmin, bmax = SCENES[name]()
        g = sa.GpuScene(0) if devices is None else sa.GpuScene(devices=list(devices))
        g.set_triangles(v9, argb, bmin, bmax)
        if (name, "grid") not in _cache:
            _cache[(name, "grid")] = vm.voxelise(v9, argb)
        _cache[key] = g
    return _cache[key], _cache[(name, "grid")][:2]


# ---- 1. the reference's goldens through the C ABI and the C++ mirror ----
@pytest.mark.parametrize("name,model,kw", vm.GOLDENS, ids=[g[0] for g in vm.GOLDENS])
def test_voxel_goldens(name, model, kw):
    g = sa.GpuScene(0)
    g.set_triangles(*load_obj3ds(model))                             # no sr_build, no sr_build_voxels: the frame needs triangles only
    got, st = gpu_rows(g, voxel_frame(**kw), stats=True, mode=sa.MODE_BVH)
    assert np.all(got >> 24 == 0xFF)
    assert int(np.count_nonzero((got & 0xFFFFFF) != golden_rgb(name))) == 0
    assert [int(x) for x in st] == [10000, 10000, 0, 0]              # NumRaysFired, NumGeometryTests (NumRayTests == 1), no nodes, no leaves


def test_cpp_mirror_reproduces_the_goldens(tmp_path):
    import subprocess
    exe = str(tmp_path / "voxel_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "voxel_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL OK" in r.stdout
    assert r.stdout.count("diff=0") == 3 and "refused ok" in r.stdout


# ---- 2. the grid: device voxeliser == host loop == model ----
@pytest.mark.parametrize("name", ["obj", "obj2", "cube20k", "cube200k"])
def test_device_grid_equals_host_grid_equals_model(name):
    v9, argb, bmin, bmax = SCENES[name]()
    want = vm.voxelise(v9, argb)
    _cache[(name, "grid")] = want
    host = sa.GpuScene(device=-1)
    host.set_triangles(v9, argb, bmin, bmax)
    host.build_voxels()
    dev = sa.GpuScene(0)
    dev.set_triangles(v9, argb, bmin, bmax)
    with pytest.raises(sa.SoftrayError) as e:
        dev.get_voxels()
    assert e.value.code == sa._lib.SR_ERR_NOT_BUILT
    dev.build_voxels()
    dev.build_voxels()                                               # idempotent
    hc, hn = host.get_voxels()
    dc, dn = dev.get_voxels()
    assert np.array_equal(hc, want[0]) and np.array_equal(hn.view(np.uint64), want[1].view(np.uint64))
    assert np.array_equal(dc, hc), "colours differ in %d cells" % int(np.count_nonzero(dc != hc))
    assert np.array_equal(dn.view(np.uint64), hn.view(np.uint64))
    assert int(np.count_nonzero(dc)) == want[2]["filled"] > 10000
    host.close(); dev.close()


def test_new_triangles_drop_the_grid():
    v9, argb, bmin, bmax = unit_cube_scene(20000)
    g = sa.GpuScene(0)
    g.set_triangles(v9, argb, bmin, bmax)
    f = voxel_frame(64, depth=2.0)
    a = gpu_rows(g, f)
    g.set_triangles(v9[:3000], argb[:3000], bmin, bmax)
    with pytest.raises(sa.SoftrayError):
        g.get_voxels()
    b = gpu_rows(g, f)
    assert np.array_equal(b, model_image(vm.voxelise(v9[:3000], argb[:3000])[:2], f)) and not np.array_equal(a, b)


# ---- 3. VoxelGrid.IntersectRay in batch ----
def ray_batch(n, seed=7):
    rng = np.random.default_rng(seed)
    k = n // 5
    parts = []
    s = rng.uniform(-0.9, 0.9, (k, 3)); parts.append((s, rng.uniform(-1, 1, (k, 3))))                    # start inside the box (-1..1)
    s = rng.uniform(-0.45, 0.45, (k, 3)); parts.append((s, rng.uniform(-0.3, 0.3, (k, 3))))              # start inside the model, short rays
    d = rng.normal(size=(k, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = rng.uniform(-0.5, 0.5, (k, 3))
    parts.append((t - d * 3.0, d * rng.uniform(0.2, 1.0, (k, 1))))                                       # from outside towards the model
    parts.append((t * 2 - d * 3.0 + 4.0, -d))                                                            # far away, pointing away: miss the box
    ax = np.zeros((n - 4 * k, 3)); i = rng.integers(0, 3, n - 4 * k)
    ax[np.arange(ax.shape[0]), i] = rng.choice([-1.0, 1.0, 0.25, -0.125], n - 4 * k)
    s = rng.uniform(-0.5, 0.5, (n - 4 * k, 3)); s[np.arange(ax.shape[0]), i] = rng.choice([-2.0, 2.0, 0.0, -0.75], n - 4 * k) * -np.sign(ax[np.arange(ax.shape[0]), i])
    parts.append((s, ax))                                                                                # axis-parallel rays
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@pytest.mark.parametrize("name", ["obj", "cube20k"])
def test_target_voxels_ray_batch_against_the_model(name):
    g, grid = scene(name)
    starts, dirs = ray_batch(120000)
    want = vm.walk(grid[0], grid[1], starts, dirs)
    got = g.trace(sa.TARGET_VOXELS, starts, dirs, counters=True)
    hits = int(want["hit"].sum())
    assert 0.15 * starts.shape[0] < hits < 0.9 * starts.shape[0]     # the batch both hits and misses
    assert np.array_equal(got["hit"], want["hit"])
    assert np.array_equal(got["color"], want["color"])
    assert np.array_equal(got["normal"].view(np.uint64), want["normal"].view(np.uint64))
    assert not got["ray_frac"].any() and not got["pos"].any() and np.all(got["tri_index"] == -1)
    assert np.all(got["counters"] == np.array([1, 0, 0], dtype=np.int32))


# ---- 4. frames without a golden against the model ----
FRAMES = {
    "shading": dict(w=100, h=100, depth=2.5),
    "no_shading": dict(w=100, h=100, depth=2.5, shading=False),
    "directional_no_specular": dict(w=96, h=96, depth=2.5, point_light=False, specular=False),
    "sub2": dict(w=80, h=80, depth=2.5, sub_pixel_res=2),
    "sub3": dict(w=64, h=64, depth=2.5, sub_pixel_res=3, yaw_deg=20.0, pitch_deg=35.0),
    "focal_blur": dict(w=64, h=64, depth=2.0, sub_pixel_res=2, focal_blur=True, focal_depth=2.0),
    "non_square": dict(w=150, h=67, depth=2.0, yaw_deg=250.0, pitch_deg=10.0, roll_deg=30.0),
    "row_window": dict(w=90, h=110, depth=2.0, start_row=31, end_row=77),
}


@pytest.mark.parametrize("name", ["obj", "cube20k"])
@pytest.mark.parametrize("case", list(FRAMES), ids=list(FRAMES))
def test_frames_against_the_model(name, case):
    g, grid = scene(name)
    kw = dict(FRAMES[case])
    f = voxel_frame(kw.pop("w"), kw.pop("h"), **kw)
    want = model_image(grid, f)
    got, st = gpu_rows(g, f, stats=True)
    assert got.shape == want.shape
    assert int(np.count_nonzero(got != want)) == 0
    rays = want.size * f.sub_pixel_res ** 2
    assert [int(x) for x in st] == [rays, rays, 0, 0]


def test_row_bands_and_the_global_table_walk_give_the_same_frame():
    g, grid = scene("cube20k")
    f = voxel_frame(100, 120, depth=2.0, sub_pixel_res=2)
    want = model_image(grid, f)
    try:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, 100 * 4 * 16)           # 16-row bands
        assert np.array_equal(gpu_rows(g, f), want)
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, -1)
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, 41)                   # no occupancy bits in LDS: a step reads the colour table
        assert np.array_equal(gpu_rows(g, f), want)
    finally:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, -1)
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)


@pytest.mark.parametrize("sub", [1, 2])
def test_strips_reassembled(sub):
    g, grid = scene("obj")
    full = voxel_frame(70, 100, depth=2.5, sub_pixel_res=sub)
    want = model_image(grid, full)
    got = np.zeros_like(want)
    for k in range(3):
        f = as_sr(voxel_frame(70, 100, depth=2.5, sub_pixel_res=sub, strips=(16, 3, k)))
        rows = [r for r in range(100) if (r // 16) % 3 == k]
        px, st = g.render(f, stats=True)
        assert px.size == len(rows) * 70 and int(st[0]) == int(st[1]) == len(rows) * 70 * sub * sub
        got[rows] = px.reshape(len(rows), 70)
    assert int(np.count_nonzero(got != want)) == 0


@pytest.mark.parametrize("parts", [2, 3])
def test_multi_device_scene(parts):
    g, grid = scene("cube20k", devices=[0] * parts)
    for kw in (dict(), dict(sub_pixel_res=2), dict(start_row=9, end_row=100)):
        f = voxel_frame(110, 130, depth=2.0, **kw)
        want = model_image(grid, f)
        got, st = gpu_rows(g, f, stats=True)
        assert int(np.count_nonzero(got != want)) == 0, kw
        assert g.last_frame_parts() == parts
        rays = want.size * f.sub_pixel_res ** 2
        assert [int(x) for x in st] == [rays, rays, 0, 0]
    dc, dn = g.get_voxels()
    assert np.array_equal(dc, grid[0]) and np.array_equal(dn.view(np.uint64), grid[1].view(np.uint64))


def test_rccl_render_and_surface_passes():
    torch = pytest.importorskip("torch")
    g, grid = scene("obj")
    f = voxel_frame(90, 75, depth=2.5, sub_pixel_res=2)
    want = model_image(grid, f)
    dev = torch.device("cuda", 0)
    r = sa.GpuScene(0)
    r.set_triangles(*load_obj3ds("obj.3ds"))
    r.rccl_init(sa.rccl_unique_id(), 1, 0)
    out = torch.zeros(90 * 75, dtype=torch.int32, device=dev)
    r.rccl_render(as_sr(f), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(75, 90), want)
    px = gpu_rows(g, f).reshape(-1)
    neg = g.post_process(px.copy(), sa._lib.STYLE_NEGATIVE, 0xFF00FF)
    assert np.array_equal(neg, orc.post_process(want.reshape(-1).copy(), orc.STYLE_NEGATIVE, 0xFF00FF))
    f1 = voxel_frame(90, 76, depth=2.5)
    hi = gpu_rows(g, f1)
    assert np.array_equal(g.anti_alias(hi.reshape(-1), 45, 38, 2), orc.anti_alias(model_image(grid, f1).reshape(-1), 45, 38, 2))


# ---- 5. what a voxel frame ignores, counts, refuses and leaves alone ----
def test_extra_geometry_and_trace_mode_do_not_change_a_voxel_frame():
    v9, argb, bmin, bmax = load_obj3ds("obj.3ds")
    g = sa.GpuScene(0)
    g.set_triangles(v9, argb, bmin, bmax)
    f = voxel_frame(100, depth=3.0)
    want = model_image(vm.voxelise(v9, argb)[:2], f)
    plain = gpu_rows(g, f)
    g.set_extra(c1_spheres(8))
    with_extra = [gpu_rows(g, f, mode=m) for m in (sa.MODE_REF_TREE, sa.MODE_BRUTE, sa.MODE_BVH, 77)]     # trace_mode is not read
    for got in [plain] + with_extra:
        assert np.array_equal(got, want)


def test_same_frame_three_times():
    g, grid = scene("cube20k")
    f = voxel_frame(128, 96, depth=1.8, sub_pixel_res=2)
    want = model_image(grid, f)
    for _ in range(3):
        got, st = gpu_rows(g, f, stats=True)
        assert np.array_equal(got, want) and [int(x) for x in st] == [128 * 96 * 4, 128 * 96 * 4, 0, 0]


def test_refused_combinations():
    g, _ = scene("obj")
    bad = [voxel_frame(64, shadows=True), voxel_frame(64, shadows=True, static_shadows=True)]
    f = voxel_frame(64); f.flags |= sa.F_PATH_TRACING; bad.append(f)
    f = voxel_frame(64); f.max_bounces = 1; f.reflectivity = 0.5; bad.append(f)
    f = voxel_frame(64); f.flags |= sa._lib.F_SINGLE_KERNEL; bad.append(f)
    for f in bad:
        with pytest.raises(sa.SoftrayError) as e:
            g.render(as_sr(f))
        assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED
    empty = sa.GpuScene(0)
    with pytest.raises(sa.SoftrayError) as e:
        empty.render(as_sr(voxel_frame(64)))
    assert e.value.code == sa._lib.SR_ERR_NO_MODEL


@pytest.mark.parametrize("mode", [sa.MODE_REF_TREE, sa.MODE_BVH])
def test_triangle_frames_on_the_same_scene_still_equal_the_oracle(mode):
    v9, argb, bmin, bmax = load_obj3ds("obj.3ds")
    g, o = sa.GpuScene(0), orc.Scene()
    for s in (g, o):
        s.set_triangles(v9, argb, bmin, bmax)
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH))
    assert o.build_tree() == 0
    plain = make_frame(100, depth=3.0, shadows=True, shadow_samples=16)
    before = gpu_rows(g, plain, mode=mode)
    vox = gpu_rows(g, voxel_frame(100, depth=3.0))                   # builds the grid between the two triangle frames
    after = gpu_rows(g, plain, mode=mode)
    want = np.zeros(100 * 100, dtype=np.uint32)
    o.render(plain, threads=os.cpu_count() or 8, out=want)
    assert np.array_equal(before.reshape(-1), want) and np.array_equal(after.reshape(-1), want)
    assert not np.array_equal(vox, after)
