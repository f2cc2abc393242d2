"""Path tracing (SR_F_PATH_TRACING, rayTracePathTracing) on the device: the reference's ten goldens through the C ABI and through the
Python Renderer mirror, and frames without a golden against the CPU model (tests/pathtrace_model.py, pinned to the goldens by
tests/test_pathtrace_model.py) -- bit for bit, every comparison an exact equality over every pixel."""
import json
import math
import os
import zlib

import numpy as np
import pytest

import pathtrace_model as ptm
import softray_amd as sa
from helpers import GOLDEN, c1_spheres, load_obj3ds, make_frame, orc, read_bmp_rgb, unit_cube_scene

pytestmark = pytest.mark.gpu
NCPU = os.cpu_count() or 8
MODES = {"tree": sa.MODE_REF_TREE, "brute": sa.MODE_BRUTE, "bvh": sa.MODE_BVH}


def golden_rgb(name):
    return read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))


def path_frame(w=100, h=None, **kw):
    f = make_frame(w, h, shading=kw.pop("shading", False), **kw)
    f.flags |= ptm.F_PATH_TRACING
    return f


def as_sr(frame, mode):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = mode
    return f


def gpu_rows(g, frame, mode, stats=False):
    """The frame's rows start_row..end_row as the library renders them, [rows, width]; the other rows must stay untouched."""
    f = as_sr(frame, mode)
    out = np.full(f.width * f.height, 0x01020304, dtype=np.uint32)
    _, st = g.render(f, out=out, stats=stats)
    a = min(max(0, f.start_row), f.height - 1)
    b = min(max(0, f.end_row), f.height - 1)
    px = out.reshape(f.height, f.width)
    assert np.all(px[:a] == 0x01020304) and np.all(px[b + 1:] == 0x01020304)
    return (px[a:b + 1].copy(), st) if stats else px[a:b + 1].copy()


def pair(v9, argb, bmin, bmax, prims=(), modes=(sa.MODE_REF_TREE, sa.MODE_BVH), on_device=None):
    g, o = sa.GpuScene(0), orc.Scene()
    for s in (g, o):
        s.set_triangles(v9, argb, bmin, bmax)
        if prims:
            s.set_extra(list(prims))
    g.build(tuple(modes), on_device=on_device)
    assert o.build_tree() == 0
    return g, o


@pytest.fixture(scope="module")
def obj2_pair():
    return pair(*load_obj3ds("obj2.3DS"))


@pytest.fixture(scope="module")
def obj_pair():
    return pair(*load_obj3ds("obj.3ds"))


@pytest.fixture(scope="module")
def primitives_pair():
    return pair(*load_obj3ds("obj.3ds"), prims=ptm.PRIMITIVES)


# ---- 1. the reference's goldens through the C ABI ----
@pytest.mark.parametrize("structure", ["tree", "bvh_device", "bvh_host"])
@pytest.mark.parametrize("name,kw", ptm.TRIANGLE_GOLDENS, ids=[n for n, _ in ptm.TRIANGLE_GOLDENS])
def test_PathTraceTrianglesTest_goldens(obj2_pair, name, kw, structure):
    g = obj2_pair[0]
    if structure == "bvh_host":
        g = pair(*load_obj3ds("obj2.3DS"), modes=(sa.MODE_BVH,), on_device=False)[0]
        assert g.bvh_stats()[3] == 0
    elif structure == "bvh_device":
        assert g.bvh_stats()[3] == 1
    got = gpu_rows(g, path_frame(**kw), sa.MODE_REF_TREE if structure == "tree" else sa.MODE_BVH)
    assert np.all(got >> 24 == 0xFF)
    assert int(np.count_nonzero((got & 0xFFFFFF) != golden_rgb(name))) == 0


@pytest.mark.parametrize("name,kw", ptm.SPHERE_GOLDENS, ids=[n for n, _ in ptm.SPHERE_GOLDENS])
def test_PathTracePrimitivesTest_goldens(primitives_pair, name, kw):
    got = gpu_rows(primitives_pair[0], path_frame(**kw), sa.MODE_REF_TREE)
    assert np.all(got >> 24 == 0xFF)
    assert int(np.count_nonzero((got & 0xFFFFFF) != golden_rgb(name))) == 0


# ---- 2. the same through the Python mirror of Engine3D.Renderer, written like RendererTests.RaytraceScenario ----
def mirror_scenario(model, objectDepth=1.0, focalBlur=False, focalDepth=None, subPixelRes=1, extraGeometry=None, resolution=100, **fields):
    from softray_amd.renderer import Instance, Renderer, Vector
    pixels = np.zeros(resolution * resolution, dtype=np.int32)
    with Renderer(0) as renderer:
        renderer.BackgroundColor = 0xff00ff
        renderer.SetRenderingSurface(resolution, resolution, pixels)
        with open(os.path.join(GOLDEN, model), "rb") as stream:
            renderer.Load3dsModelFromStream(stream)
        renderer.Instances.append(Instance(renderer.Model, Position=Vector(0.0, 0.0, objectDepth), Yaw=135.0 / 180.0 * math.pi,
                                           Pitch=-22.0 / 180.0 * math.pi, Roll=0.0))
        renderer.rayTrace = True
        renderer.rayTraceSubdivision = True
        renderer.rayTraceShading = False
        renderer.rayTracePathTracing = True
        renderer.rayTraceFocalBlur = focalBlur
        renderer.rayTraceFocalDepth = objectDepth + 0.5 if focalDepth is None else focalDepth
        renderer.rayTraceSubPixelRes = subPixelRes
        for k, v in fields.items():
            setattr(renderer, k, v)
        if extraGeometry is not None:
            renderer.ExtraGeometryToRaytrace = extraGeometry
        renderer.Render()
        assert renderer.NumRaysFired == resolution * resolution * subPixelRes ** 2
    return pixels.view(np.uint32).reshape(resolution, resolution)


@pytest.mark.parametrize("name,kw", ptm.TRIANGLE_GOLDENS + ptm.SPHERE_GOLDENS, ids=[n for n, _ in ptm.TRIANGLE_GOLDENS + ptm.SPHERE_GOLDENS])
def test_renderer_mirror_reproduces_the_goldens(name, kw):
    from softray_amd.renderer import Color, GeometryCollection, Sphere, Vector
    spheres = "geometry" in name
    extra = None
    if spheres:                                                      # RendererTests.cs:250-257
        extra = GeometryCollection()
        extra.Add(Sphere(Vector(0, -10000, 0), 9999.5, Color=Color.White))
        extra.Add(Sphere(Vector(-0.5, 0, -0.5), 0.5, Color=Color.Red))
        extra.Add(Sphere(Vector(+0.5, 0, +0.5), 0.5, Color=Color.Green))
        extra.Add(Sphere(Vector(+0.5, 0, -0.5), 0.5, Color=Color.Blue))
        extra.Add(Sphere(Vector(-0.5, 0, +0.5), 0.5, Color=Color.Yellow))
    got = mirror_scenario("obj.3ds" if spheres else "obj2.3DS", objectDepth=kw.get("depth", 1.0), focalBlur=kw.get("focal_blur", False),
                          focalDepth=kw.get("focal_depth"), subPixelRes=kw.get("sub_pixel_res", 1), extraGeometry=extra)
    assert np.all(got >> 24 == 0xFF)
    assert int(np.count_nonzero((got & 0xFFFFFF) != golden_rgb(name))) == 0


def build_cpp_pathtrace_tests(tmp_path):
    import subprocess
    from helpers import ROOT
    exe = str(tmp_path / "pathtrace_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pathtrace_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    return exe


def test_cpp_mirror_reproduces_the_goldens(tmp_path):
    """The ten goldens and the refusal of path tracing + shadows through softray_amd/host/Engine3D.hpp."""
    import subprocess
    exe = build_cpp_pathtrace_tests(tmp_path)
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL OK" in r.stdout
    assert r.stdout.count("diff=0") == 10 and "refused ok" in r.stdout


def test_renderer_mirror_refuses_path_tracing_with_shadows():
    with pytest.raises(NotImplementedError, match="rayTracePathTracing together with rayTraceShadows"):
        mirror_scenario("obj2.3DS", rayTraceShadows=True)
    for name in ("rayTraceAmbientOcclusion", "rayTraceLightField", "rayTraceVoxels"):
        with pytest.raises(NotImplementedError):
            mirror_scenario("obj2.3DS", **{name: True})


# ---- 3. against the model where no golden exists ----
def check_model(g, o, f, modes=("tree", "bvh")):
    want = {"tree": None, "bvh": None}
    for m in modes:
        key = "bvh" if m == "bvh" else "tree"
        if want[key] is None:
            want[key] = ptm.render(o, f, ptm.TRACE_NEAREST if key == "bvh" else ptm.TRACE_ROOT_TREE)
        got = gpu_rows(g, f, MODES[m])
        assert got.shape == want[key].shape
        assert int(np.count_nonzero(got != want[key])) == 0, m
    return want


def test_shading_on(obj_pair, obj2_pair):
    for g, o in (obj_pair, obj2_pair):
        w = check_model(g, o, path_frame(96, 80, shading=True))
        assert np.array_equal(w["tree"], w["bvh"])
        plain, _ = g.render(as_sr(make_frame(96, 80), sa.MODE_REF_TREE))
        assert np.count_nonzero(plain.reshape(80, 96) != w["tree"]) > 500        # the second ray changed the image
    check_model(*obj2_pair, path_frame(64, 48, shading=True, sub_pixel_res=3))
    check_model(*obj2_pair, path_frame(64, 48, shading=True, sub_pixel_res=2, focal_blur=True, point_light=False, specular=False))


@pytest.mark.parametrize("concurrency", [1, 3, 4, 7, 0, 500])
def test_concurrency_row_blocks(obj2_pair, concurrency):
    """67 rows: not divisible by 3, 4 or 7; 0 means the default 4; more blocks than rows gives one row per block."""
    g, o = obj2_pair
    images = []
    for n in (1, 2):
        f = path_frame(90, 67, sub_pixel_res=n, concurrency=concurrency)
        images.append(check_model(g, o, f)["tree"])
    if concurrency in (1, 7):
        other = ptm.render(o, path_frame(90, 67, concurrency=4))
        assert not np.array_equal(images[0], other)                             # the blocks really move the random sequence


def test_row_blocks_across_row_bands(obj2_pair):
    """Small row bands (test hook): a block's hit count carries from band to band, also where a band ends inside a block."""
    g, o = obj2_pair
    try:
        for band_samples, n, conc in ((16 * 90, 1, 3), (16 * 90, 1, 1), (16 * 96 * 4, 2, 4), (16 * 96 * 4, 2, 7)):
            g.debug_set(sa._lib.DBG_BAND_SAMPLES, band_samples)
            check_model(g, o, path_frame(90, 67, sub_pixel_res=n, concurrency=conc, shading=True))
            check_model(g, o, path_frame(90, 67, sub_pixel_res=n, concurrency=conc, start_row=9, end_row=60))
    finally:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, -1)


def test_row_window_moves_the_blocks(obj2_pair):
    g, o = obj2_pair
    for a, b in ((10, 57), (0, 0), (33, 99), (-5, 20), (50, 1000)):
        for conc in (4, 3):
            check_model(g, o, path_frame(100, 100, start_row=a, end_row=b, concurrency=conc))
    full = ptm.render(o, path_frame(100, 100))
    part = ptm.render(o, path_frame(100, 100, start_row=10, end_row=57))
    assert not np.array_equal(full[10:58], part)                                 # the window is not a crop of the full frame


def test_non_square_frames_and_another_seed(obj_pair):
    g, o = obj_pair
    for w, h in ((160, 50), (37, 121), (1, 64), (200, 3)):
        check_model(g, o, path_frame(w, h))
    base = path_frame(80, 60)
    seeded = path_frame(80, 60)
    seeded.random_seed = 42
    a = check_model(g, o, base)["tree"]
    b = check_model(g, o, seeded)["tree"]
    assert not np.array_equal(a, b)
    check_model(g, o, base)                                                     # back to the first seed: the table is made again


def test_extra_geometry_in_tree_and_brute_mode(primitives_pair):
    """Scenes with spheres: the model knows extra geometry only through the reference tree (trace target 2), whose result brute
    force shares on obj.3ds; SR_MODE_BVH gives the same image here (no leaf-face case in this scene)."""
    g, o = primitives_pair
    w = check_model(g, o, path_frame(72, 54, depth=3.0, shading=True), modes=("tree", "brute"))
    got = gpu_rows(g, path_frame(72, 54, depth=3.0, shading=True), sa.MODE_BVH)
    assert np.array_equal(got, w["tree"])


def test_sphere_only_scene():
    """c1_spheres alone.  A scene without a model draws nothing (SR_ERR_NO_MODEL, Renderer.cs:736-739), so the model is one
    triangle of 1e-3 in a corner of the box: every other hit, first or second, is a sphere's."""
    tri = np.array([[[0.499, 0.499, 0.499], [0.5, 0.499, 0.499], [0.499, 0.5, 0.499]]])
    g, o = pair(tri, np.array([0xFF123456], dtype=np.uint32), [-0.5] * 3, [0.5] * 3, prims=c1_spheres(), modes=(sa.MODE_REF_TREE,))
    for kw in (dict(), dict(shading=True, sub_pixel_res=2)):
        check_model(g, o, path_frame(96, 64, depth=3.0, **kw), modes=("tree", "brute"))


def test_every_sample_misses(obj2_pair):
    g, o = obj2_pair
    f = path_frame(64, 40, depth=-5.0)                                          # the model is behind the camera
    for n in (1, 2):
        f.sub_pixel_res = n
        got = gpu_rows(g, f, sa.MODE_BVH)
        assert np.all(got == 0xFFFF00FF)
        check_model(g, o, f)


# ---- 4. a scene that runs several workgroups per kernel and several bands: fixtures made by scripts/make_pathtrace_fixtures.py ----
@pytest.mark.parametrize("name", ["cube20k_640x480", "cube20k_640x480_2xAA"])
def test_cube20k_against_the_model_fixture(name):
    doc = json.load(open(os.path.join(GOLDEN, "pathtrace", name + ".json")))
    g = sa.GpuScene(0)
    g.set_triangles(*unit_cube_scene(doc["scene"]["triangles"]))
    g.build((sa.MODE_BVH,))
    f = path_frame(doc["width"], doc["height"], shading=True, depth=doc["frame"]["depth"], sub_pixel_res=doc["frame"].get("sub_pixel_res", 1))
    n2 = f.sub_pixel_res ** 2
    for band_samples in (-1, 48 * 640 * n2):                                    # whole frame in one band; ten bands of 48 rows
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, band_samples)
        got, st = gpu_rows(g, f, sa.MODE_BVH, stats=True)
        assert st[0] == 640 * 480 * n2
        assert len(doc["strips"]) == 30
        for s, crc in doc["strips"].items():
            s = int(s)
            assert zlib.crc32(np.ascontiguousarray(got[16 * s:16 * s + 16], dtype="<u4").tobytes()) & 0xFFFFFFFF == crc, (name, band_samples, s)
        assert int(np.count_nonzero(got == 0xFFFF00FF)) == doc["background_pixels"]
        rs = g.ray_stats()
        hits = 640 * 480 * n2 - int(np.count_nonzero(got == 0xFFFF00FF)) if n2 == 1 else None
        if hits is not None:
            assert rs[4] == hits                                                # one second ray per camera sample that hit


def test_bvh_second_rays_walk_route_equals_per_lane_walks(primitives_pair):
    """SR_MODE_BVH sends its second rays through the mirror extension's prepare / walk kernels; the per-lane form (hook 33) and the
    unsorted queue (hook 31) are independent schedules of the same result, with and without extra geometry, on both builds."""
    host = pair(*unit_cube_scene(20000), modes=(sa.MODE_BVH,), on_device=False)[0]
    dev = pair(*unit_cube_scene(20000), modes=(sa.MODE_BVH,))[0]
    for g, depth in ((host, 1.5), (dev, 1.5), (primitives_pair[0], 3.0)):
        for kw in (dict(shading=True), dict(sub_pixel_res=2, focal_blur=True)):
            f = path_frame(200, 150, depth=depth, **kw)
            a, st = gpu_rows(g, f, sa.MODE_BVH, stats=True)
            rays = g.ray_stats()[4]
            try:
                for hook in (33, 31):
                    g.debug_set(sa._lib.DBG_KERNEL_SWITCH, hook)
                    b, st_b = gpu_rows(g, f, sa.MODE_BVH, stats=True)
                    assert np.array_equal(a, b), hook
                    assert np.array_equal(st, st_b) and g.ray_stats()[4] == rays
            finally:
                g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
    assert np.array_equal(gpu_rows(host, path_frame(200, 150, depth=1.5, shading=True), sa.MODE_BVH),
                          gpu_rows(dev, path_frame(200, 150, depth=1.5, shading=True), sa.MODE_BVH))


# ---- 5. determinism, isolation, refusals ----
def test_same_frame_three_times(obj2_pair):
    g, _ = obj2_pair
    f = path_frame(128, 96, shading=True, sub_pixel_res=2)
    a = gpu_rows(g, f, sa.MODE_BVH)
    assert np.array_equal(a, gpu_rows(g, f, sa.MODE_BVH)) and np.array_equal(a, gpu_rows(g, f, sa.MODE_BVH))


def test_ordinary_frames_around_a_path_traced_one(obj_pair):
    g, o = obj_pair
    shadowed = make_frame(96, 72, shadows=True)
    bounce = make_frame(96, 72)
    bounce.max_bounces, bounce.reflectivity = 2, 0.5
    want_s, _ = o.render(shadowed, threads=NCPU)
    want_b, _ = o.render(bounce, threads=NCPU)
    for mode in (sa.MODE_REF_TREE, sa.MODE_BVH):
        for _ in range(2):
            assert np.array_equal(g.render(as_sr(shadowed, mode))[0], want_s)
            check_model(g, o, path_frame(96, 72, shading=True), modes=("tree",) if mode == sa.MODE_REF_TREE else ("bvh",))
            assert np.array_equal(g.render(as_sr(bounce, mode))[0], want_b)
            check_model(g, o, path_frame(64, 64, sub_pixel_res=2), modes=("bvh",))


def test_statistics_count_the_second_rays(obj2_pair):
    g, _ = obj2_pair
    f = path_frame(100, 100)
    got, st = gpu_rows(g, f, sa.MODE_REF_TREE, stats=True)
    hits = int(np.count_nonzero(got != 0xFFFF00FF))
    rs = g.ray_stats()
    assert st[0] == rs[0] == 10000 and rs[4] == hits and rs[5] > 0 and rs[6] > 0
    plain = make_frame(100, 100, shading=False)
    _, st_plain = g.render(as_sr(plain, sa.MODE_REF_TREE))
    assert np.array_equal(st, st_plain)                                         # the four statistics of sr_render count the primary rays
    f.flags |= sa._lib.F_PRIMARY_STATS_ONLY
    got2, st2 = gpu_rows(g, f, sa.MODE_REF_TREE, stats=True)
    assert np.array_equal(got, got2) and np.array_equal(st, st2) and all(v == 0 for v in g.ray_stats()[4:])


def test_unsupported_combinations(obj_pair):
    g, _ = obj_pair
    cases = []
    f = path_frame(32, 32, shadows=True); cases.append(f)
    f = path_frame(32, 32, shadows=True, static_shadows=True); cases.append(f)
    f = path_frame(32, 32); f.max_bounces, f.reflectivity = 1, 0.5; cases.append(f)
    f = path_frame(32, 32); f.flags |= sa._lib.F_SINGLE_KERNEL; cases.append(f)
    f = path_frame(32, 32, strips=(16, 2, 0)); cases.append(f)
    for f in cases:
        for mode in (sa.MODE_REF_TREE, sa.MODE_BVH):
            with pytest.raises(sa.SoftrayError) as e:
                g.render(as_sr(f, mode))
            assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED
    # one strip that owns every row is the whole frame
    check_model(*obj_pair, path_frame(48, 40), modes=("tree",))
    one = as_sr(path_frame(48, 40, strips=(16, 1, 0)), sa.MODE_REF_TREE)
    assert np.array_equal(g.render(one)[0].reshape(40, 48), gpu_rows(g, path_frame(48, 40), sa.MODE_REF_TREE))
    # the random table is capped: 12 bytes per sample of the largest row block
    big = path_frame(8192, 4096, concurrency=1)                                  # 32 Mi samples in one block: 384 MiB > the 256 MiB cap
    with pytest.raises(sa.SoftrayError) as e:
        g.render(as_sr(big, sa.MODE_BVH), stats=False)
    assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED
