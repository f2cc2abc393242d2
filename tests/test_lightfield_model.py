"""The colour light field without a GPU: the CPU model (tests/lightfield_model.py) against the reference's goldens, the flag on every layer,
the cache calls on a host-only scene, and the input conditions of every frame tests/test_gpu_lightfield.py compares the device against."""
import os
import re
import subprocess

import numpy as np
import pytest

import lightfield_model as lfm
from helpers import GOLDEN, ROOT, load_obj3ds, make_frame, orc, read_bmp_rgb, unit_cube_scene

GOLDEN_DIR = os.path.join(GOLDEN, "raytrace", "100x100")
TARGETS = {"root_tree": lfm.TRACE_ROOT_TREE, "nearest": lfm.TRACE_NEAREST}


def oracle_scene(model, prims=()):
    o = orc.Scene()
    o.set_triangles(*(unit_cube_scene(2000) if model == "unit_cube_2000" else load_obj3ds(model)))
    if prims:
        o.set_extra(list(prims))
    assert o.build_tree() == 0
    return o


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(model, prims=()):
        key = (model, bool(prims))
        if key not in made:
            made[key] = oracle_scene(model, prims)
        return made[key]
    return get


# ---- 1. the eight goldens, from an empty cache ----
@pytest.mark.parametrize("target", sorted(TARGETS))
@pytest.mark.parametrize("name", [g[0] for g in lfm.GOLDENS])
def test_golden_from_an_empty_cache(scenes, name, target):
    kw = dict(lfm.GOLDENS)[name]
    m = lfm.LightFieldModel(64)
    got = m.render(scenes("obj.3ds"), lfm.lf_frame(make_frame(100, **kw)), TARGETS[target]) & 0xFFFFFF
    want = read_bmp_rgb(os.path.join(GOLDEN_DIR, name + ".bmp"))
    assert int(np.count_nonzero(got != want)) == 0
    assert m.filled.size > 1000 and len(m.cache) == m.filled.size
    # the light field is visible: the golden is not the plain frame of the same name
    plain = read_bmp_rgb(os.path.join(GOLDEN_DIR, name.replace("_lightFieldColor", "") + ".bmp"))
    assert np.count_nonzero(plain != want) > 0


def test_warm_second_call_fills_nothing(scenes):
    o = scenes("obj.3ds")
    m = lfm.LightFieldModel(64)
    f = lfm.lf_frame(make_frame(100, sub_pixel_res=2, focal_blur=True))
    a = m.render(o, f)
    filled = m.filled.size
    cache = dict(m.cache)
    b = m.render(o, f)
    assert filled > 1000 and m.filled.size == 0 and np.array_equal(a, b) and cache == m.cache
    m.reset()
    assert np.array_equal(m.render(o, f), a) and m.filled.size == filled


def test_a_cell_colour_does_not_depend_on_who_fills_it(scenes):
    """The cells a neighbouring view has already filled change nothing in the next one: every cell holds the colour of its own canonical ray.
    (Without shading: a SHADED colour also depends on the pose of the frame that filled the cell, in the reference as here.)"""
    o = scenes("obj.3ds")
    second = dict(yaw_deg=137.0, shading=False)
    fresh = lfm.LightFieldModel(64)
    want = fresh.render(o, lfm.lf_frame(make_frame(100, **second)))
    m = lfm.LightFieldModel(64)
    m.render(o, lfm.lf_frame(make_frame(100, shading=False)))
    got = m.render(o, lfm.lf_frame(make_frame(100, **second)))
    assert np.array_equal(got, want) and 0 < m.filled.size < fresh.filled.size        # some of its cells were there, some were not
    assert all(m.cache[k] == v for k, v in fresh.cache.items())


def test_index_is_injective_and_patch_centres_map_to_their_own_cell():
    n = 8
    u, v, s, t = np.meshgrid(np.arange(2 * n), np.arange(n), np.arange(2 * n), np.arange(n), indexing="ij")
    index = (u * n * n * n * 2 + v * n * n * 2 + s * n + t).reshape(-1)
    assert np.array_equal(np.sort(index), np.arange(lfm.cache_entries(n)))
    for got, want in zip(lfm.decode(index, n), (u, v, s, t)):
        assert np.array_equal(got, want.reshape(-1))
    # a line through two patch centres (not the same patch, not on the poles' seam) falls into the cell of those two patches
    pts = lfm.sphere_points(n)
    a, b = pts[3, 2], pts[11, 5]
    idx, margin, _ = lfm.sample_cells((a - (b - a))[None, :], (b - a)[None, :], n)
    assert lfm.decode(idx, n) == tuple(np.array([x]) for x in (3, 2, 11, 5)) and margin > 0.05


def test_sphere_miss_and_threshold():
    """A line at distance r from the origin has term = R^2 - r^2: inside just below R, the background just above."""
    d = np.array([[0.0, 0.0, 1.0]] * 2)
    s = np.array([[lfm.RADIUS - 1e-3, 0.0, -3.0], [lfm.RADIUS + 1e-3, 0.0, -3.0]])
    idx, _, term_margin = lfm.sample_cells(s, d, 16)
    assert idx[0] >= 0 and idx[1] == -1 and 1e-3 < term_margin < 2e-3


# ---- 2. the input conditions of the frames the GPU tests use ----
@pytest.mark.parametrize("name", sorted(lfm.GPU_FRAMES))
def test_gpu_frame_keeps_clear_of_cell_boundaries(scenes, name):
    model, prims, n, f = lfm.gpu_frame(name)
    m = lfm.LightFieldModel(n)
    m.render(scenes(model, prims), f)
    print("%s: coordinate margin %.3g, term margin %.3g, %d cells filled" % (name, m.coord_margin, m.term_margin, m.filled.size))
    assert m.coord_margin > lfm.MARGIN and m.term_margin > lfm.MARGIN
    assert m.filled.size > 0


def test_known_boundary_poses_are_detected(scenes):
    """Pitch -30 degrees makes asin(0.5) land on v = 42 at resolution 64: the condition must catch such a pose."""
    m = lfm.LightFieldModel(64)
    m.render(scenes("obj.3ds"), lfm.lf_frame(make_frame(100, pitch_deg=-30.0)))
    assert m.coord_margin < lfm.MARGIN


def test_expected_cell_counts(scenes):
    """The figures the GPU tests are built around."""
    def run(name):
        model, prims, n, f = lfm.gpu_frame(name)
        m = lfm.LightFieldModel(n)
        m.render(scenes(model, prims), f)
        idx, _, _ = lfm.sample_cells(*lfm.ptm.camera_samples(f), n)
        return idx, m
    idx, m = run("contention")
    assert idx.size == 49152 and m.filled.size == 7
    idx, m = run("small_blur")
    assert m.filled.size == 36
    idx, m = run("far")
    assert idx.size == 1073 and int((idx >= 0).sum()) == 560
    idx, m = run("inside_sphere")
    assert (idx >= 0).all()                                 # the camera is inside the sphere (depth 0.6 < 0.866): no refusal, every line pierces it


# ---- 3. every layer ----
def test_flag_is_declared_on_every_layer():
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    bits = dict(re.findall(r"\b(SR_F_[A-Z_]+)\s*=\s*1u\s*<<\s*(\d+)", header))
    assert bits.get("SR_F_LIGHT_FIELD") == "15"
    values = [int(b) for b in bits.values()]
    assert len(set(values)) == len(values) and max(values) < 16          # bit 15 was the free one
    assert "#define SR_ABI_VERSION 5" in header
    symbols = ("sr_set_light_field_res", "sr_reset_light_field", "sr_get_light_field", "sr_set_light_field")
    for sym in symbols:
        assert re.search(r"\bint\s+%s\(" % sym, header), sym
    import softray_amd as sa
    assert sa._lib.F_LIGHT_FIELD == 1 << 15 == lfm.F_LIGHT_FIELD == sa.F_LIGHT_FIELD
    assert sa._lib.lib().sr_abi_version() == 5
    for sym in symbols:
        assert sym in sa._lib.SYMBOLS and hasattr(sa._lib.lib(), sym)
    for attr in ("light_field_res", "reset_light_field", "get_light_field", "set_light_field"):
        assert hasattr(sa.GpuScene, attr), attr
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "SR_F_LIGHT_FIELD" in hpp and "LightFieldStoresTriangles" in hpp and "rayTraceLightField" in hpp and "sr_reset_light_field" in hpp
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    assert "SR_F_LIGHT_FIELD" in cs and re.search(r"F_LIGHT_FIELD\s*=\s*1u\s*<<\s*15", cs)
    for sym in symbols:
        assert sym in cs, sym
    # the Python mirror keeps refusing the switch (tests/test_pathtrace_model.py pins its list)
    src = open(os.path.join(ROOT, "softray_amd", "renderer.py")).read()
    refused = re.search(r"for name in \(([^)]*)\):\s*\n\s*if getattr\(self, name\):\s*\n\s*raise NotImplementedError", src)
    assert refused and [s.strip().strip('"') for s in refused.group(1).split(",")] == ["rayTraceAmbientOcclusion", "rayTraceLightField", "rayTraceVoxels"]


def host_scene():
    import softray_amd as sa
    s = sa.GpuScene(-1)
    s.set_triangles(*load_obj3ds("obj2.3DS"))
    return s


def test_cache_calls_on_a_host_only_scene():
    import softray_amd as sa
    s = host_scene()
    assert s.light_field_res == 64
    for bad in (0, 129, -3):
        with pytest.raises(sa.SoftrayError) as e:
            s.light_field_res = bad
        assert e.value.code == sa._lib.SR_ERR_INVALID_ARG
    assert s.light_field_res == 64
    s.light_field_res = 8
    total = lfm.cache_entries(8)
    assert s.get_light_field().shape == (total,) and not s.get_light_field().any()       # never rendered: all zeros
    data = (np.arange(1000, dtype=np.uint32) * np.uint32(2654435761)) | np.uint32(1)
    s.set_light_field(data, first=5000)
    assert np.array_equal(s.get_light_field(5000, 1000), data)
    full = s.get_light_field()
    assert np.array_equal(full[5000:6000], data) and not full[:5000].any() and not full[6000:].any()
    assert np.array_equal(s.get_light_field(5990, 20), np.concatenate([data[-10:], np.zeros(10, dtype=np.uint32)]))
    for first, count in ((total - 5, 6), (total + 1, 0)):
        with pytest.raises(sa.SoftrayError) as e:
            s.get_light_field(first, count)
        assert e.value.code == sa._lib.SR_ERR_INVALID_ARG
    with pytest.raises(sa.SoftrayError):
        s.set_light_field(data, first=total - 999)
    s.reset_light_field()
    assert not s.get_light_field().any()
    s.set_light_field(data, first=0)
    s.set_triangles(*load_obj3ds("obj2.3DS"))                                             # a new model drops the cache
    assert not s.get_light_field().any()
    s.set_light_field(data, first=0)
    s.load_3ds(open(os.path.join(GOLDEN, "obj2.3DS"), "rb").read())
    assert not s.get_light_field().any()
    s.set_light_field(data, first=0)
    s.light_field_res = 8                                                                 # the same N: nothing is dropped
    assert np.array_equal(s.get_light_field(0, 1000), data)
    s.light_field_res = 9                                                                 # another N: another table
    assert s.get_light_field().shape == (lfm.cache_entries(9),) and not s.get_light_field().any()


def test_refused_combinations_are_refused_before_a_device_is_needed():
    """validate_frame runs before the device is looked at: a host-only scene answers SR_ERR_UNSUPPORTED for the refused combinations."""
    import softray_amd as sa
    s = host_scene()
    s.build((sa.MODE_REF_TREE,))
    for change in lfm.REFUSED:
        f = sa.Frame.from_buffer_copy(bytes(lfm.lf_frame(make_frame(16))))
        lfm.apply_change(f, change)
        with pytest.raises(sa.SoftrayError) as e:
            s.render(f)
        assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED and "light field" in str(e.value), change
    f = sa.Frame.from_buffer_copy(bytes(lfm.lf_frame(make_frame(16))))
    with pytest.raises(sa.SoftrayError) as e:
        s.render(f)
    assert e.value.code == sa._lib.SR_ERR_NO_DEVICE                                       # the plain light-field frame only lacks a device


def test_cpp_mirror_lightfield_program_builds(tmp_path):
    """tests/cpp/lightfield_tests.cpp compiles against Engine3D.hpp; without a GPU the program fails loudly instead of computing anything."""
    import torch
    exe = str(tmp_path / "lightfield_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "lightfield_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    if not torch.cuda.is_available():
        r = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
        assert r.returncode == 3 and "no HIP device" in r.stderr
