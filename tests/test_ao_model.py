"""Ambient occlusion without a GPU: the flag on every layer, the cache calls on a host-only scene, and the invariants of the CPU model
(tests/ao_model.py) that tests/test_gpu_ao.py compares the device against."""
import os
import re
import subprocess

import numpy as np
import pytest

import ao_model as aom
import pathtrace_model as ptm
from helpers import GOLDEN, ROOT, load_obj3ds, make_frame, orc


def test_flags_are_declared_on_every_layer():
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    bits = dict(re.findall(r"\b(SR_F_[A-Z_]+)\s*=\s*1u\s*<<\s*(\d+)", header))
    assert bits.get("SR_F_AMBIENT_OCCLUSION") == "13" and bits.get("SR_F_AO_UNCACHED") == "14"
    values = [int(b) for b in bits.values()]
    assert len(set(values)) == len(values) and max(values) < 16
    assert "#define SR_ABI_VERSION 5" in header
    for sym in ("sr_reset_ao_cache", "sr_get_ao_cache", "sr_set_ao_cache"):
        assert re.search(r"\bint\s+%s\(" % sym, header), sym
    import softray_amd as sa
    assert sa._lib.F_AMBIENT_OCCLUSION == 1 << 13 == aom.F_AMBIENT_OCCLUSION == sa.F_AMBIENT_OCCLUSION
    assert sa._lib.F_AO_UNCACHED == 1 << 14 == aom.F_AO_UNCACHED == sa.F_AO_UNCACHED
    assert sa._lib.lib().sr_abi_version() == 5
    for sym in ("sr_reset_ao_cache", "sr_get_ao_cache", "sr_set_ao_cache"):
        assert sym in sa._lib.SYMBOLS and hasattr(sa._lib.lib(), sym)
    for rel in (("softray_amd", "host", "Engine3D.hpp"), ("bindings", "csharp", "GpuRenderer.cs")):
        src = open(os.path.join(ROOT, *rel)).read()
        assert "SR_F_AMBIENT_OCCLUSION" in src, rel
        for sym in ("sr_reset_ao_cache",) if "hpp" in rel[-1] else ("sr_reset_ao_cache", "sr_get_ao_cache", "sr_set_ao_cache"):
            assert sym in src, (rel, sym)
    # the Python mirror keeps refusing the switch (tests/test_pathtrace_model.py pins its list)
    src = open(os.path.join(ROOT, "softray_amd", "renderer.py")).read()
    refused = re.search(r"for name in \(([^)]*)\):\s*\n\s*if getattr\(self, name\):\s*\n\s*raise NotImplementedError", src)
    assert refused and "rayTraceAmbientOcclusion" in refused.group(1)


def host_scene():
    import softray_amd as sa
    s = sa.GpuScene(-1)
    s.set_triangles(*load_obj3ds("obj2.3DS"))
    return s


def test_cache_round_trip_on_a_host_only_scene():
    s = host_scene()
    assert s.get_ao_cache().shape == (128, 128, 128) and not s.get_ao_cache().any()      # never rendered: all zeros
    data = (np.arange(128 ** 3, dtype=np.uint32) * 2654435761 >> 24).astype(np.uint8).reshape(128, 128, 128)
    s.set_ao_cache(data)
    assert np.array_equal(s.get_ao_cache(), data)
    s.reset_ao_cache()
    assert not s.get_ao_cache().any()
    s.set_ao_cache(data)
    s.set_triangles(*load_obj3ds("obj2.3DS"))                                            # a new model drops the cache
    assert not s.get_ao_cache().any()
    s.set_ao_cache(data)
    s.load_3ds(open(os.path.join(GOLDEN, "obj2.3DS"), "rb").read())
    assert not s.get_ao_cache().any()
    with pytest.raises(ValueError):
        s.set_ao_cache(np.zeros(5, dtype=np.uint8))


def test_ao_frame_on_a_host_only_scene_is_refused():
    import softray_amd as sa
    s = host_scene()
    s.build((sa.MODE_REF_TREE,))
    f = sa.Frame.from_buffer_copy(bytes(aom.ao_frame(make_frame(16))))
    with pytest.raises(sa.SoftrayError) as e:
        s.render(f)
    assert e.value.code == sa._lib.SR_ERR_NO_DEVICE


def test_refused_combinations_are_refused_before_a_device_is_needed():
    """validate_frame runs before the device is looked at: a host-only scene answers SR_ERR_UNSUPPORTED for the refused pairs."""
    import softray_amd as sa
    s = host_scene()
    s.build((sa.MODE_REF_TREE,))
    for change in (dict(flags=sa.F_PATH_TRACING), dict(flags=sa.F_VOXELS), dict(flags=sa.F_SHADOWS | sa.F_STATIC_SHADOWS), dict(max_bounces=1),
                   dict(flags=sa._lib.F_SINGLE_KERNEL), dict(strips=(16, 2, 0))):
        f = sa.Frame.from_buffer_copy(bytes(aom.ao_frame(make_frame(16))))
        f.flags |= change.get("flags", 0)
        f.max_bounces = change.get("max_bounces", 0)
        if "strips" in change:
            f.strip_rows, f.strip_count, f.strip_index = change["strips"]
        with pytest.raises(sa.SoftrayError) as e:
            s.render(f)
        assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED and "ambient occlusion" in str(e.value), change


# ---- model invariants ----
def one_triangle_scene():
    """One triangle in the plane z = 0 whose normal faces the camera of the yaw-180 pose: nothing can occlude it."""
    o = orc.Scene()
    v9 = np.array([[(-0.4, -0.4, 0.0), (0.4, -0.4, 0.0), (0.0, 0.4, 0.0)]])
    o.set_triangles(v9, np.array([0xFF80C0FF], dtype=np.uint32), np.array([-0.5] * 3), np.array([0.5] * 3))
    assert o.build_tree() == 0
    return o


def facing_frame(o, res=24, **kw):
    """A pose in which the scene's single triangle is hit (whichever way it faces)."""
    for yaw in (180.0, 0.0):
        f = make_frame(res, shading=False, yaw_deg=yaw, pitch_deg=0.0, **kw)
        s, d = ptm.camera_samples(f)
        if o.trace(aom.TRACE_ROOT_TREE, s, d)["hit"].any():
            return f
    raise AssertionError("the triangle is not visible")


def test_unoccluded_point_gets_255():
    o = one_triangle_scene()
    f = aom.ao_frame(facing_frame(o), uncached=True)
    m = aom.AoModel()
    got = m.render(o, f)
    s, d = ptm.camera_samples(f)
    first = o.trace(aom.TRACE_ROOT_TREE, s, d)
    hit = first["hit"].astype(bool).reshape(got.shape)
    assert hit.any() and m.generators == int(hit.sum())
    # modulate(c, 255) = (c * 255) >> 8 per channel
    want = aom.modulate(first["color"], np.full(first["color"].shape, 255)).reshape(got.shape)
    assert np.array_equal(got[hit], want[hit]) and np.all(got[~hit] == 0xFFFF00FF)
    m2 = aom.AoModel()
    m2.render(o, aom.ao_frame(facing_frame(o)))
    filled = m2.cache[m2.cache != 0]
    assert filled.size == m2.generators and np.all(filled == 255)


def closed_box(lo, hi, argb=0xFFFFFFFF):
    """12 triangles, both windings irrelevant: Triangle.IntersectRay only accepts front faces, so every face is doubled."""
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    c = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    quads = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (3, 2, 6, 7), (0, 3, 7, 4), (1, 2, 6, 5)]
    tris = []
    for a, b, cc, d in quads:
        for t in ((a, b, cc), (a, cc, d)):
            tris.append([c[t[0]], c[t[1]], c[t[2]]])
            tris.append([c[t[0]], c[t[2]], c[t[1]]])
    return np.array(tris, dtype=np.float64), np.full(len(tris), argb, dtype=np.uint32)


def test_enclosed_point_gets_1():
    """A point at the centre of a closed box of half-size 0.1.  A probe (not normalised, components in [-1, 1]) reaches a wall at
    rayFrac <= 0.101 / max|d_i|, which is <= 2.0 for every probe whose largest component is at least 0.0505: checked for the seed's
    draws, so that no probe can escape and the byte must be 1."""
    bv, bc = closed_box((-0.1, -0.1, -0.1), (0.1, 0.1, 0.1))
    o = orc.Scene()
    o.set_triangles(bv, bc, np.array([-0.5] * 3), np.array([0.5] * 3))
    assert o.build_tree() == 0
    seed = 1234567890
    d = orc.Random(seed).NextDoubles(300).reshape(100, 3) * 2 - 1
    assert np.abs(d).max(axis=1).min() >= 0.0505
    pos = np.array([[0.0, 0.0, 0.0]])
    for nz in (1.0, -1.0):
        b = aom.probe_bytes(o, aom.TRACE_ROOT_TREE, pos, np.array([[0.0, 0.0, nz]]), np.array([0]), seed)
        assert b.tolist() == [1]
    # the same point with nothing around it
    assert aom.probe_bytes(one_triangle_scene(), aom.TRACE_ROOT_TREE, np.array([[0.0, 0.0, 0.3]]), np.array([[0.0, 0.0, 1.0]]), np.array([0]), 1).tolist() == [255]


@pytest.fixture(scope="module")
def obj2():
    o = orc.Scene()
    o.set_triangles(*load_obj3ds("obj2.3DS"))
    assert o.build_tree() == 0
    return o


def test_second_cached_frame_generates_nothing(obj2):
    m = aom.AoModel()
    f = aom.ao_frame(make_frame(40))
    a = m.render(obj2, f)
    assert m.generators > 0
    cache = m.cache.copy()
    b = m.render(obj2, f)
    assert m.generators == 0 and np.array_equal(a, b) and np.array_equal(cache, m.cache)
    m.reset()
    assert np.array_equal(m.render(obj2, f), a)


def test_generators_with_one_block_are_the_first_samples_per_cell(obj2):
    f = aom.ao_frame(make_frame(40, sub_pixel_res=2, concurrency=1))
    m = aom.AoModel()
    m.render(obj2, f)
    s, d = ptm.camera_samples(f)
    first = obj2.trace(aom.TRACE_ROOT_TREE, s, d)
    hi = np.nonzero(first["hit"])[0]
    cell = aom.cells(aom.clamp_pos(first["pos"][hi]))
    _, where = np.unique(cell, return_index=True)                       # first occurrence in scan order
    assert np.array_equal(np.sort(hi[where]), m.generator_samples)
    assert np.array_equal(m.generator_k, np.arange(m.generators))       # one block: k counts the generators in scan order
    # more blocks: another order, another set of generators (the order is the library's, include/softray.h)
    m4 = aom.AoModel()
    m4.render(obj2, aom.ao_frame(make_frame(40, sub_pixel_res=2, concurrency=4)))
    assert m4.generators == m.generators and not np.array_equal(m4.generator_samples, m.generator_samples)


def test_uncached_k_is_the_path_tracers_hit_index(obj2):
    for conc in (1, 3, 0):
        f = aom.ao_frame(make_frame(36, 30, concurrency=conc), uncached=True)
        m = aom.AoModel()
        m.render(obj2, f)
        s, d = ptm.camera_samples(f)
        hit = obj2.trace(aom.TRACE_ROOT_TREE, s, d)["hit"].astype(np.int64)
        k = ptm.hit_indices(hit, f.width, f.height, f.concurrency)
        assert m.generators == int(hit.sum()) and np.array_equal(m.generator_k, k[hit.astype(bool)])
        assert not m.cache.any()                                        # nothing is stored


def test_cpp_mirror_ao_program_builds(tmp_path):
    """tests/cpp/ao_tests.cpp compiles against Engine3D.hpp; without a GPU the program fails loudly instead of computing anything."""
    import torch
    exe = str(tmp_path / "ao_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "ao_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    if not torch.cuda.is_available():
        expected = tmp_path / "expected.bin"
        np.zeros(2 * 100 * 100, dtype=np.uint32).tofile(str(expected))
        r = subprocess.run([exe, GOLDEN, str(expected)], capture_output=True, text=True)
        assert r.returncode == 3 and "no HIP device" in r.stderr
