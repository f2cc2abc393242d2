"""The CPU model of path tracing (tests/pathtrace_model.py) against the reference's own goldens, before it judges the GPU path
(tests/test_gpu_pathtrace.py): PathTraceTrianglesTest and PathTracePrimitivesTest (RendererTests.cs:247-281), 0 differing pixels
each.  Plus the source-level checks that the flag exists on every layer (no GPU needed)."""
import os
import re

import numpy as np
import pytest

import pathtrace_model as ptm
from helpers import GOLDEN, ROOT, load_obj3ds, make_frame, orc, read_bmp_rgb


def golden_rgb(name):
    return read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))


def path_frame(res=100, **kw):
    f = make_frame(res, shading=kw.pop("shading", False), **kw)
    f.flags |= ptm.F_PATH_TRACING
    return f


@pytest.fixture(scope="module")
def triangles_scene():
    s = orc.Scene()
    s.set_triangles(*load_obj3ds("obj2.3DS"))
    assert s.build_tree() == 0
    return s


@pytest.fixture(scope="module")
def primitives_scene():
    s = orc.Scene()
    s.set_triangles(*load_obj3ds("obj.3ds"))
    assert s.build_tree() == 0
    s.set_extra(ptm.PRIMITIVES)
    return s


@pytest.mark.parametrize("name,kw", ptm.TRIANGLE_GOLDENS, ids=[n for n, _ in ptm.TRIANGLE_GOLDENS])
def test_model_reproduces_PathTraceTrianglesTest(triangles_scene, name, kw):
    gold = golden_rgb(name)
    got = ptm.render(triangles_scene, path_frame(**kw))
    assert got.shape == gold.shape and np.all(got >> 24 == 0xFF)
    assert int(np.count_nonzero((got & 0xFFFFFF) != gold)) == 0
    # triangle-only scene: the global nearest hit (the own BVH's semantics) gives the same image
    got3 = ptm.render(triangles_scene, path_frame(**kw), ptm.TRACE_NEAREST)
    assert int(np.count_nonzero((got3 & 0xFFFFFF) != gold)) == 0
    assert int(np.count_nonzero(gold != 0xff00ff)) > 500           # the golden shows the model


@pytest.mark.parametrize("name,kw", ptm.SPHERE_GOLDENS, ids=[n for n, _ in ptm.SPHERE_GOLDENS])
def test_model_reproduces_PathTracePrimitivesTest(primitives_scene, name, kw):
    gold = golden_rgb(name)
    got = ptm.render(primitives_scene, path_frame(**kw))
    assert int(np.count_nonzero((got & 0xFFFFFF) != gold)) == 0


def test_hit_indices_restart_in_every_row_block():
    rng = np.random.default_rng(5)
    hit = (rng.random(7 * 10) < 0.4).astype(np.int64)                # 7 rows of 10 samples
    for conc, bh in ((1, 7), (3, 3), (4, 2), (7, 1), (0, 2), (50, 1)):
        idx = ptm.hit_indices(hit, 10, 7, conc)
        for r0 in range(0, 7, bh):
            seg = hit[r0 * 10:(r0 + bh) * 10]
            assert np.array_equal(idx[r0 * 10:(r0 + bh) * 10], np.cumsum(seg) - seg), (conc, r0)


def test_flag_is_declared_on_every_layer():
    """include/softray.h declares SR_F_PATH_TRACING on a free bit, the ctypes layer exposes the same value, and the Python mirror no
    longer lists rayTracePathTracing among the switches it refuses."""
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    m = re.search(r"\bSR_F_PATH_TRACING\s*=\s*1u\s*<<\s*(\d+)", header)
    assert m, "include/softray.h does not declare SR_F_PATH_TRACING"
    bit = int(m.group(1))
    others = {int(b) for n, b in re.findall(r"\b(SR_F_[A-Z_]+)\s*=\s*1u\s*<<\s*(\d+)", header) if n != "SR_F_PATH_TRACING"}
    assert bit not in others and bit < 16
    assert "#define SR_ABI_VERSION 5" in header
    import softray_amd as sa
    assert sa._lib.F_PATH_TRACING == 1 << bit == ptm.F_PATH_TRACING and sa.F_PATH_TRACING == sa._lib.F_PATH_TRACING
    src = open(os.path.join(ROOT, "softray_amd", "renderer.py")).read()
    refused = re.search(r"for name in \(([^)]*)\):\s*\n\s*if getattr\(self, name\):\s*\n\s*raise NotImplementedError", src)
    assert refused, "renderer.py: the list of refused switches has moved"
    names = re.findall(r'"(\w+)"', refused.group(1))
    assert "rayTracePathTracing" not in names
    assert sorted(names) == ["rayTraceAmbientOcclusion", "rayTraceLightField", "rayTraceVoxels"]
    assert "F_PATH_TRACING" in src
    for rel in (("softray_amd", "host", "Engine3D.hpp"), ("bindings", "csharp", "GpuRenderer.cs")):
        assert "PATH_TRACING" in open(os.path.join(ROOT, *rel)).read(), rel


def test_cpp_mirror_path_tracing_program_builds(tmp_path):
    """tests/cpp/pathtrace_tests.cpp compiles against Engine3D.hpp (rayTracePathTracing is a field the mirror passes on); without a
    GPU the program fails loudly instead of computing anything."""
    import subprocess
    import torch
    exe = str(tmp_path / "pathtrace_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pathtrace_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    if not torch.cuda.is_available():
        r = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
        assert r.returncode == 3 and "no HIP device" in r.stderr
