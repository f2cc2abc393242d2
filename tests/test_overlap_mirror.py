"""sr_overlap_triangles above the C ABI: the call is declared on every layer, it refuses what needs no device on a host-only scene -- in the
header's order, with its messages, the outputs untouched -- and the C++ mirror's Renderer::OverlapTriangles() (softray_amd/host/Engine3D.hpp)
is driven by tests/cpp/overlap_triangles_tests.cpp, a program that links against the ABI and knows every answer it asks for."""
import os
import re
import subprocess

import pytest

from helpers import ROOT


def build_program(tmp_path):
    exe = str(tmp_path / "overlap_triangles_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "overlap_triangles_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    return exe


def test_the_call_is_declared_on_every_layer():
    import softray_amd as sa
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert re.search(r"int\s+sr_overlap_triangles\(sr_scene\*, int32_t target, int64_t n, const double\* tris", header)
    assert re.search(r"int\s+sr_overlap_triangles_device\(sr_scene\*, int32_t target, int64_t n, const double\* d_tris, int32_t max_hits", header)
    assert "#define SR_ABI_VERSION 5" in header and "#define SR_OVERLAP_ANY 4u" in header
    assert "56 sr_overlap_triangles walks a pass in input order" in header and "57 sr_overlap_triangles" in header
    for out_of_scope in ("the intersection segment or contact points", "penetration depth", "excluding the neighbours in a self-query",
                         "the four-wide tree and persistent lanes", "a split over devices", "coplanar overlap"):
        assert out_of_scope in header, out_of_scope
    assert "sr_overlap_triangles" in sa._lib.SYMBOLS and "sr_overlap_triangles_device" in sa._lib.SYMBOLS and sa._lib.OVERLAP_ANY == 4
    lib = sa._lib.lib()
    assert hasattr(lib, "sr_overlap_triangles") and hasattr(lib, "sr_overlap_triangles_device")
    assert callable(sa.GpuScene.overlap_triangles) and callable(sa.GpuScene.overlap_triangles_device)
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "void OverlapTriangles(int64_t n, const double* tris, int32_t max_hits, uint32_t* count, int32_t* index, uint8_t* mask" in hpp
    assert "sr_overlap_triangles(" in hpp
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    assert "public OverlapTriangleLists OverlapTriangles(" in cs and "public void OverlapTrianglesDevice(" in cs
    assert "sr_overlap_triangles(IntPtr scene, int target, long n," in cs and "sr_overlap_triangles_device(IntPtr scene, int target, long n," in cs
    for doc, word in (("README.md", "sr_overlap_triangles"), ("DESIGN.md", "5.35"), ("INTEGRATION.md", "sr_overlap_triangles"),
                      (os.path.join("scripts", "README.md"), "gpu_overlap_triangles.py")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc
    makefile = open(os.path.join(ROOT, "softray_amd", "csrc", "Makefile")).read()
    assert "sr_overlap.hip" in makefile
    kernels = open(os.path.join(ROOT, "softray_amd", "csrc", "sr_kernels.hip")).read()
    assert '"k_overlap"' in kernels and '"k_overlap_sort"' in kernels
    # one text for the predicate and the row: the kernels and the host check include the same header
    for user in (os.path.join("softray_amd", "csrc", "sr_overlap.hip"), os.path.join("tests", "cpp", "tri_overlap_check.cpp")):
        assert "sr_tri_overlap.h" in open(os.path.join(ROOT, user)).read(), user
    kernel_text = open(os.path.join(ROOT, "softray_amd", "csrc", "sr_overlap.hip")).read()
    assert "k_ot_walk" in kernel_text and "k_ot_loop" in kernel_text


def test_the_call_refuses_what_needs_no_device():
    """The refusals that come before the device is looked at, in the header's order, on a host-only scene and without one."""
    import ctypes as C

    import numpy as np

    import softray_amd as sa
    from helpers import unit_cube_scene
    L = sa._lib
    q = np.zeros((2, 3, 3))
    cnt = np.full(2, 7, dtype=np.uint32); idx = np.full((2, 3), 7, dtype=np.int32); msk = np.full((2, 3), 7, dtype=np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                                  # noqa: E731
    lib = L.lib()

    def call(h, target, n, a, k, options):
        rc = lib.sr_overlap_triangles(h, target, n, p(a), k, p(cnt), p(idx), p(msk), options, None)
        return rc, (lib.sr_last_error().decode() if rc else "")

    def call_device(h, target, n, a, k, options):
        rc = lib.sr_overlap_triangles_device(h, target, n, p(a), k, p(cnt), p(idx), p(msk), options, None, None)
        return rc, (lib.sr_last_error().decode() if rc else "")

    bare = sa.GpuScene(-1)                                                    # host-only, no model
    host = sa.GpuScene(-1)                                                    # host-only, a model and its reference tree
    host.set_triangles(*unit_cube_scene(100))
    host.build((sa.MODE_REF_TREE,))
    vox, root, bvh, tree, brute = L.TARGET_VOXELS, L.TARGET_ROOT, sa.MODE_BVH, sa.MODE_REF_TREE, sa.MODE_BRUTE
    ANY = L.OVERLAP_ANY
    hits_text = "sr_overlap_triangles: max_hits must be 0 .. SR_HITS_MAX (64)"
    options_text = "sr_overlap_triangles: unknown option bits (SR_POINTS_COHERENT and SR_OVERLAP_ANY are the options)"
    any_text = "sr_overlap_triangles: SR_OVERLAP_ANY answers with a count of 0 or 1 and keeps no rows: max_hits must be 0"
    root_text = "sr_overlap_triangles: the extra geometry (SR_TARGET_ROOT) is not made of triangles with indices; pass the mode alone"
    no_device = "sr_overlap_triangles: a host-only scene has no HIP device to walk on (compute is never emulated on the CPU)"
    # every row breaks the rule it names and every later one it can: the earliest refusal is the one reported
    table = [
        ((None, vox, -1, None, 65, 2), L.SR_ERR_INVALID_ARG, "sr_overlap_triangles: the scene is NULL"),
        ((bare._h, vox, -1, None, 65, 2), L.SR_ERR_INVALID_ARG, "sr_overlap_triangles: n is negative"),
        ((bare._h, vox, 2, None, 65, 2), L.SR_ERR_INVALID_ARG, "sr_overlap_triangles: tris must not be NULL when n > 0"),
        ((bare._h, vox, 2, q, 65, 2), L.SR_ERR_INVALID_ARG, hits_text),
        ((bare._h, vox, 0, None, -1, 2), L.SR_ERR_INVALID_ARG, hits_text),
        ((bare._h, vox, 2, q, 3, 2 | ANY), L.SR_ERR_INVALID_ARG, options_text),
        ((bare._h, vox, 0, None, 64, 1 << 31), L.SR_ERR_INVALID_ARG, options_text),
        ((bare._h, vox, 2, q, 3, ANY), L.SR_ERR_INVALID_ARG, any_text),
        ((bare._h, vox | root | tree, 0, None, 1, ANY | 1), L.SR_ERR_INVALID_ARG, any_text),
        ((bare._h, vox | root | tree, 2, q, 3, 1), L.SR_ERR_UNSUPPORTED, "sr_overlap_triangles: the voxel grid (SR_TARGET_VOXELS) has no triangles to cross"),
        ((bare._h, vox, 2, q, 0, ANY), L.SR_ERR_UNSUPPORTED, "sr_overlap_triangles: the voxel grid (SR_TARGET_VOXELS) has no triangles to cross"),
        ((bare._h, root | tree, 2, q, 3, 0), L.SR_ERR_UNSUPPORTED, root_text),
        ((bare._h, root | bvh, 0, None, 0, 0), L.SR_ERR_UNSUPPORTED, root_text),
        ((bare._h, tree, 2, q, 3, 0), L.SR_ERR_UNSUPPORTED, None),
        ((host._h, tree, 0, None, 0, ANY), L.SR_ERR_UNSUPPORTED, None),
        ((bare._h, bvh, 2, q, 3, 0), L.SR_ERR_NO_MODEL, "sr_overlap_triangles: the scene has no model (sr_set_triangles, sr_load_3ds)"),
        ((host._h, bvh, 2, q, 3, 0), L.SR_ERR_NOT_BUILT, "SR_MODE_BVH needs sr_build(1 << SR_MODE_BVH)"),
        ((host._h, brute, 2, q, 3, 1), L.SR_ERR_NO_DEVICE, no_device),
        ((host._h, brute, 2, q, 0, ANY), L.SR_ERR_NO_DEVICE, no_device),
        ((host._h, brute, 0, None, 0, 0), L.SR_ERR_NO_DEVICE, no_device),
    ]
    for args, code, message in table:
        for fn in (call, call_device):
            rc, text = fn(*args)
            assert rc == code, (args[1:], text)
            if message is None:                                               # the reference tree: the message says why
                assert text.startswith("sr_overlap_triangles: SR_MODE_REF_TREE has no overlap query") and "several leaves" in text
            else:
                assert text == message
            assert np.all(cnt == 7) and np.all(idx == 7) and np.all(msk == 7)
    with pytest.raises(sa.SoftrayError):
        host.overlap_triangles(brute, q)


def test_cpp_mirror_overlap_triangles_program_builds(tmp_path):
    """The program compiles against Engine3D.hpp and links against the ABI; without a GPU it fails loudly instead of computing anything."""
    import torch
    exe = build_program(tmp_path)
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 3 and "no HIP device" in r.stderr


@pytest.mark.gpu
def test_cpp_mirror_overlap_triangles(tmp_path):
    exe = build_program(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL OK" in r.stdout
    assert r.stdout.count("  ok") == 16 and "FAILED" not in r.stdout
