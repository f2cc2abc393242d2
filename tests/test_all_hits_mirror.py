"""sr_all_hits_rays above the C ABI: the call is declared on every layer, it refuses what needs no device on a host-only scene, and the C++
mirror's Renderer::AllHitRays() (softray_amd/host/Engine3D.hpp) is driven by tests/cpp/all_hits_tests.cpp, a program that links against the ABI
and knows every answer it asks for."""
import os
import re
import subprocess

import pytest

from helpers import ROOT


def build_program(tmp_path):
    exe = str(tmp_path / "all_hits_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "all_hits_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    return exe


def test_the_call_is_declared_on_every_layer():
    import softray_amd as sa
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert re.search(r"int\s+sr_all_hits_rays\(sr_scene\*, int32_t target, int64_t n, const double\* starts, const double\* dirs,", header)
    assert re.search(r"int\s+sr_all_hits_rays_device\(sr_scene\*, int32_t target, int64_t n, const double\* d_starts, const double\* d_dirs,", header)
    assert "#define SR_HITS_MAX 64" in header and "#define SR_ABI_VERSION 5" in header
    assert "sr_all_hits_rays" in sa._lib.SYMBOLS and "sr_all_hits_rays_device" in sa._lib.SYMBOLS
    assert sa._lib.HITS_MAX == 64
    lib = sa._lib.lib()
    assert hasattr(lib, "sr_all_hits_rays") and hasattr(lib, "sr_all_hits_rays_device")
    assert callable(sa.GpuScene.all_hits) and callable(sa.GpuScene.all_hits_device)
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "void AllHitRays(int64_t n, const double* starts, const double* dirs, const double* limits, int32_t max_hits, uint32_t* count" in hpp
    assert "sr_all_hits_rays(" in hpp
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    assert "public RayHitLists AllHitRays(" in cs and "public void AllHitRaysDevice(" in cs
    assert "sr_all_hits_rays(IntPtr scene, int target, long n," in cs and "sr_all_hits_rays_device(IntPtr scene, int target, long n," in cs
    for doc, word in (("README.md", "sr_all_hits_rays"), ("DESIGN.md", "5.31"), ("INTEGRATION.md", "sr_all_hits_rays"),
                      (os.path.join("scripts", "README.md"), "gpu_all_hits.py")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc


def test_the_call_refuses_what_needs_no_device():
    """The refusals that come before the device is looked at, in the header's order, on a host-only scene and without one."""
    import ctypes as C

    import numpy as np

    import softray_amd as sa
    from helpers import unit_cube_scene
    L = sa._lib
    s = np.zeros((2, 3)); d = np.ones((2, 3))
    cnt = np.full(2, 7, dtype=np.uint32); idx = np.full((2, 4), 7, dtype=np.int32); rf = np.full((2, 4), 7.0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                                  # noqa: E731
    lib = L.lib()

    def call(h, target, n, a, b, k, options):
        rc = lib.sr_all_hits_rays(h, target, n, p(a), p(b), None, k, p(cnt), p(idx), p(rf), options, None)
        return rc, (lib.sr_last_error().decode() if rc else "")

    bare = sa.GpuScene(-1)                                                    # host-only, no model
    host = sa.GpuScene(-1)                                                    # host-only, a model and its reference tree
    host.set_triangles(*unit_cube_scene(100))
    host.build((sa.MODE_REF_TREE,))
    vox, bvh, tree, brute = L.TARGET_VOXELS, sa.MODE_BVH, sa.MODE_REF_TREE, sa.MODE_BRUTE
    options_text = "sr_all_hits_rays: unknown option bits (SR_RAYS_COHERENT and SR_RAYS_ENDPOINTS are the options)"
    k_text = "sr_all_hits_rays: max_hits must be 0 .. SR_HITS_MAX (64)"
    # every row breaks the rule it names and every later one it can: the earliest refusal is the one reported
    table = [
        ((None, vox, -1, None, None, 65, 4), L.SR_ERR_INVALID_ARG, "sr_all_hits_rays: the scene is NULL"),
        ((bare._h, vox, -1, None, None, 65, 4), L.SR_ERR_INVALID_ARG, "sr_all_hits_rays: n is negative"),
        ((bare._h, vox, 2, None, d, 65, 4), L.SR_ERR_INVALID_ARG, "sr_all_hits_rays: starts and dirs must not be NULL when n > 0"),
        ((bare._h, vox, 2, s, None, 65, 4), L.SR_ERR_INVALID_ARG, "sr_all_hits_rays: starts and dirs must not be NULL when n > 0"),
        ((bare._h, vox, 2, s, d, 65, 4), L.SR_ERR_INVALID_ARG, k_text),
        ((bare._h, vox, 2, s, d, -1, 4), L.SR_ERR_INVALID_ARG, k_text),
        ((bare._h, vox, 2, s, d, 4, 4), L.SR_ERR_INVALID_ARG, options_text),
        ((bare._h, vox, 0, None, None, 4, 1 << 31), L.SR_ERR_INVALID_ARG, options_text),
        ((bare._h, vox | tree, 2, s, d, 4, 3), L.SR_ERR_UNSUPPORTED,
         "sr_all_hits_rays: the voxel grid (SR_TARGET_VOXELS) has no tree to walk and its hits have rayFrac 0; use sr_trace_rays"),
        ((bare._h, tree, 2, s, d, 4, 0), L.SR_ERR_UNSUPPORTED, None),
        ((bare._h, tree | L.TARGET_ROOT, 0, None, None, 0, 0), L.SR_ERR_UNSUPPORTED, None),
        ((bare._h, bvh, 2, s, d, 4, 0), L.SR_ERR_NO_MODEL, "sr_all_hits_rays: the scene has no model (sr_set_triangles, sr_load_3ds)"),
        ((host._h, bvh, 2, s, d, 4, 0), L.SR_ERR_NOT_BUILT, "SR_MODE_BVH needs sr_build(1 << SR_MODE_BVH)"),
        ((host._h, brute, 2, s, d, 4, 0), L.SR_ERR_NO_DEVICE,
         "sr_all_hits_rays: a host-only scene has no HIP device to walk on (compute is never emulated on the CPU)"),
        ((host._h, brute, 0, None, None, 0, 0), L.SR_ERR_NO_DEVICE,
         "sr_all_hits_rays: a host-only scene has no HIP device to walk on (compute is never emulated on the CPU)"),
    ]
    for args, code, message in table:
        rc, text = call(*args)
        assert rc == code, (args[1:], text)
        if message is None:                                                   # the reference tree: the message says why
            assert text.startswith("sr_all_hits_rays: SR_MODE_REF_TREE has no notion of all hits") and "first leaf" in text and "several leaves" in text
        else:
            assert text == message
        assert np.all(cnt == 7) and np.all(idx == 7) and np.all(rf == 7.0)
    with pytest.raises(sa.SoftrayError):
        host.all_hits(brute, s, d)


def test_cpp_mirror_all_hits_program_builds(tmp_path):
    """The program compiles against Engine3D.hpp and links against the ABI; without a GPU it fails loudly instead of computing anything."""
    import torch
    exe = build_program(tmp_path)
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 3 and "no HIP device" in r.stderr


@pytest.mark.gpu
def test_cpp_mirror_all_hits(tmp_path):
    exe = build_program(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL OK" in r.stdout
    assert r.stdout.count("  ok") == 15 and "FAILED" not in r.stdout
