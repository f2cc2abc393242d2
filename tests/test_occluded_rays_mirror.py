"""sr_occluded_rays above the C ABI: the call is declared on every layer, and the C++ mirror's Renderer::OccludedRays() (softray_amd/host/
Engine3D.hpp) is driven by tests/cpp/occluded_rays_tests.cpp, a program that links against the ABI and knows every answer it asks for."""
import os
import re
import subprocess

import pytest

from helpers import ROOT


def build_program(tmp_path):
    exe = str(tmp_path / "occluded_rays_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "occluded_rays_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    return exe


def test_the_call_is_declared_on_every_layer():
    import softray_amd as sa
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert re.search(r"int\s+sr_occluded_rays\(sr_scene\*, int32_t target, int64_t n, const double\* starts, const double\* dirs,", header)
    assert re.search(r"int\s+sr_occluded_rays_device\(sr_scene\*, int32_t target, int64_t n, const double\* d_starts, const double\* d_dirs,", header)
    assert "#define SR_RAYS_ENDPOINTS 2u" in header and "#define SR_RAYS_COHERENT 1u" in header and "#define SR_ABI_VERSION 5" in header
    assert "sr_occluded_rays" in sa._lib.SYMBOLS and "sr_occluded_rays_device" in sa._lib.SYMBOLS
    assert sa._lib.RAYS_ENDPOINTS == 2 and sa._lib.RAYS_COHERENT == 1
    lib = sa._lib.lib()
    assert hasattr(lib, "sr_occluded_rays") and hasattr(lib, "sr_occluded_rays_device")
    assert callable(sa.GpuScene.occluded) and callable(sa.GpuScene.occluded_device)
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "void OccludedRays(int64_t n, const double* starts, const double* dirs, const double* limits, uint8_t* occluded" in hpp and "sr_occluded_rays(" in hpp
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    assert "public byte[] OccludedRays(" in cs and "public void OccludedRaysDevice(" in cs
    assert "sr_occluded_rays(IntPtr scene, int target, long n," in cs and "sr_occluded_rays_device(IntPtr scene, int target, long n," in cs


def test_the_call_refuses_what_needs_no_device():
    """The refusals that come before the device is looked at, on a host-only scene and without one."""
    import ctypes as C

    import numpy as np

    import softray_amd as sa
    L = sa._lib
    s = np.zeros((2, 3)); d = np.ones((2, 3)); out = np.full(2, 7, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                  # noqa: E731
    lib = L.lib()
    assert lib.sr_occluded_rays(None, 0, 2, p(s), p(d), None, p(out), 0, None) == L.SR_ERR_INVALID_ARG
    assert lib.sr_last_error().decode() == "sr_occluded_rays: the scene is NULL"
    g = sa.GpuScene(-1)
    for args, code in (((-1, p(s), p(d), None, p(out), 0), L.SR_ERR_INVALID_ARG), ((2, None, p(d), None, p(out), 0), L.SR_ERR_INVALID_ARG),
                       ((2, p(s), p(d), None, p(out), 4), L.SR_ERR_INVALID_ARG), ((2, p(s), p(d), None, p(out), 0), L.SR_ERR_NO_MODEL)):
        assert lib.sr_occluded_rays(g._h, L.MODE_REF_TREE, *args, None) == code
    assert lib.sr_occluded_rays(g._h, L.TARGET_VOXELS, 2, p(s), p(d), None, p(out), 0, None) == L.SR_ERR_UNSUPPORTED
    assert "rayFrac 0" in lib.sr_last_error().decode()
    assert np.all(out == 7)


def test_cpp_mirror_occluded_rays_program_builds(tmp_path):
    """The program compiles against Engine3D.hpp and links against the ABI; without a GPU it fails loudly instead of computing anything."""
    import torch
    exe = build_program(tmp_path)
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 3 and "no HIP device" in r.stderr


@pytest.mark.gpu
def test_cpp_mirror_occluded_rays(tmp_path):
    exe = build_program(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL OK" in r.stdout
    assert r.stdout.count("  ok") == 9 and "FAILED" not in r.stdout
