"""sr_light_field_rays above the C ABI: the C++ mirror's Renderer::LightFieldRays() (softray_amd/host/Engine3D.hpp) is driven by
tests/cpp/lightfield_rays_tests.cpp, a program that links against the ABI and knows every answer it asks for.  (The declarations on every
layer: tests/test_lightfield_rays_model.py.)"""
import os
import subprocess

import pytest

from helpers import ROOT


def build_program(tmp_path):
    exe = str(tmp_path / "lightfield_rays_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "lightfield_rays_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    return exe


def test_cpp_mirror_light_field_rays_program_builds(tmp_path):
    """The program compiles against Engine3D.hpp and links against the ABI; without a GPU it fails loudly instead of computing anything."""
    import torch
    exe = build_program(tmp_path)
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 3 and "no HIP device" in r.stderr


@pytest.mark.gpu
def test_cpp_mirror_light_field_rays(tmp_path):
    exe = build_program(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL OK" in r.stdout
    assert r.stdout.count("  ok") == 8 and "FAILED" not in r.stdout
