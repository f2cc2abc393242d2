"""The CPU model of voxel-grid rendering (tests/voxel_model.py) against the reference's own goldens, before it judges the GPU path
(tests/test_gpu_voxels.py): RaytraceVoxelGrid and RaytraceVoxelGridWithOtherObject (RendererTests.cs:285-306), 0 differing pixels each.
Then the library's host voxeliser (a host-only scene, no GPU) against the model's grid, and the source-level checks that the flag exists
on every layer."""
import os
import re

import numpy as np
import pytest

import voxel_model as vm
from helpers import GOLDEN, ROOT, load_obj3ds, make_frame, read_bmp_rgb, unit_cube_scene


def voxel_frame(res=100, **kw):
    f = make_frame(res, **kw)
    f.flags |= vm.F_VOXELS
    return f


@pytest.mark.parametrize("name,model,kw", vm.GOLDENS, ids=[g[0] for g in vm.GOLDENS])
def test_model_reproduces_the_voxel_goldens(name, model, kw):
    gold = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))
    v9, argb, _, _ = load_obj3ds(model)
    colors, normals, stats = vm.voxelise(v9, argb)
    got = vm.render((colors, normals), voxel_frame(**kw))
    assert got.shape == gold.shape and np.all(got >> 24 == 0xFF)
    assert int(np.count_nonzero((got & 0xFFFFFF) != gold)) == 0
    assert int(np.count_nonzero(gold != 0xff00ff)) >= 2000           # the golden shows the model
    assert stats["filled"] > 10000 and stats["pairs"] >= stats["filled"]


def host_grid(v9, argb, bmin, bmax):
    import softray_amd as sa
    s = sa.GpuScene(device=-1)
    try:
        s.set_triangles(v9, argb, bmin, bmax)
        s.build_voxels()
        s.build_voxels()                                              # idempotent
        return s.get_voxels()
    finally:
        s.close()


def assert_same_grid(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ": colours differ in %d cells" % int(np.count_nonzero(got[0] != want[0]))
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), what + ": normals differ"


@pytest.mark.parametrize("model", ["obj.3ds", "obj2.3DS"])
def test_host_voxeliser_equals_the_model_for_the_reference_models(model):
    v9, argb, bmin, bmax = load_obj3ds(model)
    want = vm.voxelise(v9, argb)
    assert_same_grid(host_grid(v9, argb, bmin, bmax), want, model)
    assert int(np.count_nonzero(want[0])) == want[2]["filled"] > 10000


def test_host_voxeliser_equals_the_model_for_the_unit_cube_scene():
    v9, argb, bmin, bmax = unit_cube_scene(20000)
    want = vm.voxelise(v9, argb)
    assert_same_grid(host_grid(v9, argb, bmin, bmax), want, "unit_cube_scene(20000)")
    assert want[2]["filled"] > 100000 and want[2]["max_per_cell"] > 3     # many cells sum several triangles


def test_grid_is_dropped_with_the_model_and_needs_one():
    import softray_amd as sa
    s = sa.GpuScene(device=-1)
    try:
        with pytest.raises(sa.SoftrayError) as e:
            s.build_voxels()
        assert e.value.code == sa._lib.SR_ERR_NO_MODEL
        v9, argb, bmin, bmax = unit_cube_scene(50)
        s.set_triangles(v9, argb, bmin, bmax)
        with pytest.raises(sa.SoftrayError) as e:
            s.get_voxels()
        assert e.value.code == sa._lib.SR_ERR_NOT_BUILT
        s.build_voxels()
        a = s.get_voxels()
        s.set_triangles(v9[:25], argb[:25], bmin, bmax)                # a new model drops the grid
        with pytest.raises(sa.SoftrayError):
            s.get_voxels()
        s.build_voxels()
        b = s.get_voxels()
        assert_same_grid(b, vm.voxelise(v9[:25], argb[:25]), "second model")
        assert not np.array_equal(a[0], b[0])
    finally:
        s.close()


def test_accumulated_steps_are_part_of_the_result():
    """`pos += delta` step by step is reproduced as it is: on the golden frame's own rays `start + k * delta` rounds to other cells for
    some steps, and the walks are long (hundreds of steps), so the difference is not hypothetical."""
    v9, argb, _, _ = load_obj3ds("obj.3ds")
    colors, normals, _ = vm.voxelise(v9, argb)
    from pathtrace_model import camera_samples
    starts, dirs = camera_samples(voxel_frame(depth=4.0))
    r = vm.walk(colors, normals, starts, dirs, return_steps=True)
    live = r["steps"] > 0
    assert int(r["hit"].sum()) >= 2000 and r["steps"].max() > 300 and r["steps"][live].mean() > 100
    ok, s, e = vm._clip(starts, starts + dirs * 10)
    s, e = (s[ok] * 0.5 + 0.5) * 63.999, (e[ok] * 0.5 + 0.5) * 63.999
    delta = e - s
    delta = delta * (0.1 / np.abs(delta).max(axis=1))[:, None]
    acc = s.copy()
    differ = 0
    for k in range(1, 200):
        acc = acc + delta
        differ += int(np.count_nonzero((acc.astype(np.int64) != (s + k * delta).astype(np.int64)).any(axis=1)))
    assert differ > 0


def test_flag_is_declared_on_every_layer():
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    m = re.search(r"\bSR_F_VOXELS\s*=\s*1u\s*<<\s*(\d+)", header)
    assert m, "include/softray.h does not declare SR_F_VOXELS"
    bit = int(m.group(1))
    others = {int(b) for n, b in re.findall(r"\b(SR_F_[A-Z_]+)\s*=\s*1u\s*<<\s*(\d+)", header) if n != "SR_F_VOXELS"}
    assert bit not in others and bit < 16
    assert "#define SR_ABI_VERSION 5" in header
    for sym in ("sr_build_voxels", "sr_get_voxels", "SR_TARGET_VOXELS"):
        assert sym in header, sym
    import softray_amd as sa
    assert sa._lib.F_VOXELS == 1 << bit == vm.F_VOXELS and sa.F_VOXELS == sa._lib.F_VOXELS
    assert sa.TARGET_VOXELS == vm.TARGET_VOXELS == int(re.search(r"#define SR_TARGET_VOXELS (0x[0-9a-fA-F]+)", header).group(1), 16)
    for rel in (("softray_amd", "host", "Engine3D.hpp"), ("bindings", "csharp", "GpuRenderer.cs")):
        assert "SR_F_VOXELS" in open(os.path.join(ROOT, *rel)).read(), rel
    # the Python mirror keeps refusing the switch (tests/test_pathtrace_model.py pins its list)
    src = open(os.path.join(ROOT, "softray_amd", "renderer.py")).read()
    refused = re.search(r"for name in \(([^)]*)\):\s*\n\s*if getattr\(self, name\):\s*\n\s*raise NotImplementedError", src)
    assert refused and "rayTraceVoxels" in refused.group(1)


def test_cpp_mirror_voxel_program_builds(tmp_path):
    """tests/cpp/voxel_tests.cpp compiles against Engine3D.hpp (rayTraceVoxels is a field the mirror passes on); without a GPU the
    program fails loudly instead of computing anything."""
    import subprocess
    import torch
    exe = str(tmp_path / "voxel_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "voxel_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    if not torch.cuda.is_available():
        r = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
        assert r.returncode == 3 and "no HIP device" in r.stderr
