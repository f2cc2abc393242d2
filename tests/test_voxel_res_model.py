"""Voxel grids of any resolution (sr_set_voxel_res, 1..256) on the CPU: the size-parameterised model (tests/voxel_model_n.py) against
tests/voxel_model.py at 64 and against the reference's own two voxel unit tests at 32 (TriangleTests.cs:368-393, :396-452); the library's
host voxeliser (a host-only scene) against the model for every size class, including triangles whose vertices lie on the planes
k / N - 0.5 to the last bit; the device voxeliser's cell-range arithmetic (axis_cells of sr_voxels.hip, compiled for the host) against a
test of all N cells; and the bookkeeping of the two new calls.  Every comparison is an exact equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import voxel_model as vm
import voxel_model_n as vn
from helpers import ROOT, load_obj3ds, make_frame

SIZES = [1, 2, 5, 32, 63, 65, 98, 256]


def voxel_frame(res=100, **kw):
    f = make_frame(res, **kw)
    f.flags |= vn.F_VOXELS
    return f


def assert_same_grid(got, want, what):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    assert np.array_equal(got[0], want[0]), "%s: colours differ in %d cells" % (what, int(np.count_nonzero(got[0] != want[0])))
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), what + ": normals differ"


def host_grid(v9, argb, n, bmin=None, bmax=None):
    import softray_amd as sa
    s = sa.GpuScene(device=-1)
    try:
        s.set_triangles(v9, argb, np.array([-0.5] * 3) if bmin is None else bmin, np.array([0.5] * 3) if bmax is None else bmax)
        s.voxel_res = n
        assert s.voxel_res == n
        s.build_voxels()
        return s.get_voxels()
    finally:
        s.close()


# ---- the model ----
@pytest.mark.parametrize("name,model,kw", vm.GOLDENS, ids=[g[0] for g in vm.GOLDENS])
def test_model_at_64_is_voxel_model(name, model, kw):
    v9, argb, _, _ = load_obj3ds(model)
    old, new = vm.voxelise(v9, argb), vn.voxelise(v9, argb, 64)
    assert_same_grid(new, old, model)
    assert new[2] == old[2]
    f = voxel_frame(**kw)
    a, b = vm.render(old[:2], f), vn.render(new[:2], f)
    assert np.array_equal(a, b) and int(np.count_nonzero(a != 0xFFFF00FF)) >= 2000


def test_reference_kat_one_triangle_fills_32_by_32_cells():
    """TriangleTests.cs:368-393: the triangle at z = 0.001 in a 32^3 grid."""
    colors, normals, stats = vn.voxelise(vn.KAT_TRIANGLE, vn.KAT_COLOR, 32)
    assert stats["filled"] == 32 * 32 and stats["pairs"] == 32 * 32
    x, y, z = np.nonzero(colors)
    assert np.all(z == 16) and len(set(zip(x.tolist(), y.tolist()))) == 1024
    assert np.all(colors[:, :, 16] == vn.KAT_COLOR[0])
    assert_same_grid(host_grid(vn.KAT_TRIANGLE, vn.KAT_COLOR, 32), (colors, normals), "KAT")


def test_reference_random_triangles_fill_the_32_grid():
    """TriangleTests.cs:396-452: 1000 triangles with vertices uniform in [-0.5, 0.5]^3 fill more than 99 % of 32^3 cells."""
    rng = np.random.default_rng(12345)
    v9 = rng.uniform(-0.5, 0.5, (1000, 3, 3))
    argb = (rng.integers(0, 1 << 24, 1000).astype(np.uint32) | np.uint32(0xFF000000))
    colors, _, stats = vn.voxelise(v9, argb, 32)
    assert stats["filled"] > 0.99 * 32 ** 3 and int(np.count_nonzero(colors)) == stats["filled"]


# ---- the host voxeliser (sr_host.cpp voxelise_host) ----
@pytest.mark.parametrize("n", SIZES)
def test_host_grid_equals_the_model(n):
    v9, argb, bmin, bmax = load_obj3ds("obj.3ds")
    want = vn.voxelise(v9, argb, n)
    assert want[2]["filled"] >= 1
    assert_same_grid(host_grid(v9, argb, n, bmin, bmax), want, "obj.3ds at %d" % n)


@pytest.mark.parametrize("n", [5, 98])
def test_host_grid_of_triangles_on_the_planes(n):
    v9, argb = vn.boundary_triangles(n)
    planes = vn.planes_of(n)
    flat = v9.reshape(-1)
    on = np.isin(flat, planes).sum()
    near = (np.isin(np.nextafter(flat, np.inf), planes) | np.isin(np.nextafter(flat, -np.inf), planes)).sum()
    assert on > 300 and near > 600                                    # the scene is what it says
    want = vn.voxelise(v9, argb, n)
    assert_same_grid(host_grid(v9, argb, n), want, "boundary triangles at %d" % n)


# ---- axis_cells of the device voxeliser, compiled for the host ----
def build_axis_cells(tmp_path):
    src = open(os.path.join(ROOT, "softray_amd", "csrc", "sr_voxels.hip")).read()
    m = re.search(r"(__device__ __forceinline__ double cell_plane\(.*?\n}\n)\s*\nstruct CellBox", src, flags=re.S)
    assert m and "void axis_cells(double mn, double mx, int n, int& lo, int& hi)" in m.group(1)
    code = ("#include <math.h>\n#define __device__\n#define __forceinline__ inline\n" + m.group(1) +
            "extern \"C\" void axis_cells_batch(const double* mn, const double* mx, long long count, int n, int* lo, int* hi) {\n"
            "    for (long long i = 0; i < count; ++i) axis_cells(mn[i], mx[i], n, lo[i], hi[i]);\n}\n")
    cpp, so = str(tmp_path / "axis_cells.cpp"), str(tmp_path / "axis_cells.so")
    open(cpp, "w").write(code)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, cpp])
    lib = C.CDLL(so)
    lib.axis_cells_batch.restype = None
    lib.axis_cells_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def axis_ranges(n, rng):
    planes = vn.planes_of(n)
    near = np.concatenate([planes, np.nextafter(planes, np.inf), np.nextafter(planes, -np.inf)])
    a = rng.uniform(-0.75, 0.75, 60000)
    b = a + rng.uniform(0.0, 1.0, 60000) ** 4                         # mostly short ranges, some across the grid
    c = rng.choice(near, 30000)
    d = rng.choice(near, 30000)
    e = rng.uniform(-0.75, 0.75, 15000)
    f = rng.choice(near, 15000)
    g = rng.uniform(-0.9, -0.5, 500)                                  # across the whole grid
    mn = np.concatenate([a, np.minimum(c, d), np.minimum(e, f), near, near, g])
    mx = np.concatenate([b, np.maximum(c, d), np.maximum(e, f), near, np.full(near.size, 0.75), -g])
    return np.ascontiguousarray(mn), np.ascontiguousarray(mx)


@pytest.mark.parametrize("n", [5, 98, 255, 256])
def test_axis_cells_equals_a_test_of_all_cells(n, tmp_path):
    lib = build_axis_cells(tmp_path)
    mn, mx = axis_ranges(n, np.random.default_rng(99 + n))
    assert mn.size >= 100000
    lo = np.zeros(mn.size, dtype=np.int32)
    hi = np.zeros(mn.size, dtype=np.int32)
    lib.axis_cells_batch(mn.ctypes.data, mx.ctypes.data, mn.size, n, lo.ctypes.data, hi.ctypes.data)
    planes = vn.planes_of(n)
    want_lo = np.zeros(mn.size, dtype=np.int64)
    want_cnt = np.zeros(mn.size, dtype=np.int64)
    for i in range(0, mn.size, 20000):                                # max >= plane(k) and min <= plane(k + 1), every k, no epsilon
        inside = (mx[i:i + 20000, None] >= planes[None, :n]) & (mn[i:i + 20000, None] <= planes[None, 1:])
        want_lo[i:i + 20000] = inside.argmax(axis=1)
        want_cnt[i:i + 20000] = inside.sum(axis=1)
    got_cnt = np.maximum(0, hi.astype(np.int64) - lo + 1)
    assert np.array_equal(got_cnt, want_cnt), "cell counts differ for %d ranges" % int(np.count_nonzero(got_cnt != want_cnt))
    some = want_cnt > 0
    assert np.array_equal(lo[some], want_lo[some])
    assert int(np.count_nonzero(~some)) > 1000 and int(np.count_nonzero(want_cnt == n)) > 100     # ranges beside the grid, ranges across it


# ---- the two calls ----
def test_voxel_res_bookkeeping():
    import softray_amd as sa
    s = sa.GpuScene(device=-1)
    try:
        assert s.voxel_res == 64                                      # Renderer.cs:1570
        for bad in (0, -1, 257):
            with pytest.raises(sa.SoftrayError) as e:
                s.voxel_res = bad
            assert e.value.code == sa._lib.SR_ERR_INVALID_ARG and "1..256" in str(e.value)
            assert s.voxel_res == 64
        s.set_triangles(vn.KAT_TRIANGLE, vn.KAT_COLOR, np.array([-0.5] * 3), np.array([0.5] * 3))
        s.build_voxels()
        a = s.get_voxels()
        assert a[0].shape == (64, 64, 64) and a[1].shape == (64, 64, 64, 3)
        s.voxel_res = 64                                              # the same value keeps the grid
        assert_same_grid(s.get_voxels(), a, "kept")
        s.voxel_res = 32                                              # another one drops it
        with pytest.raises(sa.SoftrayError) as e:
            s.get_voxels()
        assert e.value.code == sa._lib.SR_ERR_NOT_BUILT
        s.build_voxels()
        b = s.get_voxels()
        assert b[0].shape == (32, 32, 32) and int(np.count_nonzero(b[0])) == 1024
        s.voxel_res = 32
        assert_same_grid(s.get_voxels(), b, "kept")
        s.voxel_res = 256
        assert s.voxel_res == 256
        s.voxel_res = 1
        s.build_voxels()
        assert s.get_voxels()[0].shape == (1, 1, 1)
    finally:
        s.close()


def test_the_calls_are_declared_on_every_layer():
    import softray_amd as sa
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert re.search(r"int\s+sr_set_voxel_res\(sr_scene\*, int32_t n\);", header) and re.search(r"int32_t\s+sr_get_voxel_res\(const sr_scene\*\);", header)
    assert "#define SR_ABI_VERSION 5" in header and "sr_get_voxel_res" in header.split("sr_get_voxels(sr_scene*")[0][-600:]
    assert "sr_set_voxel_res" in sa._lib.SYMBOLS and "sr_get_voxel_res" in sa._lib.SYMBOLS
    L = sa._lib.lib()
    assert hasattr(L, "sr_set_voxel_res") and hasattr(L, "sr_get_voxel_res")
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "int VoxelGridSize() const" in hpp and "void VoxelGridSize(int n)" in hpp and "sr_set_voxel_res" in hpp
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    assert "public int VoxelResolution" in cs and "sr_set_voxel_res(IntPtr scene, int n)" in cs and "sr_get_voxel_res(IntPtr scene)" in cs
    # the Python mirror keeps refusing the switch
    src = open(os.path.join(ROOT, "softray_amd", "renderer.py")).read()
    refused = re.search(r"for name in \(([^)]*)\):\s*\n\s*if getattr\(self, name\):\s*\n\s*raise NotImplementedError", src)
    assert refused and "rayTraceVoxels" in refused.group(1)


def test_cpp_mirror_voxel_res_program_builds(tmp_path):
    """tests/cpp/voxel_res_tests.cpp compiles against Engine3D.hpp (VoxelGridSize getter and setter); without a GPU the program fails
    loudly instead of computing anything."""
    import torch
    from helpers import GOLDEN
    exe = str(tmp_path / "voxel_res_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "voxel_res_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    if not torch.cuda.is_available():
        r = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
        assert r.returncode == 3 and "no HIP device" in r.stderr
