"""sr_ao_points without a GPU: System.Random's jump-ahead against the generator itself, the points model (tests/ao_points_model.py)
pinned to the frame model the AO frames are held to (tests/ao_model.py), every refusal on a host-only scene in the header's order, and
the symbols on every layer.  Every comparison is an exact equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ao_model as aom
import ao_points_model as apm
import pathtrace_model as ptm
import softray_amd as sa
from helpers import ROOT, load_obj3ds, make_frame, orc, unit_cube_scene

L = sa._lib
INT_MIN = -2 ** 31
SEEDS = [1234567890, 0, 1, -1, INT_MIN, 161803398, 161803399]


# ---- 1. the jump-ahead ----
def sequential(seed, skip):
    return np.round(sa.net_random_doubles(seed, 55, skip=skip) * 2147483647).astype(np.int64)


@pytest.mark.parametrize("seed", SEEDS)
def test_jump_equals_the_sequence(seed):
    for skip in (0, 1, 33, 34, 54, 55, 56, 299, 300, 19200, 300 * 2 ** 17):
        assert np.array_equal(sa.net_random_jump(seed, skip).astype(np.int64), sequential(seed, skip)), skip


def test_jump_over_1e8_draws():
    assert np.array_equal(sa.net_random_jump(1234567890, 10 ** 8).astype(np.int64), sequential(1234567890, 10 ** 8))


@pytest.mark.parametrize("seed", SEEDS)
def test_jump_beyond_what_can_be_drawn(seed):
    skip = 2 ** 40 - 55
    a, b, d = (sa.net_random_jump(seed, s).astype(np.int64) for s in (skip, skip + 1, skip + 55))
    assert np.array_equal(a[1:], b[:54])
    assert np.array_equal((a[:34] - a[21:55]) % 2147483647, d[:34])          # s[n + 55] = s[n] - s[n + 21] mod 2^31 - 1
    assert np.array_equal((a[34:] - d[:21]) % 2147483647, d[34:])            # ... where s[n + 21] is of the next window
    assert a.min() >= 0 and a.max() <= 2147483646


def test_jump_host_code_under_sanitizers(tmp_path):
    """tests/cpp/net_jump_tests.cpp: a stand-alone program of the jump's host code (sr_host.cpp) and NetRandom, built with the address and
    undefined-behaviour sanitizers."""
    exe = str(tmp_path / "net_jump_tests")
    csrc = os.path.join(ROOT, "softray_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "net_jump_tests.cpp"),
                           os.path.join(csrc, "sr_host.cpp"), "-pthread"])
    r = subprocess.run([exe, "20000"], capture_output=True, text=True)              # (the longer skips: the tests above)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr


# ---- 2. the points model is the frame model with the frame taken away ----
@pytest.fixture(scope="module")
def cube():
    o = orc.Scene()
    o.set_triangles(*unit_cube_scene(2000))
    assert o.build_tree() == 0
    return o


def frame_hits(o, f):
    s, d = ptm.camera_samples(f)
    first = o.trace(aom.TRACE_ROOT_TREE, s, d)
    hit = first["hit"].astype(bool)
    return hit, first["pos"][hit], first["normal"][hit], first["color"][hit]


def test_points_model_equals_the_frame_model_cached(cube):
    f = aom.ao_frame(make_frame(40, 32, shading=False, concurrency=1))
    hit, pos, nrm, col = frame_hits(cube, f)
    assert hit.sum() > 300
    frame_model = aom.AoModel()
    cache = np.zeros(aom.RES ** 3, dtype=np.uint8)
    for warm in (False, True):
        want = frame_model.sample_colors(cube, f)
        amount, out, gens = apm.ao_points(cube, aom.TRACE_ROOT_TREE, pos, nrm, f.random_seed, cache, color=col)
        assert gens == frame_model.generators and (gens == 0) == warm
        assert np.array_equal(out, want[hit]) and np.array_equal(cache, frame_model.cache)
        assert np.array_equal(amount, cache[aom.cells(aom.clamp_pos(pos))])


def test_points_model_equals_the_frame_model_uncached(cube):
    f = aom.ao_frame(make_frame(40, 32, shading=False, concurrency=1), uncached=True)
    hit, pos, nrm, col = frame_hits(cube, f)
    cache = np.zeros(aom.RES ** 3, dtype=np.uint8)
    want = aom.AoModel().sample_colors(cube, f)
    amount, out, gens = apm.ao_points(cube, aom.TRACE_ROOT_TREE, pos, nrm, f.random_seed, cache, uncached=True, color=col)
    assert gens == int(hit.sum()) and np.array_equal(out, want[hit]) and not cache.any()
    # a split batch continues the sequence: first_generator = the generators before it
    h = gens // 3
    a2, o2, g2 = apm.ao_points(cube, aom.TRACE_ROOT_TREE, pos[h:], nrm[h:], f.random_seed, cache, uncached=True, color=col[h:], first_generator=h)
    assert g2 == gens - h and np.array_equal(a2, amount[h:]) and np.array_equal(o2, out[h:])


def test_points_model_clamps_nan_positions_to_the_upper_face():
    p = np.array([[np.nan, 0.0, -7.0], [0.25, np.nan, np.nan]])
    assert np.array_equal(apm.clamp_pos(p), np.array([[0.5, 0.0, -0.5], [0.25, 0.5, 0.5]]))


# ---- 3. validation on a host-only scene, in the header's order ----
def call(s, f, n=4, pos=True, nrm=True, out=True, amount=True, first=0, options=0, device=False):
    p = np.zeros((max(n, 1), 3))
    o = np.zeros(max(n, 1), dtype=np.uint32)
    a = np.zeros(max(n, 1), dtype=np.uint8)
    made = C.c_uint64(77)
    vp = lambda x, on: x.ctypes.data_as(C.c_void_p) if on else None
    fr = C.byref(f) if f is not None else None
    if device:
        rc = L.lib().sr_ao_points_device(s, fr, n, vp(p, pos), vp(p, nrm), None, vp(o, out), vp(a, amount), first, options, None, None, None)
    else:
        rc = L.lib().sr_ao_points(s, fr, n, vp(p, pos), vp(p, nrm), None, vp(o, out), vp(a, amount), first, options, C.byref(made))
    return rc, made.value


@pytest.mark.parametrize("device", [False, True], ids=["host_variant", "device_variant"])
def test_refusals_in_order_on_a_host_only_scene(device):
    s = sa.GpuScene(-1)
    s.set_triangles(*load_obj3ds("obj2.3DS"))
    h = s._h
    good = sa.Frame.from_buffer_copy(bytes(make_frame(16)))

    def changed(**kw):
        f = sa.Frame.from_buffer_copy(bytes(good))
        f.flags |= kw.pop("flags", 0)
        for k, v in kw.items():
            setattr(f, k, v)
        return f
    # (the refused frame, the whole message of sr_last_error)
    unsupported = [(changed(flags=L.F_STATIC_SHADOWS),
                    "sr_ao_points: static shadows (SR_F_STATIC_SHADOWS) are another decorator's cache, not AmbientOcclusionMethod's step"),
                   (changed(flags=L.F_PATH_TRACING),
                    "sr_ao_points: path tracing (SR_F_PATH_TRACING) replaces the decorator chain AmbientOcclusionMethod is part of"),
                   (changed(flags=L.F_VOXELS), "sr_ao_points: voxel rendering (SR_F_VOXELS) has no occlusion step"),
                   (changed(flags=L.F_LIGHT_FIELD),
                    "sr_ao_points: the light field (SR_F_LIGHT_FIELD) stores colours of canonical rays, not of a caller's points"),
                   (changed(flags=L.F_SINGLE_KERNEL), "sr_ao_points: the one-kernel renderer (SR_F_SINGLE_KERNEL) has no stage to enter"),
                   (changed(max_bounces=1), "sr_ao_points: mirror bounces (max_bounces > 0) belong to a camera ray, not to a point"),
                   (changed(strip_rows=16, strip_count=2, strip_index=0),
                    "sr_ao_points: row strips (strip_count > 0) divide a frame's rows, not a batch of points")]
    # 1. SR_ERR_INVALID_ARG, whatever else is wrong with the frame (the model has no tree yet: SR_ERR_NOT_BUILT would come later)
    bad_frame = unsupported[0][0]
    for kw in (dict(n=-1), dict(pos=False), dict(nrm=False), dict(out=False, amount=False), dict(options=1), dict(options=0x80000000),
               dict(first=2 ** 40 - 3), dict(first=2 ** 40 + 1, n=0), dict(first=2 ** 64 - 1)):
        assert call(h, bad_frame, device=device, **kw)[0] == L.SR_ERR_INVALID_ARG, kw
        assert L.lib().sr_last_error().decode() == "bad argument to sr_ao_points", kw
    assert call(None, good, device=device)[0] == L.SR_ERR_INVALID_ARG
    assert call(h, None, device=device)[0] == L.SR_ERR_INVALID_ARG
    assert call(h, good, first=2 ** 40 - 4, device=device)[0] != L.SR_ERR_INVALID_ARG                    # first_generator + n == 2^40 is legal
    # 2. SR_ERR_UNSUPPORTED before the frame and its trace mode are validated (width 0 and no tree would be refused otherwise)
    for f, text in unsupported:
        f.width = 0
        rc, _ = call(h, f, device=device)
        assert rc == L.SR_ERR_UNSUPPORTED and L.lib().sr_last_error().decode() == text and text.startswith("sr_ao_points: ")
    # 3. sr_render's validation of the frame, then of its trace mode
    assert call(h, changed(width=0), device=device)[0] == L.SR_ERR_INVALID_ARG
    assert call(h, changed(sub_pixel_res=0), device=device)[0] == L.SR_ERR_INVALID_ARG
    assert call(h, good, device=device)[0] == L.SR_ERR_NOT_BUILT
    assert call(h, good, n=0, device=device)[0] == L.SR_ERR_NOT_BUILT                                    # n == 0 must pass these checks too
    s.build((sa.MODE_REF_TREE,))
    assert call(h, changed(trace_mode=sa.MODE_BVH), device=device)[0] == L.SR_ERR_NOT_BUILT
    assert call(h, changed(trace_mode=7), device=device)[0] == L.SR_ERR_INVALID_ARG
    # 4. the device comes last; one output is enough; SR_F_AMBIENT_OCCLUSION and SR_F_AO_UNCACHED are accepted
    for kw in (dict(), dict(out=False), dict(amount=False)):
        assert call(h, good, device=device, **kw)[0] == L.SR_ERR_NO_DEVICE
    assert call(h, changed(flags=L.F_AMBIENT_OCCLUSION | L.F_AO_UNCACHED | L.F_SHADOWS), device=device)[0] == L.SR_ERR_NO_DEVICE
    # n == 0: SR_OK before a device is asked for, *generators = 0, both outputs may be NULL
    rc, made = call(h, good, n=0, out=False, amount=False, pos=False, nrm=False, device=device)
    assert rc == L.SR_OK and (device or made == 0)
    assert not s.get_ao_cache().any()


def test_python_wrapper_checks_shapes():
    s = sa.GpuScene(-1)
    s.set_triangles(*load_obj3ds("obj2.3DS"))
    s.build((sa.MODE_REF_TREE,))
    f = sa.Frame.from_buffer_copy(bytes(make_frame(16)))
    with pytest.raises(ValueError):
        s.ao_points(f, np.zeros((3, 3)), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        s.ao_points(f, np.zeros((3, 3)), np.zeros((3, 3)), color=np.zeros(2, dtype=np.uint32))
    with pytest.raises(sa.SoftrayError) as e:
        s.ao_points(f, np.zeros((3, 3)), np.zeros((3, 3)))
    assert e.value.code == L.SR_ERR_NO_DEVICE
    assert s.ao_points(f, np.zeros((0, 3)), np.zeros((0, 3)))[2] == 0


# ---- 4. the symbols on every layer ----
def test_symbols_on_every_layer():
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert "#define SR_ABI_VERSION 5" in header and L.lib().sr_abi_version() == 5
    for sym in ("sr_ao_points", "sr_ao_points_device", "sr_net_random_jump"):
        assert re.search(r"\bint\s+%s\(" % sym, header), sym
        assert sym in L.SYMBOLS and hasattr(L.lib(), sym)
    assert hasattr(sa.GpuScene, "ao_points") and hasattr(sa.GpuScene, "ao_points_device") and hasattr(sa, "net_random_jump")
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "AmbientOcclusionPoints(" in hpp and "sr_ao_points(" in hpp
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    for sym in ("sr_ao_points(", "sr_ao_points_device(", "sr_net_random_jump(", " AoPoints(", " AoPointsDevice("):
        assert sym in cs, sym
    kernels = open(os.path.join(ROOT, "softray_amd", "csrc", "sr_kernels.hip")).read()
    assert '"k_draws"' in kernels and '"k_aop_probe"' in kernels
    # the Python mirror keeps its refusal list (tests/test_pathtrace_model.py pins it)
    src = open(os.path.join(ROOT, "softray_amd", "renderer.py")).read()
    assert "ao_points" not in src
