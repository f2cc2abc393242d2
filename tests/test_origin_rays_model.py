"""Ray batches from one origin (sr_trace_origin_rays) without a GPU: the calls on every layer, the refusals in the documented order on a
host-only scene, and -- with the oracle -- what keeps the GPU tests (tests/test_gpu_origin_rays.py) from passing vacuously: between 10 % and
90 % of the regular rays of every case hit, the origins stand where their names say, the sets hold the directions their names promise."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gbuffer_cases as gbc
import origin_rays_cases as orc_cases
from helpers import ROOT, load_obj3ds


# ---- 1. the calls on every layer ----
def test_calls_are_declared_on_every_layer():
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert re.search(r"#define SR_RAYS_COHERENT 1u\b", header)
    assert re.search(r"\bint\s+sr_trace_origin_rays\(sr_scene\*, int32_t target, const double origin\[3\], int64_t n, const double\* dirs,", header)
    assert re.search(r"\bint\s+sr_trace_origin_rays_device\(sr_scene\*, int32_t target, const double origin\[3\] /\* HOST \*/, int64_t n, const double\* d_dirs,", header)
    assert "#define SR_ABI_VERSION 5" in header
    import softray_amd as sa
    assert sa._lib.lib().sr_abi_version() == 5 and sa._lib.RAYS_COHERENT == 1
    for sym in ("sr_trace_origin_rays", "sr_trace_origin_rays_device"):
        assert sym in sa._lib.SYMBOLS and hasattr(sa._lib.lib(), sym)
    for name in ("trace_origin", "trace_origin_device"):
        assert callable(getattr(sa.GpuScene, name, None)), name
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "void TraceOriginRays(const Vector& origin, int64_t n, const double* dirs," in hpp and "sr_trace_origin_rays(scene_, SR_TARGET_ROOT | Mode()," in hpp
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    assert "public FrameHits TraceOriginRays(" in cs and "public void TraceOriginRaysDevice(" in cs
    for sym in ("sr_trace_origin_rays(", "sr_trace_origin_rays_device("):
        assert "extern int " + sym in cs, sym
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "sr_trace_origin_rays" in open(os.path.join(ROOT, doc)).read(), doc
    kernels = open(os.path.join(ROOT, "softray_amd", "csrc", "sr_kernels.hip")).read()
    assert "case K_ORIGIN_RAYS:" in kernels and "case K_ORIGIN_SORT:" in kernels


# ---- 2. refusals, in order, before the device is looked at ----
def host_scene(build=True):
    import softray_amd as sa
    s = sa.GpuScene(-1)
    s.set_triangles(*load_obj3ds("obj2.3DS"))
    if build:
        s.build((sa.MODE_REF_TREE,))
    return s


GUARD = 0xA5
N = 16


def guarded():
    """Six output arrays for N rays, filled with a guard byte."""
    return [np.full(N * k, GUARD, dtype=np.uint8) for k in (1, 8, 24, 24, 4, 4)]


def raw_call(s, target, origin, n, dirs, arrays, options, device):
    import softray_amd as sa
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    h = None if s is None else s._h
    args = [p(a) for a in arrays]
    if device:
        return sa._lib.lib().sr_trace_origin_rays_device(h, target, p(origin), n, p(dirs), *args, options, None, None)
    return sa._lib.lib().sr_trace_origin_rays(h, target, p(origin), n, p(dirs), *args, options, None)


@pytest.mark.parametrize("device", [False, True], ids=["host_arrays", "device_arrays"])
def test_refusals_come_in_order_on_a_host_only_scene(device):
    import softray_amd as sa
    E = sa._lib
    s, unbuilt, empty = host_scene(), host_scene(build=False), sa.GpuScene(-1)
    arrays, none = guarded(), [None] * 6
    origin, dirs = np.array([0.3, 0.2, -2.0]), np.tile(np.array([0.0, 0.0, 1.0]), (N, 1))
    tree, bvh, voxels = sa.MODE_REF_TREE, sa.MODE_BVH, E.TARGET_VOXELS
    call = lambda sc, target=tree, o=origin, n=N, d=dirs, arr=arrays, opt=0: raw_call(sc, target, o, n, d, arr, opt, device)
    # (1) SR_ERR_INVALID_ARG: a NULL scene or origin, n < 0, NULL dirs with n > 0, unknown option bits, a non-finite origin -- each also on
    #     the voxel target, on a mode that is not built and on a scene without a model: those refusals come later
    for target, sc in ((tree, s), (voxels, s), (bvh, s), (tree, unbuilt), (tree, empty)):
        assert call(None, target) == E.SR_ERR_INVALID_ARG
        assert call(sc, target, o=None) == E.SR_ERR_INVALID_ARG
        assert call(sc, target, n=-1) == E.SR_ERR_INVALID_ARG
        assert call(sc, target, d=None) == E.SR_ERR_INVALID_ARG
        for opt in (2, 4, 1 << 31, 3):
            assert call(sc, target, opt=opt) == E.SR_ERR_INVALID_ARG, opt
        for k in range(3):
            for bad in (np.nan, np.inf, -np.inf):
                o = origin.copy()
                o[k] = bad
                assert call(sc, target, o=o) == E.SR_ERR_INVALID_ARG, (k, bad)
    # (2) SR_TARGET_VOXELS, by name -- before the model and the mode are looked at
    for sc in (s, unbuilt, empty):
        for opt in (0, E.RAYS_COHERENT):
            assert call(sc, voxels, opt=opt) == E.SR_ERR_UNSUPPORTED
            assert "SR_TARGET_VOXELS" in E.lib().sr_last_error().decode()
        assert call(sc, voxels, n=0, d=None, arr=none) == E.SR_ERR_UNSUPPORTED
    # (3) sr_trace_rays' own checks -- SR_ERR_NOT_BUILT comes before SR_ERR_NO_DEVICE
    assert call(empty) == E.SR_ERR_NO_MODEL and call(empty, n=0, d=None) == E.SR_ERR_NO_MODEL
    assert call(unbuilt) == E.SR_ERR_NOT_BUILT and call(unbuilt, E.TARGET_ROOT | tree) == E.SR_ERR_NOT_BUILT
    assert call(s, bvh) == E.SR_ERR_NOT_BUILT and call(s, E.TARGET_ROOT | bvh, opt=E.RAYS_COHERENT) == E.SR_ERR_NOT_BUILT
    assert call(s, bvh, n=0, d=None) == E.SR_ERR_NOT_BUILT
    assert call(s, 7) == E.SR_ERR_INVALID_ARG                       # (an unknown mode, as sr_trace_rays answers it)
    # n == 0 that passes (1)-(3) is SR_OK and touches nothing -- no device is asked for
    for target in (tree, sa.MODE_BRUTE, E.TARGET_ROOT | tree):
        for d in (dirs, None):
            for arr in (arrays, none):
                assert call(s, target, n=0, d=d, arr=arr, opt=E.RAYS_COHERENT) == 0
    # (4) a valid call lacks only a device: SR_ERR_NO_DEVICE last
    for target in (tree, sa.MODE_BRUTE, E.TARGET_ROOT | tree, E.TARGET_ROOT | sa.MODE_BRUTE):
        for opt in (0, E.RAYS_COHERENT):
            for arr in (arrays, none):
                assert call(s, target, arr=arr, opt=opt) == E.SR_ERR_NO_DEVICE
    far = np.array([1e300, -1e300, 1e-300])                          # any finite origin is legal
    assert call(s, o=far) == E.SR_ERR_NO_DEVICE
    for a in arrays:
        assert np.all(a == GUARD)
    assert s.trace_origin(tree, origin, np.zeros((0, 3)))["hit"].shape == (0,)
    with pytest.raises(sa.SoftrayError) as e:
        s.trace_origin(tree, origin, dirs, coherent=True, stats=True)
    assert e.value.code == E.SR_ERR_NO_DEVICE


# ---- 3. the cases of the GPU tests: checked here, on the CPU, not tuned on the GPU ----
@pytest.fixture(scope="module")
def oracles():
    return {name: gbc.oracle_scenes(name) for name in orc_cases.SCENES}


def test_origins_stand_where_their_names_say():
    for scene in orc_cases.SCENES:
        lo, hi = orc_cases.box(scene)
        ext = hi - lo
        margin = 0.01 + 1e-3 * ext                                  # the library's margin for "outside the slab" (point_outside_axes)
        outside = lambda o: [bool(o[a] > hi[a] + margin[a] or o[a] < lo[a] - margin[a]) for a in range(3)]
        assert outside(orc_cases.origin_of(scene, "out")) == [True] * 3
        assert sum(outside(orc_cases.origin_of(scene, "one"))) == 1
        assert np.array_equal(orc_cases.origin_of(scene, "centre"), 0.5 * (lo + hi))
        far = orc_cases.origin_of(scene, "far")
        assert outside(far) == [True] * 3 and np.allclose(np.abs(far - 0.5 * (lo + hi)) / ext, 2.5e5)
        # "plane": on the plane of a model triangle (to rounding), inside its outline, inside the box
        p = orc_cases.plane_point(scene)
        v9 = np.asarray(gbc.scene_data(scene)[0][0], dtype=np.float64).reshape(-1, 3, 3)
        best = None
        for t in v9:
            n = np.cross(t[1] - t[0], t[2] - t[0])
            if np.linalg.norm(n) == 0:
                continue
            d = abs(np.dot(n / np.linalg.norm(n), p - t[0]))
            if best is None or d < best[0]:
                best = (d, t, n)
        d, t, n = best
        assert d < 1e-15 * max(1.0, np.abs(t).max()) * 8
        bary = [np.dot(np.cross(t[(k + 1) % 3] - t[k], p - t[k]), n) for k in range(3)]
        assert min(bary) > 0.05 * np.dot(n, n)
        assert outside(p) == [False] * 3


def test_direction_sets_hold_what_their_names_promise():
    sph = orc_cases.sphere_dirs()
    assert sph.shape == (64 * 32, 3) and orc_cases.regular(sph).all()
    rows = {tuple(r) for r in sph.tolist()}
    for axis in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        assert any(np.array_equal(np.array(r), np.array(axis, dtype=np.float64)) for r in rows), axis
    zeros = sph[sph == 0.0]
    assert np.signbit(zeros).any() and (~np.signbit(zeros)).any()             # zero components of both signs
    for scene in orc_cases.SCENES:
        assert not orc_cases.facing(scene, "out", sph).all() and orc_cases.facing(scene, "out", sph).any()   # rays pointing away, and not
    order = orc_cases.tile_order()
    assert sorted(order.tolist()) == list(range(orc_cases.GRID_W * orc_cases.GRID_H)) and not np.array_equal(order, np.arange(order.size))
    first = order[:64].reshape(8, 8)
    assert np.array_equal(first, np.arange(8)[None, :] + orc_cases.GRID_W * np.arange(8)[:, None])
    for scene in orc_cases.SCENES:
        g = orc_cases.dirs_of(scene, "out", "grid")
        assert np.array_equal(orc_cases.dirs_of(scene, "out", "tiles"), g[order])
        for n in (1, 63, 64, 65, 64 * 7 + 1):
            first = (g.shape[0] - n) // 2
            assert np.array_equal(orc_cases.dirs_of(scene, "out", "n%d" % n), g[first:first + n])
    sh = orc_cases.dirs_of("cube", "out", "shuffled")
    assert not np.array_equal(sh, sph) and sorted(map(tuple, sh.tolist())) == sorted(map(tuple, sph.tolist()))
    # the irregular set: every listed kind, in every eighth position, classified as the library classifies it
    d, kinds = orc_cases.irregular_dirs()
    assert {k for k in kinds if k} == set(orc_cases.IRREGULAR_KINDS + orc_cases.EDGE_KINDS)
    assert all((k != "") == (i % 8 == 0) for i, k in enumerate(kinds))
    reg = orc_cases.regular(d)
    for i, k in enumerate(kinds):
        assert reg[i] == (k not in orc_cases.IRREGULAR_KINDS), (i, k)
        if k == "zero":
            assert not d[i].any()
        elif k == "nan":
            assert np.isnan(d[i]).sum() == 1
        elif k in ("+inf", "-inf"):
            assert np.isinf(d[i]).sum() == 1 and (d[i][np.isinf(d[i])] > 0).all() == (k == "+inf")
        elif k == "x1e300":
            assert np.isfinite(d[i]).all() and np.abs(d[i]).max() > 1e299
        elif k == "x1e-300":
            assert 0 < np.abs(d[i]).max() < 1e-299
        elif k == "x2^40":
            assert np.abs(d[i]).max() == 2.0 ** 40
        elif k == "x2^-40":
            assert np.abs(d[i]).max() == 2.0 ** -40
    assert np.array_equal(orc_cases.dirs_of("cube", "out", "irregular").view(np.uint64), d.view(np.uint64))


@pytest.mark.parametrize("scene", orc_cases.SCENES)
@pytest.mark.parametrize("origin", orc_cases.ORIGINS)
def test_gpu_cases_hit_between_10_and_90_percent(oracles, scene, origin):
    """Every (scene, origin, set) the GPU tests use: of the regular rays that do not point away from the box (their half-line meets it), between 10 % and 90 % hit the
    model (fewer than 50 such rays are too few for a band: the one-ray set)."""
    tree, brute = oracles[scene]
    prims = gbc.scene_data(scene)[1]
    o = orc_cases.origin_of(scene, origin)
    extra_hits = 0
    for name in orc_cases.SETS:
        dirs = orc_cases.dirs_of(scene, origin, name)
        reg = orc_cases.regular(dirs)
        use = reg & orc_cases.facing(scene, origin, np.where(reg[:, None], dirs, 0.0))
        res = orc_cases.oracle_trace(tree, brute, "bvh", False, prims, o, np.ascontiguousarray(dirs[use]))
        hit = np.asarray(res["hit"]).astype(bool)
        print("%s %s %s: %d of %d facing regular rays hit (%d rays)" % (scene, origin, name, hit.sum(), hit.size, dirs.shape[0]))
        if hit.size >= 50:
            assert 0.1 * hit.size < int(hit.sum()) < 0.9 * hit.size, (scene, origin, name, int(hit.sum()), hit.size)
        if prims:
            root = orc_cases.oracle_trace(tree, brute, "tree", True, prims, o, np.ascontiguousarray(dirs[reg]))
            extra_hits += int(np.count_nonzero((np.asarray(root["hit"]) == 1) & (np.asarray(root["tri_index"]) < 0)))
    if prims and origin != "far":
        assert extra_hits > 0                                       # the root geometry differs from the model alone somewhere
