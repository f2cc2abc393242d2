"""sr_shadow_points without a GPU: the call on every layer, its refusals in the documented order on a host-only scene, the CPU model
(tests/shadow_points_model.py) pinned by the reference's shading_shadows golden, and the rule for points that are not finite against what
the oracle answers for their rays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lightfield_model as lfm
import lightfield_shadow_model as lsm
import shadow_points_model as spm
from helpers import GOLDEN, ROOT, camera_rays, edge_light_case, edge_light_frame, load_obj3ds, make_frame, orc, read_bmp_rgb, unit_cube_scene


# ---- 1. the call on every layer ----
def test_call_is_declared_on_every_layer():
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert re.search(r"\bint\s+sr_shadow_points\(sr_scene\*, const sr_frame\* frame, int64_t n, const double\* pos, const double\* normal,", header)
    assert re.search(r"\bint\s+sr_shadow_points_device\(sr_scene\*, const sr_frame\* frame, int64_t n, const double\* d_pos, const double\* d_normal,", header)
    assert "#define SR_POINTS_COHERENT 1u" in header
    assert "#define SR_ABI_VERSION 5" in header and re.search(r"SR_DBG_COUNT\s+= 17\b", header)
    import softray_amd as sa
    assert sa._lib.lib().sr_abi_version() == 5
    for sym in ("sr_shadow_points", "sr_shadow_points_device"):
        assert sym in sa._lib.SYMBOLS and hasattr(sa._lib.lib(), sym)
    assert sa._lib.POINTS_COHERENT == 1
    assert callable(getattr(sa.GpuScene, "shadow_points", None)) and callable(getattr(sa.GpuScene, "shadow_points_device", None))
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "void ShadowPoints(int64_t n, const double* pos, const double* normal, const uint32_t* color, uint32_t* out, bool coherent = false)" in hpp
    assert "sr_shadow_points(scene_, &f, n, pos, normal, color, out" in hpp
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    assert "public uint[] ShadowPoints(" in cs and "public void ShadowPointsDevice(" in cs
    assert "extern int sr_shadow_points(" in cs and "extern int sr_shadow_points_device(" in cs
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "sr_shadow_points" in open(os.path.join(ROOT, doc)).read(), doc


# ---- 2. refusals, in order, before the device is looked at ----
def host_scene(build=True):
    import softray_amd as sa
    s = sa.GpuScene(-1)
    s.set_triangles(*load_obj3ds("obj2.3DS"))
    if build:
        s.build((sa.MODE_REF_TREE,))
    return s


def sr_frame(**kw):
    import softray_amd as sa
    return sa.Frame.from_buffer_copy(bytes(make_frame(16, **kw)))


def raw_call(s, f, n, pos, nrm, color, out, options=0, device=False):
    """The C call itself: every argument may be None."""
    import softray_amd as sa
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    fr = None if f is None else C.byref(f)
    h = None if s is None else s._h
    if device:
        return sa._lib.lib().sr_shadow_points_device(h, fr, n, p(pos), p(nrm), p(color), p(out), options, None, None)
    return sa._lib.lib().sr_shadow_points(h, fr, n, p(pos), p(nrm), p(color), p(out), options)


# (the change, the name it is refused by, the whole message of sr_last_error)
REFUSED = [(dict(flags=1 << 5), "SR_F_STATIC_SHADOWS",
            "sr_shadow_points: static shadows (SR_F_STATIC_SHADOWS) are a cache over a frame's fill order, not a step on a point"),
           (dict(flags=1 << 13), "SR_F_AMBIENT_OCCLUSION",
            "sr_shadow_points: ambient occlusion (SR_F_AMBIENT_OCCLUSION) is another decorator, not ShadowMethod's step"),
           (dict(flags=1 << 6), "SR_F_PATH_TRACING",
            "sr_shadow_points: path tracing (SR_F_PATH_TRACING) replaces the decorator chain ShadowMethod is part of"),
           (dict(flags=1 << 7), "SR_F_VOXELS", "sr_shadow_points: voxel rendering (SR_F_VOXELS) has no shadow step"),
           (dict(flags=1 << 15), "SR_F_LIGHT_FIELD",
            "sr_shadow_points: the light field (SR_F_LIGHT_FIELD) stores colours of canonical rays, not of a caller's points"),
           (dict(flags=1 << 8), "SR_F_SINGLE_KERNEL", "sr_shadow_points: the one-kernel renderer (SR_F_SINGLE_KERNEL) has no stage to enter"),
           (dict(max_bounces=1), "max_bounces > 0", "sr_shadow_points: mirror bounces (max_bounces > 0) belong to a camera ray, not to a point"),
           (dict(strips=(16, 2, 0)), "strip_count > 0",
            "sr_shadow_points: row strips (strip_count > 0) divide a frame's rows, not a batch of points")]


@pytest.mark.parametrize("device", [False, True], ids=["host_arrays", "device_arrays"])
def test_refusals_come_in_order_on_a_host_only_scene(device):
    import softray_amd as sa
    E = sa._lib
    s = host_scene()
    pos, nrm = np.zeros((4, 3)), np.ones((4, 3))
    col, out = np.full(4, 0xFF808080, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    f = sr_frame()
    call = lambda *a, **k: raw_call(*a, device=device, **k)
    # (1) bad arguments -- also together with a refused flag, a frame that does not validate and a mode that is not built
    worst = lfm.apply_change(sr_frame(mode=sa.MODE_BVH), dict(flags=1 << 5))
    worst.sub_pixel_res = 0
    for fr in (f, worst):
        assert call(s, fr, -1, pos, nrm, col, out) == E.SR_ERR_INVALID_ARG
        assert E.lib().sr_last_error().decode() == "bad argument to sr_shadow_points"
        assert call(s, fr, 4, None, nrm, col, out) == E.SR_ERR_INVALID_ARG
        assert call(s, fr, 4, pos, None, col, out) == E.SR_ERR_INVALID_ARG
        assert call(s, fr, 4, pos, nrm, col, None) == E.SR_ERR_INVALID_ARG
        assert call(None, fr, 4, pos, nrm, col, out) == E.SR_ERR_INVALID_ARG
        for options in (2, 3, 1 << 31):
            assert call(s, fr, 4, pos, nrm, col, out, options) == E.SR_ERR_INVALID_ARG
    assert call(s, None, 4, pos, nrm, col, out) == E.SR_ERR_INVALID_ARG
    assert call(s, None, 0, None, None, None, None) == E.SR_ERR_INVALID_ARG
    # (2) what names no step of ShadowMethod on a bare point, each by name -- before the rest of the frame's validation and the mode
    for change, name, text in REFUSED:
        for base in (sr_frame(), sr_frame(mode=sa.MODE_BVH)):
            fr = lfm.apply_change(base, change)
            fr.sub_pixel_res = 0 if base.trace_mode == sa.MODE_BVH else 1
            assert call(s, fr, 4, pos, nrm, col, out) == E.SR_ERR_UNSUPPORTED, name
            msg = E.lib().sr_last_error().decode()
            assert msg == text and msg.startswith("sr_shadow_points:") and name in msg, (name, msg)
            assert call(s, fr, 0, None, None, None, None) == E.SR_ERR_UNSUPPORTED, name           # n == 0 passes no check
    # (3) the rest of the frame's validation, then the trace mode
    bad = sr_frame()
    bad.sub_pixel_res = 0
    assert call(s, bad, 4, pos, nrm, col, out) == E.SR_ERR_INVALID_ARG
    assert call(s, sr_frame(mode=sa.MODE_BVH), 4, pos, nrm, col, out) == E.SR_ERR_NOT_BUILT
    assert call(host_scene(build=False), f, 4, pos, nrm, col, out) == E.SR_ERR_NOT_BUILT
    assert call(sa.GpuScene(-1), f, 4, pos, nrm, col, out) == E.SR_ERR_NO_MODEL
    # (4) a valid call lacks only a device; shadows are implied, the library options and both lights pass
    for fr in (f, sr_frame(shadows=True), sr_frame(point_light=False), sr_frame(shadow_samples=130)):
        for flags in (0, 1 << 9, 1 << 11, 1 << 12):
            fr.flags |= flags
            for options in (0, E.POINTS_COHERENT):
                assert call(s, fr, 4, pos, nrm, col, out, options) == E.SR_ERR_NO_DEVICE
                assert call(s, fr, 4, pos, nrm, None, out, options) == E.SR_ERR_NO_DEVICE
    assert not out.any()
    # n == 0 is SR_OK and touches nothing
    assert call(s, f, 0, None, None, None, None) == 0
    assert call(s, f, 0, pos, nrm, col, out) == 0 and not out.any()


def test_python_wrapper_refuses_mismatched_arrays():
    s = host_scene()
    with pytest.raises(ValueError):
        s.shadow_points(sr_frame(), np.zeros((4, 3)), np.zeros((3, 3)))
    with pytest.raises(ValueError):
        s.shadow_points(sr_frame(), np.zeros((4, 3)), np.zeros((4, 3)), np.zeros(5, dtype=np.uint32))
    import softray_amd as sa
    with pytest.raises(sa.SoftrayError) as e:
        s.shadow_points(sr_frame(), np.zeros((4, 3)), np.zeros((4, 3)))
    assert e.value.code == sa._lib.SR_ERR_NO_DEVICE
    assert s.shadow_points(sr_frame(), np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)


# ---- 3. the model is pinned by the reference's golden ----
@pytest.fixture(scope="module")
def obj_scene():
    o = orc.Scene()
    o.set_triangles(*load_obj3ds())
    assert o.build_tree() == 0
    return o


def test_model_over_the_oracles_hit_points_is_the_golden_frame(obj_scene):
    f = make_frame(100, 100, shadows=True)
    origin, dirs = camera_rays(f)
    res = obj_scene.trace(lfm.TRACE_ROOT_TREE, np.broadcast_to(origin, dirs.shape).copy(), dirs)
    hit = res["hit"].astype(bool)
    assert 3000 < int(hit.sum()) < 8000
    pos, nrm = res["pos"][hit], res["normal"][hit]
    shaded = orc.shade_points(f, pos, nrm, res["color"][hit])
    got = np.full(hit.size, (f.background_argb | 0xFF000000) & 0xFFFFFFFF, dtype=np.uint32)
    got[hit] = spm.shadowed(obj_scene, f, pos, nrm, shaded, lfm.TRACE_ROOT_TREE)
    want = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", "shading_shadows.bmp"))
    assert int(np.count_nonzero((got.reshape(100, 100) & 0xFFFFFF) != want)) == 0
    esc = spm.escapes(obj_scene, f, pos, nrm, lfm.TRACE_ROOT_TREE)
    assert esc.min() == 0 and esc.max() == 100 and 0 < int(np.count_nonzero((esc > 0) & (esc < 100)))       # umbra, light and penumbra are all in it
    assert np.array_equal((esc / 100 * 255).astype(np.uint8), lsm.shadow_bytes(obj_scene, f, pos, nrm, lfm.TRACE_ROOT_TREE).astype(np.uint8))
    white = spm.shadowed(obj_scene, f, pos[:50], nrm[:50], None, lfm.TRACE_ROOT_TREE)
    assert np.array_equal(white, spm.shadowed(obj_scene, f, pos[:50], nrm[:50], np.full(50, 0xFFFFFFFF, dtype=np.uint32), lfm.TRACE_ROOT_TREE))


# ---- 4. points that are not finite ----
def rule_scenes():
    out = []
    o = orc.Scene()
    o.set_triangles(*load_obj3ds())
    assert o.build_tree() == 0
    out.append(("obj", o, make_frame(16, shadows=True, shadow_samples=17)))
    for signs in ((1, 0, 0), (0, -1, 0), (-1, -1, -1), (1, 1, -1)):
        c = edge_light_case(signs, 0.1, 0.6)
        plain, extra = orc.Scene(), orc.Scene()
        for s in (plain, extra):
            s.set_triangles(*unit_cube_scene(2000))
            assert s.build_tree() == 0
        extra.set_extra(c["prims"])
        out.append(("cube%s" % (signs,), plain, edge_light_frame(c, 16, 16), c))
        out.append(("cube+extra%s" % (signs,), extra, edge_light_frame(c, 16, 16), c))
    return out


@pytest.mark.parametrize("point_light", [True, False], ids=["point", "directional"])
def test_non_finite_rule_is_what_the_oracle_answers(point_light):
    pos, nrm, has_nan = spm.bad_points()
    assert has_nan.sum() >= 12 and (~has_nan).sum() >= 20
    blocked_somewhere = False
    for entry in rule_scenes():
        name, o, f = entry[:3]
        if not point_light:
            f.flags &= ~orc.F_POINT_LIGHT
        samples = lsm.shadow_samples_of(f)
        src, dirs = spm.sample_rays(f, spm.probe_ends(pos, nrm))
        for target in (lfm.TRACE_ROOT_TREE, 0, 1):                                      # Scene.trace: the root geometry; the triangles by brute force; their tree
            res = o.trace(target, src.reshape(-1, 3), dirs.reshape(-1, 3))
            hit = res["hit"].astype(bool).reshape(-1, samples)
            assert not hit[has_nan].any(), name                                    # a NaN component: nothing answers, the model traces nothing
            if "extra" not in name:
                assert not hit.any(), name                                         # an infinite component: no triangle answers
            else:
                assert np.all(res["tri_index"][res["hit"].astype(bool)] < 0), name # ... the extra primitives can
            blocked = (hit & (res["ray_frac"].reshape(-1, samples) <= 1.0)).sum(axis=1)
            if target == lfm.TRACE_ROOT_TREE:
                assert np.array_equal(spm.escapes(o, f, pos, nrm, target), samples - blocked), name
                assert np.all(spm.escapes(o, f, pos, nrm, target)[has_nan] == samples)
            blocked_somewhere |= bool(blocked.any())
    assert blocked_somewhere == point_light          # an infinite direction is cut at rayFrac 0 by a plane; an infinite start by nothing
