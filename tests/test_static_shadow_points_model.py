"""sr_static_shadow_points without a GPU: the call on every layer, its refusals in the documented order on a host-only scene, the cache's
read-back and upload on a host-only scene, and the CPU model (tests/static_shadow_points_model.py) pinned by the reference's two static
goldens: the oracle's hit points of the 100x100 frame in a static frame's fill order, first point of a cell generates, every point reads."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lightfield_model as lfm
import shadow_points_model as spm
import static_shadow_points_model as ssm
from helpers import GOLDEN, ROOT, camera_rays, load_obj3ds, make_frame, orc, read_bmp_rgb

NAME = "sr_static_shadow_points"


# ---- 1. the call on every layer ----
def test_call_is_declared_on_every_layer():
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert re.search(r"\bint\s+sr_static_shadow_points\(sr_scene\*, const sr_frame\* frame, int64_t n, const double\* pos, const double\* normal,", header)
    assert re.search(r"\bint\s+sr_static_shadow_points_device\(sr_scene\*, const sr_frame\* frame, int64_t n, const double\* d_pos, const double\* d_normal,", header)
    assert re.search(r"\bint\s+sr_get_shadow_cache\(sr_scene\*, uint8_t out\[128 \* 128 \* 128\]\);", header)
    assert re.search(r"\bint\s+sr_set_shadow_cache\(sr_scene\*, const uint8_t in\[128 \* 128 \* 128\]\);", header)
    assert "#define SR_ABI_VERSION 5" in header and re.search(r"SR_DBG_COUNT\s+= 17\b", header)
    import softray_amd as sa
    assert sa._lib.lib().sr_abi_version() == 5
    for sym in (NAME, NAME + "_device", "sr_get_shadow_cache", "sr_set_shadow_cache"):
        assert sym in sa._lib.SYMBOLS and hasattr(sa._lib.lib(), sym)
    for method in ("static_shadow_points", "static_shadow_points_device", "get_shadow_cache", "set_shadow_cache"):
        assert callable(getattr(sa.GpuScene, method, None)), method
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "uint64_t StaticShadowPoints(int64_t n, const double* pos, const double* normal, const uint32_t* color, uint32_t* out, uint8_t* amount," in hpp
    assert "sr_static_shadow_points(scene_, &f, n, pos, normal, color, out, amount" in hpp
    assert "void GetStaticShadowCache(uint8_t* out)" in hpp and "void SetStaticShadowCache(const uint8_t* in)" in hpp
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    assert "public uint[] StaticShadowPoints(" in cs and "public void StaticShadowPointsDevice(" in cs
    assert "public byte[] GetShadowCache()" in cs and "public void SetShadowCache(byte[] data)" in cs
    for sym in (NAME, NAME + "_device", "sr_get_shadow_cache", "sr_set_shadow_cache"):
        assert "extern int %s(" % sym in cs, sym
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc
    # the refusals the issue leaves in place
    api = open(os.path.join(ROOT, "softray_amd", "csrc", "sr_api.cpp")).read()
    assert '"sr_shadow_points: static shadows (SR_F_STATIC_SHADOWS)' in api and '"sr_ao_points: static shadows (SR_F_STATIC_SHADOWS)' in api


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


def raw_call(s, f, n, pos, nrm, color, out, amount, options=0, generators=None, device=False):
    """The C call itself: every argument may be None."""
    import softray_amd as sa
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    fr = None if f is None else C.byref(f)
    h = None if s is None else s._h
    if device:
        return sa._lib.lib().sr_static_shadow_points_device(h, fr, n, p(pos), p(nrm), p(color), p(out), p(amount), options, None, None, None)
    return sa._lib.lib().sr_static_shadow_points(h, fr, n, p(pos), p(nrm), p(color), p(out), p(amount), options,
                                                 None if generators is None else C.byref(generators))


# (the change, the name it is refused by, the whole message of sr_last_error)
REFUSED = [(dict(flags=1 << 13), "SR_F_AMBIENT_OCCLUSION",
            "sr_static_shadow_points: ambient occlusion (SR_F_AMBIENT_OCCLUSION) is another decorator, not ShadowMethod's step"),
           (dict(flags=1 << 6), "SR_F_PATH_TRACING",
            "sr_static_shadow_points: path tracing (SR_F_PATH_TRACING) replaces the decorator chain ShadowMethod is part of"),
           (dict(flags=1 << 7), "SR_F_VOXELS", "sr_static_shadow_points: voxel rendering (SR_F_VOXELS) has no shadow step"),
           (dict(flags=1 << 15), "SR_F_LIGHT_FIELD",
            "sr_static_shadow_points: the light field (SR_F_LIGHT_FIELD) stores colours of canonical rays, not of a caller's points"),
           (dict(flags=1 << 8), "SR_F_SINGLE_KERNEL",
            "sr_static_shadow_points: the one-kernel renderer (SR_F_SINGLE_KERNEL) has no stage to enter"),
           (dict(max_bounces=1), "max_bounces > 0",
            "sr_static_shadow_points: mirror bounces (max_bounces > 0) belong to a camera ray, not to a point"),
           (dict(strips=(16, 2, 0)), "strip_count > 0",
            "sr_static_shadow_points: row strips (strip_count > 0) divide a frame's rows, not a batch of points")]


@pytest.mark.parametrize("device", [False, True], ids=["host_arrays", "device_arrays"])
def test_refusals_come_in_order_on_a_host_only_scene(device):
    import softray_amd as sa
    E = sa._lib
    s = host_scene()
    pos, nrm = np.zeros((4, 3)), np.ones((4, 3))
    col, out, amt = np.full(4, 0xFF808080, dtype=np.uint32), np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint8)
    f = sr_frame()
    call = lambda *a, **k: raw_call(*a, device=device, **k)
    # (1) bad arguments -- also together with a refused flag, a frame that does not validate and a mode that is not built
    worst = lfm.apply_change(sr_frame(mode=sa.MODE_BVH), dict(flags=1 << 13))
    worst.sub_pixel_res = 0
    for fr in (f, worst):
        assert call(s, fr, -1, pos, nrm, col, out, amt) == E.SR_ERR_INVALID_ARG
        assert E.lib().sr_last_error().decode() == "bad argument to " + NAME
        assert call(s, fr, 4, None, nrm, col, out, amt) == E.SR_ERR_INVALID_ARG
        assert call(s, fr, 4, pos, None, col, out, amt) == E.SR_ERR_INVALID_ARG
        assert call(s, fr, 4, pos, nrm, col, None, None) == E.SR_ERR_INVALID_ARG
        assert call(None, fr, 4, pos, nrm, col, out, amt) == E.SR_ERR_INVALID_ARG
        for options in (2, 3, 1 << 31):
            assert call(s, fr, 4, pos, nrm, col, out, amt, options) == E.SR_ERR_INVALID_ARG
    assert call(s, None, 4, pos, nrm, col, out, amt) == E.SR_ERR_INVALID_ARG
    assert call(s, None, 0, None, None, None, None, None) == E.SR_ERR_INVALID_ARG
    # (2) what names no step of ShadowMethod on a bare point, each by name -- before the rest of the frame's validation and the mode
    for change, name, text in REFUSED:
        for base in (sr_frame(), sr_frame(mode=sa.MODE_BVH)):
            fr = lfm.apply_change(base, change)
            fr.sub_pixel_res = 0 if base.trace_mode == sa.MODE_BVH else 1
            assert call(s, fr, 4, pos, nrm, col, out, amt) == E.SR_ERR_UNSUPPORTED, name
            msg = E.lib().sr_last_error().decode()
            assert msg == text and msg.startswith(NAME + ":") and name in msg, (name, msg)
            assert call(s, fr, 0, None, None, None, None, None) == E.SR_ERR_UNSUPPORTED, name     # n == 0 passes no check
    # (3) the rest of the frame's validation, then the trace mode
    bad = sr_frame()
    bad.sub_pixel_res = 0
    assert call(s, bad, 4, pos, nrm, col, out, amt) == E.SR_ERR_INVALID_ARG
    assert call(s, bad, 0, None, None, None, None, None) == E.SR_ERR_INVALID_ARG
    assert call(s, sr_frame(mode=sa.MODE_BVH), 4, pos, nrm, col, out, amt) == E.SR_ERR_NOT_BUILT
    assert call(s, sr_frame(mode=sa.MODE_BVH), 0, None, None, None, None, None) == E.SR_ERR_NOT_BUILT
    assert call(host_scene(build=False), f, 4, pos, nrm, col, out, amt) == E.SR_ERR_NOT_BUILT
    assert call(sa.GpuScene(-1), f, 4, pos, nrm, col, out, amt) == E.SR_ERR_NO_MODEL
    # (4) a valid call lacks only a device; the shadow switches are implied or given, the library options and both lights pass, each output
    #     is optional
    for fr in (f, sr_frame(shadows=True), sr_frame(shadows=True, static_shadows=True), sr_frame(static_shadows=True), sr_frame(point_light=False),
               sr_frame(shadow_samples=130), sr_frame(concurrency=3)):
        for flags in (0, 1 << 9, 1 << 11, 1 << 12):
            fr.flags |= flags
            for options in (0, E.POINTS_COHERENT):
                assert call(s, fr, 4, pos, nrm, col, out, amt, options) == E.SR_ERR_NO_DEVICE
                assert call(s, fr, 4, pos, nrm, None, out, None, options) == E.SR_ERR_NO_DEVICE
                assert call(s, fr, 4, pos, nrm, None, None, amt, options) == E.SR_ERR_NO_DEVICE
    assert not out.any() and not amt.any()
    # n == 0 is SR_OK, touches nothing and reports no generator
    assert call(s, f, 0, None, None, None, None, None) == 0
    assert call(s, f, 0, pos, nrm, col, out, amt) == 0 and not out.any() and not amt.any()
    if not device:
        made = C.c_uint64(77)
        assert call(s, f, 0, None, None, None, None, None, generators=made) == 0 and made.value == 0
    assert not s.get_shadow_cache().any()


def test_python_wrapper_refuses_mismatched_arrays():
    import softray_amd as sa
    s = host_scene()
    with pytest.raises(ValueError):
        s.static_shadow_points(sr_frame(), np.zeros((4, 3)), np.zeros((3, 3)))
    with pytest.raises(ValueError):
        s.static_shadow_points(sr_frame(), np.zeros((4, 3)), np.zeros((4, 3)), np.zeros(5, dtype=np.uint32))
    with pytest.raises(ValueError):
        s.set_shadow_cache(np.zeros(128 * 128, dtype=np.uint8))
    with pytest.raises(sa.SoftrayError) as e:
        s.static_shadow_points(sr_frame(), np.zeros((4, 3)), np.zeros((4, 3)))
    assert e.value.code == sa._lib.SR_ERR_NO_DEVICE
    with pytest.raises(sa.SoftrayError) as e:
        s.static_shadow_points(sr_frame(), np.zeros((4, 3)), np.zeros((4, 3)), want_out=False, want_amount=False)
    assert e.value.code == sa._lib.SR_ERR_INVALID_ARG
    out, amount, made = s.static_shadow_points(sr_frame(), np.zeros((0, 3)), np.zeros((0, 3)))
    assert out.shape == (0,) and amount.shape == (0,) and made == 0


# ---- 3. the cache on a host-only scene ----
def test_cache_round_trip_on_a_host_only_scene():
    import softray_amd as sa
    s = host_scene()
    assert s.get_shadow_cache().shape == (128, 128, 128) and not s.get_shadow_cache().any()          # a fresh scene reads zeros
    data = np.random.default_rng(7).integers(0, 256, (128, 128, 128)).astype(np.uint8)
    s.set_shadow_cache(data)
    assert np.array_equal(s.get_shadow_cache(), data)
    s.set_shadow_cache(data.reshape(-1)[::-1])                                                       # flat arrays are the file's bytes
    assert np.array_equal(s.get_shadow_cache().reshape(-1), data.reshape(-1)[::-1])
    s.reset_shadow_cache()
    assert not s.get_shadow_cache().any()
    s.set_shadow_cache(data)
    s.set_triangles(*load_obj3ds("obj2.3DS"))                                                        # a new model drops what was set
    assert not s.get_shadow_cache().any()
    s.set_shadow_cache(data)
    s.load_3ds(open(os.path.join(GOLDEN, "obj.3ds"), "rb").read())
    assert not s.get_shadow_cache().any()
    E = sa._lib
    buf = np.zeros(128 ** 3, dtype=np.uint8)
    assert E.lib().sr_get_shadow_cache(None, buf.ctypes.data_as(C.c_void_p)) == E.SR_ERR_INVALID_ARG
    assert E.lib().sr_get_shadow_cache(s._h, None) == E.SR_ERR_INVALID_ARG
    assert E.lib().sr_set_shadow_cache(s._h, None) == E.SR_ERR_INVALID_ARG
    assert E.lib().sr_set_shadow_cache(None, buf.ctypes.data_as(C.c_void_p)) == E.SR_ERR_INVALID_ARG
    # the AO cache is another array
    s.set_shadow_cache(data)
    assert not s.get_ao_cache().any()


# ---- 4. the model's parts ----
def test_cell_formula_and_first_wins():
    pos = np.array([[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0], [-0.7, 0.2, 9.0], [np.nan, 0.5, -0.5], [np.inf, -np.inf, 0.0],
                    [-0.5 + 1.5 / 127, -0.5 + 0.5 / 127, 0.4999], [-0.504, 1e300, -1e300]])
    want = [(0, 0, 0), (127, 127, 127), (63, 63, 63), (0, 88, 127), (0, 127, 0), (127, 0, 63), (1, 0, 126), (0, 127, 0)]
    assert ssm.cells(pos).tolist() == [(x * 128 + y) * 128 + z for x, y, z in want]
    assert ssm.cache_bytes(np.array([0, 1, 50, 99, 100]), 100).tolist() == [1, 3, 128, 252, 255]
    assert ssm.cache_bytes(np.array([0, 1]), 1).tolist() == [1, 255]
    cache = np.zeros(ssm.CELLS, dtype=np.uint8)
    cache[5] = 9
    cell = np.array([7, 5, 7, 3, 5, 3, 7])
    assert ssm.generators_of(cell, cache).tolist() == [True, False, False, True, False, False, False]
    assert ssm.golden_order(100, 100)[:101].tolist() == list(range(100)) + [2500]                     # row 0 of block 0, then row 0 of block 1


# ---- 5. the model is pinned by the reference's two static goldens ----
@pytest.fixture(scope="module")
def obj_scene():
    o = orc.Scene()
    o.set_triangles(*load_obj3ds())
    assert o.build_tree() == 0
    return o


@pytest.mark.parametrize("name,kw", [("shading_staticShadows", dict()), ("noShading_staticShadows", dict(shading=False))])
def test_model_over_the_oracles_hit_points_in_fill_order_is_the_golden_frame(obj_scene, name, kw):
    f = make_frame(100, 100, shadows=True, **kw)
    origin, dirs = camera_rays(f)
    res = obj_scene.trace(lfm.TRACE_ROOT_TREE, np.broadcast_to(origin, dirs.shape).copy(), dirs)
    hit = res["hit"].astype(bool)
    order = ssm.golden_order(100, 100)
    row, col = np.arange(10000) // 100, np.arange(10000) % 100
    assert np.array_equal(order, np.argsort(((row % 25) * 4 + row // 25) * 100 + col, kind="stable"))
    pix = order[hit[order]]                                                   # the hit pixels in fill order
    assert pix.size == 6716
    pos, nrm = res["pos"][pix], res["normal"][pix]
    shaded = orc.shade_points(f, pos, nrm, res["color"][pix]) if kw.get("shading", True) else res["color"][pix]
    cache = np.zeros(ssm.CELLS, dtype=np.uint8)
    amount, out, made = ssm.static_shadow_points(obj_scene, f, pos, nrm, lfm.TRACE_ROOT_TREE, cache, shaded)
    got = np.full(hit.size, (f.background_argb | 0xFF000000) & 0xFFFFFFFF, dtype=np.uint32)
    got[pix] = out
    want = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))
    assert int(np.count_nonzero((got.reshape(100, 100) & 0xFFFFFF) != want)) == 0
    # the input's own conditions: generators, readers of a cell another point generated, penumbra bytes
    gen = ssm.generators_of(ssm.cells(pos), np.zeros(ssm.CELLS, dtype=np.uint8))
    penumbra = int(np.count_nonzero((amount[gen] > 1) & (amount[gen] < 255)))
    print("%s: %d generators, %d readers, %d penumbra bytes, bytes %d .. %d" % (name, made, pix.size - made, penumbra, amount.min(), amount.max()))
    assert made == int(gen.sum()) >= 5000 and pix.size - made >= 1000 and penumbra >= 500
    assert amount.min() == 1 and amount.max() == 255
    assert np.all(np.abs(pos) <= 0.5)                                         # no point lies outside the cube
    assert int(np.count_nonzero(cache)) == made
    # a second application reads only; the batch in two halves equals the one call
    again = ssm.static_shadow_points(obj_scene, f, pos, nrm, lfm.TRACE_ROOT_TREE, cache, shaded)
    assert again[2] == 0 and np.array_equal(again[0], amount) and np.array_equal(again[1], out)
    half, c2 = pix.size // 2, np.zeros(ssm.CELLS, dtype=np.uint8)
    a = ssm.static_shadow_points(obj_scene, f, pos[:half], nrm[:half], lfm.TRACE_ROOT_TREE, c2, shaded[:half])
    b = ssm.static_shadow_points(obj_scene, f, pos[half:], nrm[half:], lfm.TRACE_ROOT_TREE, c2, shaded[half:])
    assert a[2] + b[2] == made and np.array_equal(np.concatenate([a[0], b[0]]), amount) and np.array_equal(c2, cache)
    # scan order is another cache: the fill order matters
    c3 = np.zeros(ssm.CELLS, dtype=np.uint8)
    scan = np.flatnonzero(hit)
    ssm.static_shadow_points(obj_scene, f, res["pos"][scan], res["normal"][scan], lfm.TRACE_ROOT_TREE, c3)
    assert np.array_equal(c3 != 0, cache != 0) and not np.array_equal(c3, cache)


def test_model_bytes_are_the_dynamic_escape_counts(obj_scene):
    """A generator's byte is made of exactly sr_shadow_points' escape count, not-finite probe ends included."""
    f = make_frame(16, shadows=True, shadow_samples=17)
    bpos, bnrm, has_nan = spm.bad_points()
    cache = np.zeros(ssm.CELLS, dtype=np.uint8)
    amount, out, made = ssm.static_shadow_points(obj_scene, f, bpos, bnrm, lfm.TRACE_ROOT_TREE, cache)
    gen = ssm.generators_of(ssm.cells(bpos), np.zeros(ssm.CELLS, dtype=np.uint8))
    esc = spm.escapes(obj_scene, f, bpos, bnrm, lfm.TRACE_ROOT_TREE)
    assert made == int(gen.sum()) and 3 < made < bpos.shape[0]
    assert np.array_equal(amount[gen], ssm.cache_bytes(esc[gen], 17))
    assert np.all(amount[gen & has_nan] == 255)
    assert np.array_equal(out, spm.ao_model.modulate(np.full(bpos.shape[0], 0xFFFFFFFF, dtype=np.uint32), amount))
