"""The frame G-buffer (sr_render_hits) without a GPU: the calls on every layer, sr_frame_sample_count against the CPU model's camera samples,
the refusals in the documented order on a host-only scene, and the model the GPU tests compare with (tests/gbuffer_model.py) pinned by the
reference's goldens: scan order and resolve of the composition are the reference's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gbuffer_cases as gbc
import gbuffer_model as gbm
import lightfield_model as lfm
import pathtrace_model as ptm
from helpers import GOLDEN, ROOT, load_obj3ds, make_frame, orc, read_bmp_rgb


# ---- 1. the calls on every layer ----
def test_calls_are_declared_on_every_layer():
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert re.search(r"\bint64_t\s+sr_frame_sample_count\(const sr_frame\*\);", header)
    assert re.search(r"\bint\s+sr_render_hits\(sr_scene\*, const sr_frame\* frame, double\* starts, double\* dirs, uint8_t\* hit, double\* ray_frac,", header)
    assert re.search(r"\bint\s+sr_render_hits_device\(sr_scene\*, const sr_frame\* frame, double\* d_starts, double\* d_dirs, uint8_t\* d_hit,", header)
    assert re.search(r"\bint\s+sr_shade_points_device\(sr_scene\*, const sr_frame\* frame, int64_t n, const double\* d_pos, const double\* d_normal,", header)
    assert "#define SR_ABI_VERSION 5" in header and re.search(r"SR_DBG_COUNT\s+= 17\b", header) and re.search(r"#define SR_STATS_COUNT 24\b", header)
    import softray_amd as sa
    assert sa._lib.lib().sr_abi_version() == 5
    for sym in ("sr_frame_sample_count", "sr_render_hits", "sr_render_hits_device", "sr_shade_points_device"):
        assert sym in sa._lib.SYMBOLS and hasattr(sa._lib.lib(), sym)
    for name in ("render_hits", "render_hits_device", "shade_points_device", "sample_count"):
        assert callable(getattr(sa.GpuScene, name, None)), name
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "void RenderHits(double* starts, double* dirs, uint8_t* hit, double* ray_frac, double* pos, double* normal, uint32_t* color, int32_t* tri_index)" in hpp
    assert "sr_render_hits(scene_, &f, starts, dirs, hit, ray_frac, pos, normal, color, tri_index" in hpp
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    assert "public FrameHits RenderHits(" in cs and "public void RenderHitsDevice(" in cs and "public void ShadePointsDevice(" in cs
    for sym in ("sr_render_hits(", "sr_render_hits_device(", "sr_shade_points_device(", "sr_frame_sample_count("):
        assert "extern int " + sym in cs or "extern long " + sym in cs, sym
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "sr_render_hits" in text and "sr_shade_points_device" in text, doc


# ---- 2. sr_frame_sample_count ----
@pytest.mark.parametrize("n", [1, 2, 3])
def test_sample_count_is_the_models(n):
    import softray_amd as sa
    for w, h, a, b in ((37, 21, 0, 20), (37, 21, -5, 9), (37, 21, 4, 400), (48, 40, 5, 17), (1, 1, 0, 0), (16, 16, -3, -1), (16, 16, 20, 30),
                       (16, 16, 9, 3), (16, 16, 30, -2)):
        f = make_frame(w, h, sub_pixel_res=n, start_row=a, end_row=b)
        sf = sa.Frame.from_buffer_copy(bytes(f))
        lo, hi = min(max(0, a), h - 1), min(max(0, b), h - 1)
        want = ptm.camera_samples(f)[0].shape[0] if hi >= lo else 0
        assert sa.GpuScene.sample_count(sf) == want == max(0, hi - lo + 1) * w * n * n, (w, h, a, b)
    assert sa._lib.lib().sr_frame_sample_count(None) == 0


# ---- 3. refusals, in order, before the device is looked at ----
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


GUARD = 0xA5


def guarded():
    """Eight output arrays for a 16x16 frame, filled with a guard byte."""
    n = 256
    return [np.full(n * k, GUARD, dtype=np.uint8) for k in (24, 24, 1, 8, 24, 24, 4, 4)]


def raw_call(s, f, arrays, device=False):
    import softray_amd as sa
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    fr = None if f is None else C.byref(f)
    h = None if s is None else s._h
    args = [p(a) for a in arrays]
    if device:
        return sa._lib.lib().sr_render_hits_device(h, fr, *args, None, None)
    return sa._lib.lib().sr_render_hits(h, fr, *args, None)


# (the change, the name it is refused by, the whole message of sr_last_error)
REFUSED = [(dict(flags=1 << 7), "SR_F_VOXELS",
            "sr_render_hits: voxel rendering (SR_F_VOXELS) replaces the root geometry; a voxel hit has no position or triangle"),
           (dict(flags=1 << 15), "SR_F_LIGHT_FIELD",
            "sr_render_hits: the light field (SR_F_LIGHT_FIELD) replaces the primary stage: a cell stores a colour, not a hit"),
           (dict(flags=1 << 8), "SR_F_SINGLE_KERNEL", "sr_render_hits: the one-kernel renderer (SR_F_SINGLE_KERNEL) has no primary stage to read"),
           (dict(strips=(16, 2, 0)), "strip_count > 0", "sr_render_hits: row strips (strip_count > 0) lay the rows out compactly; pass a row range")]


@pytest.mark.parametrize("device", [False, True], ids=["host_arrays", "device_arrays"])
def test_refusals_come_in_order_on_a_host_only_scene(device):
    import softray_amd as sa
    E = sa._lib
    s = host_scene()
    arrays = guarded()
    none = [None] * 8
    call = lambda sc, fr, arr=arrays: raw_call(sc, fr, arr, device=device)
    f = sr_frame()
    # (1) a NULL scene or frame -- also with a refused flag, a frame that does not validate and a mode that is not built
    worst = lfm.apply_change(sr_frame(mode=sa.MODE_BVH), dict(flags=1 << 7))
    worst.sub_pixel_res = 0
    for fr in (f, worst):
        assert call(None, fr) == E.SR_ERR_INVALID_ARG
        assert E.lib().sr_last_error().decode() == "bad argument to sr_render_hits"
    assert call(s, None) == E.SR_ERR_INVALID_ARG and call(s, None, none) == E.SR_ERR_INVALID_ARG
    # (2) what replaces the root geometry or the primary stage, each by name -- before the rest of the frame's validation and the mode
    for change, name, text in REFUSED:
        for base in (sr_frame(), sr_frame(mode=sa.MODE_BVH)):
            fr = lfm.apply_change(base, change)
            fr.sub_pixel_res = 0 if base.trace_mode == sa.MODE_BVH else 1
            for arr in (arrays, none):
                assert call(s, fr, arr) == E.SR_ERR_UNSUPPORTED, name
                msg = E.lib().sr_last_error().decode()
                assert msg == text and msg.startswith("sr_render_hits:") and name in msg, (name, msg)
    # (3) sr_render's validation of the frame, then of its trace mode
    bad = sr_frame()
    bad.sub_pixel_res = 0
    assert call(s, bad) == E.SR_ERR_INVALID_ARG
    bad = sr_frame()
    bad.width = 0
    assert call(s, bad) == E.SR_ERR_INVALID_ARG
    assert call(s, sr_frame(mode=sa.MODE_BVH)) == E.SR_ERR_NOT_BUILT
    assert call(host_scene(build=False), f) == E.SR_ERR_NOT_BUILT
    assert call(sa.GpuScene(-1), f) == E.SR_ERR_NO_MODEL
    # (4) a valid call lacks only a device: the decorator switches are not read, so whatever sr_render would refuse in them passes
    decorated = [sr_frame(), sr_frame(shading=False), sr_frame(shadows=True), sr_frame(shadows=True, static_shadows=True),
                 sr_frame(sub_pixel_res=2, focal_blur=True), sr_frame(shadows=True, shadow_samples=130)]
    for flags in (1 << 13, (1 << 13) | (1 << 14), 1 << 6, (1 << 6) | (1 << 13), 1 << 10, 1 << 12, 1 << 9, 1 << 11):
        fr = sr_frame()
        fr.flags |= flags
        decorated.append(fr)
    bounced = sr_frame(shadows=True)
    bounced.max_bounces = 2
    bounced.flags |= 1 << 13                       # (ambient occlusion with mirror bounces: sr_render refuses the pair)
    decorated.append(bounced)
    for fr in decorated:
        for arr in (arrays, none):
            assert call(s, fr, arr) == E.SR_ERR_NO_DEVICE, hex(fr.flags)
    for a in arrays:
        assert np.all(a == GUARD)
    # an empty row range that passes these checks is SR_OK and touches nothing; one that does not pass them is refused all the same
    for rows in ((9, 3), (30, -2)):
        empty = sr_frame(start_row=rows[0], end_row=rows[1])
        assert sa.GpuScene.sample_count(empty) == 0
        for arr in (arrays, none):
            assert call(s, empty, arr) == 0
        assert call(s, lfm.apply_change(sr_frame(start_row=9, end_row=3), dict(flags=1 << 15))) == E.SR_ERR_UNSUPPORTED
        assert call(s, sr_frame(start_row=9, end_row=3, mode=sa.MODE_BVH)) == E.SR_ERR_NOT_BUILT
    for a in arrays:
        assert np.all(a == GUARD)
    assert s.render_hits(sr_frame(start_row=9, end_row=3), rays=True)["starts"].shape == (0, 3)
    with pytest.raises(sa.SoftrayError) as e:
        s.render_hits(sr_frame())
    assert e.value.code == E.SR_ERR_NO_DEVICE


def test_shade_points_device_refuses_like_shade_points():
    import softray_amd as sa
    E, L = sa._lib, sa._lib.lib()
    s = host_scene()
    f = sr_frame()
    pos, nrm = np.zeros((4, 3)), np.ones((4, 3))
    col, out = np.full(4, 0xFF808080, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    host = lambda sc, fr, n, a, b, c, d: L.sr_shade_points(None if sc is None else sc._h, None if fr is None else C.byref(fr), n, p(a), p(b), p(c), p(d))
    dev = lambda sc, fr, n, a, b, c, d: L.sr_shade_points_device(None if sc is None else sc._h, None if fr is None else C.byref(fr), n, p(a), p(b), p(c), p(d), None)
    bad = sr_frame()
    bad.sub_pixel_res = 0
    cases = [(None, f, 4, pos, nrm, col, out), (s, f, -1, pos, nrm, col, out), (s, f, 4, None, nrm, col, out), (s, f, 4, pos, None, col, out),
             (s, f, 4, pos, nrm, None, out), (s, f, 4, pos, nrm, col, None), (s, None, 4, pos, nrm, col, out), (s, bad, 4, pos, nrm, col, out),
             (s, f, 4, pos, nrm, col, out), (s, f, 0, None, None, None, None), (s, lfm.apply_change(sr_frame(), dict(flags=(1 << 13) | (1 << 6))), 4, pos, nrm, col, out)]
    for case in cases:
        want = host(*case)
        assert dev(*case) == want, case[2:3]
        assert want != 0                                  # (a host-only scene: even n == 0 asks for the device first, in both)
    assert host(*cases[0]) == E.SR_ERR_INVALID_ARG and host(*cases[8]) == E.SR_ERR_NO_DEVICE
    assert not out.any()


# ---- 4. the model of the GPU tests is pinned by the reference's goldens ----
@pytest.fixture(scope="module")
def obj_scene():
    o = orc.Scene()
    o.set_triangles(*load_obj3ds())
    assert o.build_tree() == 0
    return o


@pytest.mark.parametrize("name,kw", [("shading", dict()), ("shading_4xAA", dict(sub_pixel_res=4)),
                                     ("shading_focalBlurx2", dict(focal_blur=True, sub_pixel_res=2)), ("shading_shadows", dict(shadows=True))])
def test_chain_over_the_models_hits_is_the_golden_frame(obj_scene, name, kw):
    f = make_frame(100, 100, **kw)
    got = gbm.compose(obj_scene, f, ptm.TRACE_ROOT_TREE)
    want = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))
    assert got.shape == want.shape
    assert int(np.count_nonzero((got & 0xFFFFFF) != want)) == 0
    # ... and is what the oracle renders, alpha included
    ref, _ = obj_scene.render(f, threads=os.cpu_count() or 1)
    assert np.array_equal(got.reshape(-1), np.asarray(ref, dtype=np.uint32).reshape(-1))


def test_model_conventions_of_a_miss_and_of_extra_geometry(obj_scene):
    """What the GPU tests rely on in Scene.trace: a miss is zeros and triangle -1."""
    f = gbc.frame_of(("obj", "away", 16, 16, None, 2, False))        # the model lies behind the camera
    _, _, res = gbm.hits(obj_scene, f, ptm.TRACE_ROOT_TREE)
    assert not res["hit"].any() and not res["pos"].any() and not res["normal"].any() and not res["ray_frac"].any() and not res["color"].any()
    assert np.all(res["tri_index"] == -1)


# ---- 5. the cases of the GPU tests: checked here, on the CPU, not tuned on the GPU ----
def test_gpu_cases_hit_between_10_and_90_percent_and_cover_both_camera_positions():
    scenes = {name: gbc.oracle_scenes(name)[0] for name in ("obj", "cube", "small")}
    seen, extra_hits = set(), 0
    for case in gbc.CASES:
        f = gbc.frame_of(case)
        _, _, res = gbm.hits(scenes[case[0]], f, ptm.TRACE_ROOT_TREE)
        hit = res["hit"].astype(bool)
        outside = gbc.outside_axes(gbc.frame_of(case, focal_blur=False), gbc.scene_data(case[0])[0])      # (the camera; focal blur moves the origin per sample)
        if case[1] == "away":
            assert not hit.any()
            continue
        assert (outside == 7) == (case[1] == "out"), gbc.case_id(case)
        seen.add(case[1])
        if hit.size >= 256:                                # (a 1x1 frame is one pixel: degenerate)
            assert 0.1 * hit.size < int(hit.sum()) < 0.9 * hit.size, (gbc.case_id(case), int(hit.sum()), hit.size)
        if case[0] == "cube":
            n_extra = int(np.count_nonzero(res["tri_index"][hit] < 0))
            assert n_extra > 0, gbc.case_id(case)
            extra_hits += n_extra
    assert seen == {"out", "in"} and extra_hits > 100
    assert gbc.scene_data("small")[0][1].size <= 64
