"""sr_light_field_rays on the CPU: the ray sets of tests/lightfield_rays_model.py and what the input condition removes from them, the batch
model against the frame model and the reference's goldens, the declarations on every layer, and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lightfield_model as lfm
import lightfield_rays_model as lrm
import softray_amd as sa
from helpers import GOLDEN, ROOT, load_obj3ds, make_frame, orc, read_bmp_rgb

L = sa._lib
CAMERA_FRAMES = ("contention", "small_blur", "far_primitives", "view0_n64", "res128_high")


def oracle(model, prims=()):
    o = orc.Scene()
    o.set_triangles(*load_obj3ds(model))
    if prims:
        o.set_extra(list(prims))
    assert o.build_tree() == 0
    return o


# ---- the ray sets and the input condition ----
@pytest.mark.parametrize("name,cells", [("segments", {2: 9, 4: 441, 64: 10219}), ("panorama", {2: 7, 4: 72, 64: 7450})])
def test_segments_and_panorama_lose_no_ray(name, cells):
    starts, dirs = getattr(lrm, name)()
    assert starts.shape == dirs.shape == ((20000, 3) if name == "segments" else (128 * 64, 3))
    kept_s, kept_d, removed = lrm.usable(starts, dirs, lrm.RESOLUTIONS)
    assert removed == 0 and removed <= 0.01 * starts.shape[0] and kept_s.shape == starts.shape
    for n in lrm.RESOLUTIONS:
        with np.errstate(all="ignore"):
            idx, coord_margin, term_margin = lfm.sample_cells(kept_s, kept_d, n)     # the frame model's own margins agree with the per-ray filter
        assert coord_margin > lfm.MARGIN and term_margin > lfm.MARGIN
        if n in cells:
            assert np.unique(idx[idx >= 0]).size == cells[n]                           # many rays per cell and one ray per cell both occur
    inside = lrm.cells(starts, dirs, 4) >= 0
    assert (0.505 < inside.mean() < 0.515) if name == "segments" else inside.all()


@pytest.mark.parametrize("name", CAMERA_FRAMES)
def test_camera_sets_lose_at_most_one_percent(name):
    n, f, starts, dirs = lrm.camera(name)
    _, _, removed = lrm.usable(starts, dirs, (n,))
    assert removed <= 0.01 * starts.shape[0]
    assert removed == 0                                   # (their margins are what tests/test_lightfield_model.py checks per frame)


def test_irregular_set():
    starts, dirs = lrm.irregular()
    assert starts.shape[0] == 8 * 6 * len(lrm.SPECIALS)
    for x in lrm.SPECIALS:                                # every special value occurs in starts and in directions
        same = (lambda a: np.isnan(a)) if x != x else (lambda a: a == x)
        assert same(starts).any() and same(dirs).any()
    s, d, removed = lrm.usable(starts, dirs, lrm.RESOLUTIONS)
    assert removed <= 0.01 * starts.shape[0]
    cm, tm, inside = lrm.ray_margins(s, d, 4)
    assert (~inside).sum() > 20                           # lines that miss the sphere
    assert (inside & ~np.isfinite(cm)).sum() > 20         # lines whose coordinates are NaN: cell 0 on both sides
    idx = lrm.cells(s, d, 4)
    assert np.all(idx[inside & ~np.isfinite(cm)] == 0)


def test_resolution_one_has_one_cell():
    starts, dirs = lrm.segments(2000)
    s, d, removed = lrm.usable(starts, dirs, (1,))
    assert removed == 0
    idx = lrm.cells(s, d, 1)
    assert set(np.unique(idx).tolist()) == {-1, 0}
    o = oracle("obj.3ds")
    f = lfm.lf_frame(make_frame(16))
    m = lrm.LightFieldRaysModel(lfm.LightFieldModel(1))
    col, inside, filled = m.rays(o, f, s, d)
    assert filled == 1 and m.traced() == 0                # the canonical ray of cell 0 is NaN: the background, and nothing is traced
    assert np.all(col == m.background(f)) and inside.sum() == (idx == 0).sum()


# ---- the batch model against the frame model ----
@pytest.mark.parametrize("name", ("contention", "small_blur", "far_primitives", "view0_n64"))
def test_batch_model_equals_frame_model_on_camera_rays(name):
    model_file, prims, n, f = lfm.gpu_frame(name)
    o = oracle(model_file, prims)
    _, _, starts, dirs = lrm.camera(name)
    frame_model = lfm.LightFieldModel(n)
    want = frame_model.sample_colors(o, f)
    m = lrm.LightFieldRaysModel(lfm.LightFieldModel(n))
    got, inside, filled = m.rays(o, f, starts, dirs)
    assert np.array_equal(got, want) and filled == frame_model.filled.size and m.table.cache == frame_model.cache
    assert np.array_equal(inside.astype(bool), lrm.cells(starts, dirs, n) >= 0)
    again, _, filled = m.rays(o, f, starts, dirs)
    assert np.array_equal(again, want) and filled == 0


@pytest.mark.parametrize("name", ("noShading_lightFieldColor", "shading_lightFieldColor_focalBlurx4"))
def test_batch_model_gives_the_goldens(name):
    n, f, starts, dirs = lrm.camera(name)
    m = lrm.LightFieldRaysModel(lfm.LightFieldModel(n))
    col, _, _ = m.rays(oracle("obj.3ds"), f, starts, dirs)
    want = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))
    assert int(np.count_nonzero((lrm.resolve(col, f) & 0xFFFFFF) != want)) == 0


# ---- the layers ----
def test_the_call_is_declared_on_every_layer():
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert re.search(r"int\s+sr_light_field_rays\(sr_scene\*, const sr_frame\* frame, int64_t n, const double\* starts, const double\* dirs, uint32_t\* out,", header)
    assert re.search(r"int\s+sr_light_field_rays_device\(sr_scene\*, const sr_frame\* frame, int64_t n, const double\* d_starts, const double\* d_dirs, uint32_t\* d_out,", header)
    assert "#define SR_ABI_VERSION 5" in header
    assert "sr_light_field_rays" in L.SYMBOLS and "sr_light_field_rays_device" in L.SYMBOLS
    lib = L.lib()
    assert hasattr(lib, "sr_light_field_rays") and hasattr(lib, "sr_light_field_rays_device")
    assert callable(sa.GpuScene.light_field_rays) and callable(sa.GpuScene.light_field_rays_device)
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "uint64_t LightFieldRays(int64_t n, const double* starts, const double* dirs, uint32_t* out, uint8_t* inside = nullptr)" in hpp
    assert "sr_light_field_rays(" in hpp
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    assert "public uint[] LightFieldRays(" in cs and "public void LightFieldRaysDevice(" in cs
    assert "sr_light_field_rays(IntPtr scene, ref SrFrame frame, long n," in cs and "sr_light_field_rays_device(IntPtr scene, ref SrFrame frame, long n," in cs
    kernels = open(os.path.join(ROOT, "softray_amd", "csrc", "sr_kernels.hip")).read()
    for k in ("k_lfr_lookup", "k_lfr_finish", "k_lfri_lookup", "k_lfri_finish"):
        assert 'return "%s";' % k in kernels


# ---- the refusals that need no device ----
UNTOUCHED = 0x01020304
MESSAGES, TRIANGLES_MESSAGE, SHADOWS_MESSAGE, changed = lrm.MESSAGES, lrm.TRIANGLES_MESSAGE, lrm.SHADOWS_MESSAGE, lrm.changed


def call(s, f, n=2, starts=True, dirs=True, out=True, inside=True, options=0, device=False):
    """(return code, the `out` array, *filled) of one raw call with host arrays (never dereferenced: every case here is refused first)."""
    a = np.zeros((max(n, 1), 3))
    o = np.full(max(n, 1), UNTOUCHED, dtype=np.uint32)
    i = np.full(max(n, 1), 9, dtype=np.uint8)
    made = C.c_uint64(77)
    vp = lambda x, on: x.ctypes.data_as(C.c_void_p) if on else None                  # noqa: E731
    fr = C.byref(f) if f is not None else None
    if device:
        rc = L.lib().sr_light_field_rays_device(s, fr, n, vp(a, starts), vp(a, dirs), vp(o, out), vp(i, inside), options, None, None, None)
    else:
        rc = L.lib().sr_light_field_rays(s, fr, n, vp(a, starts), vp(a, dirs), vp(o, out), vp(i, inside), options, C.byref(made))
    assert np.all(o == UNTOUCHED) and np.all(i == 9)
    return rc, made.value


@pytest.mark.parametrize("device", [False, True], ids=["host_variant", "device_variant"])
def test_refusals_in_order_on_a_host_only_scene(device):
    s = sa.GpuScene(-1)
    s.set_triangles(*load_obj3ds("obj2.3DS"))
    h = s._h
    good = sa.Frame.from_buffer_copy(bytes(make_frame(16)))
    err = lambda: L.lib().sr_last_error().decode()                                   # noqa: E731
    # 1. SR_ERR_INVALID_ARG, whatever else is wrong with the frame
    bad_frame = changed(good, flags=L.F_VOXELS)
    for kw in (dict(n=-1), dict(starts=False), dict(dirs=False), dict(out=False), dict(options=1), dict(options=0x80000000)):
        assert call(h, bad_frame, device=device, **kw)[0] == L.SR_ERR_INVALID_ARG, kw
        assert err() == "bad argument to sr_light_field_rays", kw
    assert call(None, good, device=device)[0] == L.SR_ERR_INVALID_ARG
    assert call(h, None, device=device)[0] == L.SR_ERR_INVALID_ARG
    # ... the triangle switch, by name
    s.light_field_triangles = True
    assert call(h, good, device=device)[0] == L.SR_ERR_UNSUPPORTED and err() == TRIANGLES_MESSAGE
    assert call(h, good, n=0, device=device)[0] == L.SR_ERR_UNSUPPORTED
    assert call(h, good, options=1, device=device)[0] == L.SR_ERR_INVALID_ARG      # (bad arguments come first)
    s.light_field_triangles = False
    # 2. SR_ERR_UNSUPPORTED before the frame and its trace mode are validated (width 0 and no tree would be refused otherwise)
    for kw, text in MESSAGES:
        f = changed(good, **kw)
        f.width = 0
        assert call(h, f, device=device)[0] == L.SR_ERR_UNSUPPORTED and err() == text
    # 3. sr_render's validation of the frame -- shadows need the scene's switch, static ones are never accepted -- then of its trace mode
    assert call(h, changed(good, width=0), device=device)[0] == L.SR_ERR_INVALID_ARG
    assert call(h, changed(good, flags=L.F_SHADOWS), device=device)[0] == L.SR_ERR_UNSUPPORTED and err() == SHADOWS_MESSAGE
    s.light_field_shadows = True
    assert call(h, changed(good, flags=L.F_SHADOWS | L.F_STATIC_SHADOWS), device=device)[0] == L.SR_ERR_UNSUPPORTED and err() == SHADOWS_MESSAGE
    assert call(h, changed(good, flags=L.F_SHADOWS), device=device)[0] == L.SR_ERR_NOT_BUILT
    s.light_field_shadows = False
    assert call(h, good, device=device)[0] == L.SR_ERR_NOT_BUILT
    assert call(h, good, n=0, device=device)[0] == L.SR_ERR_NOT_BUILT                # n == 0 must pass these checks too
    s.build((sa.MODE_REF_TREE,))
    assert call(h, changed(good, trace_mode=sa.MODE_BVH), device=device)[0] == L.SR_ERR_NOT_BUILT
    # 4. the device comes last; `inside` may be NULL; SR_F_LIGHT_FIELD is implied and accepted
    for f in (good, lfm.lf_frame(changed(good))):
        assert call(h, f, device=device)[0] == L.SR_ERR_NO_DEVICE
        assert call(h, f, inside=False, device=device)[0] == L.SR_ERR_NO_DEVICE
    # n == 0: SR_OK before a device is asked for, *filled = 0, every array may be NULL
    rc, made = call(h, good, n=0, starts=False, dirs=False, out=False, inside=False, device=device)
    assert rc == L.SR_OK and (device or made == 0)
    assert not s.get_light_field().any()


def test_python_wrapper_checks_shapes():
    s = sa.GpuScene(-1)
    s.set_triangles(*load_obj3ds("obj2.3DS"))
    s.build((sa.MODE_REF_TREE,))
    f = sa.Frame.from_buffer_copy(bytes(make_frame(16)))
    with pytest.raises(ValueError):
        s.light_field_rays(f, np.zeros((3, 3)), np.zeros((2, 3)))
    with pytest.raises(sa.SoftrayError) as e:
        s.light_field_rays(f, np.zeros((3, 3)), np.ones((3, 3)))
    assert e.value.code == L.SR_ERR_NO_DEVICE
    out, inside, filled = s.light_field_rays(f, np.zeros((0, 3)), np.zeros((0, 3)))
    assert out.size == 0 and inside.size == 0 and filled == 0
