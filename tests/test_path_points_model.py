"""sr_path_points without a GPU: the points model (tests/path_points_model.py) pinned to the frame model the path-traced frames are held
to (tests/pathtrace_model.py) and through it to the reference's goldens, the split-batch rule, every refusal on a host-only scene in the
header's order, and the symbols on every layer.  Every comparison is an exact equality."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import path_points_model as ppm
import pathtrace_model as ptm
import softray_amd as sa
from helpers import GOLDEN, ROOT, load_obj3ds, make_frame, orc, read_bmp_rgb

L = sa._lib
GOLDENS = [("pathTracing_noShading", "triangles", {}),
           ("pathTracing_noShading_focalBlurx2", "triangles", dict(focal_blur=True, sub_pixel_res=2, focal_depth=1.0)),
           ("pathTracing_noShading_6_geometry", "primitives", dict(depth=3.0))]


def path_frame(res=100, **kw):
    f = make_frame(res, shading=kw.pop("shading", False), **kw)
    f.flags |= ptm.F_PATH_TRACING
    return f


@pytest.fixture(scope="module")
def scenes():
    t = orc.Scene()
    t.set_triangles(*load_obj3ds("obj2.3DS"))
    assert t.build_tree() == 0
    p = orc.Scene()
    p.set_triangles(*load_obj3ds("obj.3ds"))
    assert p.build_tree() == 0
    p.set_extra(ptm.PRIMITIVES)
    q = orc.Scene()                                                  # the primitives scene's model without its extra geometry
    q.set_triangles(*load_obj3ds("obj.3ds"))
    assert q.build_tree() == 0
    return dict(triangles=t, primitives=p, triangles_of_primitives=q)


def primary_hits(scene, f, shade):
    s, d = ptm.camera_samples(f)
    first = scene.trace(ptm.TRACE_ROOT_TREE, s, d)
    hit = first["hit"].astype(bool)
    pos, nrm, col = first["pos"][hit], first["normal"][hit], first["color"][hit]
    if shade:
        col = orc.shade_points(f, pos, nrm, col)
    return hit, pos, nrm, col


def resolve(col, f):
    n = f.sub_pixel_res
    if n == 1:
        return col.reshape(-1, f.width)
    c = col.reshape(-1, n * n).astype(np.int64)
    ch = [((c >> s) & 255).sum(1) // (n * n) for s in (16, 8, 0)]
    return (0xFF000000 | (ch[0] << 16) | (ch[1] << 8) | ch[2]).astype(np.uint32).reshape(-1, f.width)


# ---- 1. the points model is the frame model with the frame taken away ----
@pytest.mark.parametrize("name,scene,kw", GOLDENS, ids=[g[0] for g in GOLDENS])
def test_chain_over_the_primary_hits_is_the_frame_and_the_golden(scenes, name, scene, kw):
    o = scenes[scene]
    f = path_frame(concurrency=1, **kw)
    hit, pos, nrm, col = primary_hits(o, f, False)
    assert hit.sum() > 500
    out, incoming, dirs = ppm.path_points(o, ptm.TRACE_ROOT_TREE, f, pos, nrm, col, first_sample=0)
    want = ptm.sample_colors(o, f)
    got = np.full(hit.size, (f.background_argb | 0xFF000000) & 0xFFFFFFFF, dtype=np.uint32)
    got[hit] = out
    assert np.array_equal(got, want)
    gold = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))
    # (the goldens were rendered with the default four row blocks: the first block of the one-block frame is theirs)
    px = resolve(got, f) & 0xFFFFFF
    assert px.shape == gold.shape and np.array_equal(px[:25], gold[:25])
    assert np.all(np.abs((dirs * dirs).sum(axis=1) - 1.0) < 1e-12) and np.all((dirs * nrm).sum(axis=1) >= -1e-15)


@pytest.mark.parametrize("name,scene,kw", GOLDENS, ids=[g[0] for g in GOLDENS])
def test_every_block_of_a_four_block_frame_is_a_call_from_sample_zero(scenes, name, scene, kw):
    o = scenes[scene]
    f = path_frame(concurrency=4, **kw)
    hit, pos, nrm, col = primary_hits(o, f, False)
    want = ptm.sample_colors(o, f)
    got = np.full(hit.size, (f.background_argb | 0xFF000000) & 0xFFFFFFFF, dtype=np.uint32)
    block_samples = 25 * f.width * f.sub_pixel_res ** 2
    before = np.concatenate([[0], np.cumsum(hit)])
    for b in range(4):
        a, e = before[b * block_samples], before[(b + 1) * block_samples]
        assert e > a
        out, _, _ = ppm.path_points(o, ptm.TRACE_ROOT_TREE, f, pos[a:e], nrm[a:e], col[a:e], first_sample=0)
        blk = np.flatnonzero(hit[b * block_samples:(b + 1) * block_samples]) + b * block_samples
        got[blk] = out
    assert np.array_equal(got, want)
    gold = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))
    assert np.array_equal(resolve(got, f) & 0xFFFFFF, gold)                            # the committed .bmp, whole


def test_shaded_chain_is_the_shaded_frame(scenes):
    o = scenes["primitives"]
    f = path_frame(40, shading=True, concurrency=1, depth=3.0)
    hit, pos, nrm, col = primary_hits(o, f, True)
    out, incoming, _ = ppm.path_points(o, ptm.TRACE_ROOT_TREE, f, pos, nrm, col)
    assert np.array_equal(out, ptm.sample_colors(o, f)[hit]) and len(np.unique(incoming)) > 20


def test_one_call_equals_three_chained_calls(scenes):
    o = scenes["primitives"]
    f = path_frame(40, concurrency=1, depth=3.0)
    hit, pos, nrm, col = primary_hits(o, f, False)
    n = int(hit.sum())
    info = {}
    whole = ppm.path_points(o, ptm.TRACE_ROOT_TREE, f, pos, nrm, col, first_sample=11, info=info)
    assert info["hit"].mean() > 0.2 and (~info["hit"]).mean() > 0.2
    cuts = [0, 101, 102 + n // 3, n]
    first, parts = 11, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        parts.append(ppm.path_points(o, ptm.TRACE_ROOT_TREE, f, pos[a:b], nrm[a:b], col[a:b], first_sample=first))
        first += b - a
    for k in range(3):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k])
    moved = ppm.path_points(o, ptm.TRACE_ROOT_TREE, f, pos, nrm, col, first_sample=12)
    assert not np.array_equal(moved[2], whole[2]) and not np.array_equal(moved[0], whole[0])           # the sequence really moved


def test_origins_that_are_not_finite(scenes):
    """The rules of include/softray.h, each asserted on the model: a NaN component of the origin -- no hit; an infinite one -- no model
    triangle answers under either target, and an extra primitive's rayFrac from such an origin is +-inf or NaN, which is never `< best`,
    so the ray misses as well.  The colour step then runs on what IEEE gives: incoming 0 times an infinite or NaN n . d is NaN, a NaN
    channel is byte 0; a zero normal gives n . d = 0 and leaves the own colour."""
    o = scenes["primitives"]
    f = path_frame(16, depth=3.0)
    p0 = (0.1, 0.2, -0.1)
    inf = np.inf
    cases = [(p0, (0.0, 1.0, 0.0), "finite"), (p0, (np.nan, 1.0, 0.0), "nan"), (p0, (0.0, inf, 0.0), "inf"), (p0, (0.0, -inf, 0.0), "inf"),
             (p0, (inf, -inf, 0.0), "inf"), ((np.nan, 0.0, 0.0), (0.0, 0.0, 0.0), "nan"), (p0, (inf, 0.0, 0.0), "inf"), (p0, (0.0, 0.0, -inf), "inf"),
             ((inf, 0.2, -0.1), (0.0, 1.0, 0.0), "inf"), ((0.1, -inf, -0.1), (0.0, 0.0, 0.0), "inf"), ((inf, inf, inf), (-inf, 0.0, 0.0), "nan"),
             ((1.7976e308, 0.0, 0.0), (1.79e308, 0.0, 0.0), "inf")]                       # finite inputs, the origin overflows
    pos = np.array([c[0] for c in cases])
    nrm = np.array([c[1] for c in cases])
    kind = np.array([c[2] for c in cases])
    with np.errstate(invalid="ignore", over="ignore"):
        origin = pos + nrm * ppm.OFFSET
    assert np.array_equal(np.isnan(origin).any(axis=1), kind == "nan")
    assert np.array_equal(np.isinf(origin).any(axis=1) & ~np.isnan(origin).any(axis=1), kind == "inf")
    own = 0xFF102030
    col = np.full(len(cases), own, dtype=np.uint32)
    info = {}
    out, incoming, dirs = ppm.path_points(o, ptm.TRACE_ROOT_TREE, f, pos, nrm, col, info=info)
    assert np.isfinite(dirs).all()                                                     # the direction comes from the draws alone
    assert np.allclose((dirs * dirs).sum(axis=1), 1.0, rtol=0, atol=1e-15)
    bad = kind != "finite"
    assert not info["hit"][bad].any() and not incoming[bad].any()
    # the colour step: n . d is NaN or infinite wherever the normal is not finite -> 0 * that = NaN -> bytes 0; a finite normal keeps the own colour + 0
    with np.errstate(invalid="ignore"):
        frac = (nrm[:, 0] * dirs[:, 0] + nrm[:, 1] * dirs[:, 1]) + nrm[:, 2] * dirs[:, 2]
    wild = ~np.isfinite(frac)
    assert np.array_equal(wild, ~np.isfinite(nrm).all(axis=1)) and wild.sum() == 7
    assert np.all(out[wild] == 0xFF000000) and np.all(out[bad & ~wild] == own)
    # the pieces of the rule, on the oracle itself: its triangles never answer an infinite origin, under either target ...
    tris = scenes["triangles_of_primitives"]
    sel = kind == "inf"
    with np.errstate(invalid="ignore", over="ignore"):
        for target in (ptm.TRACE_ROOT_TREE, ptm.TRACE_NEAREST):
            assert not tris.trace(target, origin[sel], dirs[sel])["hit"].any()
        # ... and with the extra primitives (spheres here) nothing answers either
        assert not o.trace(ptm.TRACE_ROOT_TREE, origin[sel], dirs[sel])["hit"].any()
    # the same points in another order and split in two calls: each point's answer depends on its own draws alone
    a = ppm.path_points(o, ptm.TRACE_ROOT_TREE, f, pos[:5], nrm[:5], col[:5])
    b = ppm.path_points(o, ptm.TRACE_ROOT_TREE, f, pos[5:], nrm[5:], col[5:], first_sample=5)
    assert np.array_equal(np.concatenate([a[0], b[0]]), out) and np.array_equal(np.concatenate([a[2], b[2]]), dirs)
    white, _, _ = ppm.path_points(o, ptm.TRACE_ROOT_TREE, f, pos[:1], nrm[:1], None)
    assert white[0] != out[0] and white[0] >> 24 == 0xFF                               # color None is 0xFFFFFFFF, not the caller's colour


# ---- 2. validation on a host-only scene, in the header's order ----
def call(s, f, n=4, pos=True, nrm=True, out=True, incoming=True, dirs=True, first=0, options=0, device=False):
    p = np.zeros((max(n, 1), 3))
    o = np.zeros(max(n, 1), dtype=np.uint32)
    i = np.zeros(max(n, 1), dtype=np.uint32)
    d = np.zeros((max(n, 1), 3))
    vp = lambda x, on: x.ctypes.data_as(C.c_void_p) if on else None
    fr = C.byref(f) if f is not None else None
    if device:
        return L.lib().sr_path_points_device(s, fr, n, vp(p, pos), vp(p, nrm), None, vp(o, out), vp(i, incoming), vp(d, dirs), first, options, None, None)
    return L.lib().sr_path_points(s, fr, n, vp(p, pos), vp(p, nrm), None, vp(o, out), vp(i, incoming), vp(d, dirs), first, options)


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
    shadows = "sr_path_points: shadows (SR_F_SHADOWS, dynamic or static) are ShadowMethod's step, which follows this one: sr_shadow_points"
    unsupported = [(changed(flags=L.F_SHADOWS), shadows), (changed(flags=L.F_SHADOWS | L.F_STATIC_SHADOWS), shadows),
                   (changed(flags=L.F_AMBIENT_OCCLUSION),
                    "sr_path_points: ambient occlusion (SR_F_AMBIENT_OCCLUSION) is AmbientOcclusionMethod's step, which follows this one: sr_ao_points"),
                   (changed(flags=L.F_VOXELS), "sr_path_points: voxel rendering (SR_F_VOXELS) has no surface point to bounce from"),
                   (changed(flags=L.F_LIGHT_FIELD),
                    "sr_path_points: the light field (SR_F_LIGHT_FIELD) stores colours of canonical rays, not of a caller's points"),
                   (changed(flags=L.F_SINGLE_KERNEL), "sr_path_points: the one-kernel renderer (SR_F_SINGLE_KERNEL) has no stage to enter"),
                   (changed(max_bounces=1), "sr_path_points: mirror bounces (max_bounces > 0) belong to a camera ray, not to a point"),
                   (changed(strip_rows=16, strip_count=2, strip_index=0),
                    "sr_path_points: row strips (strip_count > 0) divide a frame's rows, not a batch of points")]
    # 1. SR_ERR_INVALID_ARG, whatever else is wrong with the frame (the model has no tree yet: SR_ERR_NOT_BUILT would come later)
    bad_frame = unsupported[0][0]
    for kw in (dict(n=-1), dict(pos=False), dict(nrm=False), dict(out=False, incoming=False, dirs=False), dict(options=1), dict(options=0x80000000),
               dict(first=2 ** 40 - 3), dict(first=2 ** 40 + 1, n=0), dict(first=2 ** 64 - 1)):
        assert call(h, bad_frame, device=device, **kw) == L.SR_ERR_INVALID_ARG, kw
        assert L.lib().sr_last_error().decode() == "bad argument to sr_path_points", kw
    assert call(None, good, device=device) == L.SR_ERR_INVALID_ARG
    assert call(h, None, device=device) == L.SR_ERR_INVALID_ARG
    assert call(h, good, first=2 ** 40 - 4, device=device) != L.SR_ERR_INVALID_ARG                       # first_sample + n == 2^40 is legal
    # 2. SR_ERR_UNSUPPORTED before the frame and its trace mode are validated (width 0 and no tree would be refused otherwise)
    for f, text in unsupported:
        f.width = 0
        assert call(h, f, device=device) == L.SR_ERR_UNSUPPORTED and L.lib().sr_last_error().decode() == text and text.startswith("sr_path_points: ")
    # the order inside the group: shadows are named before ambient occlusion, that before voxels
    assert call(h, changed(flags=L.F_SHADOWS | L.F_AMBIENT_OCCLUSION | L.F_VOXELS), device=device) == L.SR_ERR_UNSUPPORTED
    assert "shadows" in L.lib().sr_last_error().decode()
    assert call(h, changed(flags=L.F_AMBIENT_OCCLUSION | L.F_VOXELS), device=device) == L.SR_ERR_UNSUPPORTED
    assert "ambient occlusion" in L.lib().sr_last_error().decode()
    # 3. sr_render's validation of the frame, then of its trace mode
    assert call(h, changed(width=0), device=device) == L.SR_ERR_INVALID_ARG
    assert call(h, changed(sub_pixel_res=0), device=device) == L.SR_ERR_INVALID_ARG
    assert call(h, good, device=device) == L.SR_ERR_NOT_BUILT
    assert call(h, good, n=0, device=device) == L.SR_ERR_NOT_BUILT                                       # n == 0 must pass these checks too
    s.build((sa.MODE_REF_TREE,))
    assert call(h, changed(trace_mode=sa.MODE_BVH), device=device) == L.SR_ERR_NOT_BUILT
    assert call(h, changed(trace_mode=7), device=device) == L.SR_ERR_INVALID_ARG
    # 4. the device comes last; one output is enough; SR_F_PATH_TRACING is accepted (it is implied)
    for kw in (dict(), dict(out=False, incoming=False), dict(incoming=False, dirs=False), dict(out=False, dirs=False)):
        assert call(h, good, device=device, **kw) == L.SR_ERR_NO_DEVICE
    assert call(h, changed(flags=L.F_PATH_TRACING | L.F_PRIMARY_STATS_ONLY), device=device) == L.SR_ERR_NO_DEVICE
    # n == 0: SR_OK before a device is asked for, every pointer may be NULL
    assert call(h, good, n=0, out=False, incoming=False, dirs=False, pos=False, nrm=False, device=device) == L.SR_OK


def test_python_wrapper_checks_shapes():
    s = sa.GpuScene(-1)
    s.set_triangles(*load_obj3ds("obj2.3DS"))
    s.build((sa.MODE_REF_TREE,))
    f = sa.Frame.from_buffer_copy(bytes(make_frame(16)))
    with pytest.raises(ValueError):
        s.path_points(f, np.zeros((3, 3)), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        s.path_points(f, np.zeros((3, 3)), np.zeros((3, 3)), color=np.zeros(2, dtype=np.uint32))
    with pytest.raises(sa.SoftrayError) as e:
        s.path_points(f, np.zeros((3, 3)), np.zeros((3, 3)))
    assert e.value.code == L.SR_ERR_NO_DEVICE
    out, incoming, dirs = s.path_points(f, np.zeros((0, 3)), np.zeros((0, 3)))
    assert out.size == 0 and incoming.size == 0 and dirs.shape == (0, 3)


# ---- 3. the symbols on every layer ----
def test_symbols_on_every_layer():
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert "#define SR_ABI_VERSION 5" in header and L.lib().sr_abi_version() == 5
    assert re.search(r"\bSR_DBG_COUNT\s*=\s*17\b", header) and re.search(r"#define\s+SR_STATS_COUNT\s+24\b|\bSR_STATS_COUNT\s*=\s*24\b", header)
    assert len([k for k in dir(L) if k.startswith("DBG_")]) == 17
    for sym in ("sr_path_points", "sr_path_points_device"):
        assert re.search(r"\bint\s+%s\(" % sym, header), sym
        assert sym in L.SYMBOLS and hasattr(L.lib(), sym)
    assert "uint64_t first_sample" in header and "double* dirs" in header and "uint32_t* incoming" in header
    vp, i64, u64, u32 = C.c_void_p, C.c_int64, C.c_uint64, C.c_uint32
    assert L.lib().sr_path_points.argtypes == [vp, vp, i64, vp, vp, vp, vp, vp, vp, u64, u32]
    assert L.lib().sr_path_points_device.argtypes == [vp, vp, i64, vp, vp, vp, vp, vp, vp, u64, u32, vp, vp]
    assert L.lib().sr_path_points.restype == C.c_int32 and L.lib().sr_path_points_device.restype == C.c_int32
    assert hasattr(sa.GpuScene, "path_points") and hasattr(sa.GpuScene, "path_points_device")
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "PathTracePoints(" in hpp and "sr_path_points(" in hpp
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    for sym, nargs in (("sr_path_points", 11), ("sr_path_points_device", 13)):
        m = re.search(r"\[DllImport\(Lib\)\] public static extern int %s\(([^)]*)\);" % sym, cs)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs == len(getattr(L.lib(), sym).argtypes)
    # the wrappers shade as a frame does: what ShadingMethod reads is theirs to take and to pass on, as ShadePointsDevice does
    for name in ("PathPoints", "PathPointsDevice"):
        m = re.search(r"public \w+(?:\[\])? %s\(([^)]*)\)\s*\{(.*?)\n        \}" % name, cs, re.S)
        assert m, name
        for prm in ("double fieldOfViewDepth", "double ambient", "double shininess", "Vector lightDirView", "Vector lightPosView", "ulong firstSample"):
            assert prm in m.group(1), (name, prm)
        fill = re.search(r"FillFrame\(([^;]*)\);", m.group(2), re.S).group(1)
        assert re.search(r"randomSeed,\s*fieldOfViewDepth, 1\.0, 0\.0, ambient, shininess, lightDirView, lightPosView, 4$", fill), (name, fill)
    kernels = open(os.path.join(ROOT, "softray_amd", "csrc", "sr_kernels.hip")).read()
    assert '"path_points_rays"' in kernels
    pipeline = open(os.path.join(ROOT, "softray_amd", "csrc", "sr_pipeline.hip")).read()
    for k in ("k_pp_ingest", "k_pp_finish", "k_pp_finish_walked"):
        assert re.search(r"\bvoid %s\(" % k, pipeline), k
