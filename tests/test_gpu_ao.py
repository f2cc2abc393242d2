"""Ambient occlusion (SR_F_AMBIENT_OCCLUSION, rayTraceAmbientOcclusion) on the device against the CPU model (tests/ao_model.py, whose
invariants tests/test_ao_model.py checks) -- bit for bit: every comparison is an exact equality over every pixel and every cache byte."""
import os
import subprocess

import numpy as np
import pytest

import ao_model as aom
import pathtrace_model as ptm
import softray_amd as sa
from helpers import GOLDEN, ROOT, c1_spheres, load_obj3ds, make_frame, orc

pytestmark = pytest.mark.gpu
MODES = {"tree": sa.MODE_REF_TREE, "brute": sa.MODE_BRUTE, "bvh": sa.MODE_BVH}


def ao_frame(w=100, h=None, uncached=False, **kw):
    return aom.ao_frame(make_frame(w, h, shading=kw.pop("shading", False), **kw), uncached)


def as_sr(frame, mode):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = mode
    return f


def gpu_rows(g, frame, mode, extra_flags=0):
    """The frame's rows start_row..end_row as the library renders them, [rows, width]; the other rows must stay untouched."""
    f = as_sr(frame, mode)
    f.flags |= extra_flags
    out = np.full(f.width * f.height, 0x01020304, dtype=np.uint32)
    g.render(f, out=out, stats=True)
    a = min(max(0, f.start_row), f.height - 1)
    b = min(max(0, f.end_row), f.height - 1)
    px = out.reshape(f.height, f.width)
    assert np.all(px[:a] == 0x01020304) and np.all(px[b + 1:] == 0x01020304)
    return px[a:b + 1].copy()


def pair(v9, argb, bmin, bmax, prims=(), modes=(sa.MODE_REF_TREE, sa.MODE_BVH), on_device=None, devices=None):
    g, o = (sa.GpuScene(devices=devices) if devices else sa.GpuScene(0)), orc.Scene()
    for s in (g, o):
        s.set_triangles(v9, argb, bmin, bmax)
        if prims:
            s.set_extra(list(prims))
    g.build(tuple(modes), on_device=on_device)
    assert o.build_tree() == 0
    return g, o


@pytest.fixture(scope="module")
def obj2_pair():
    return pair(*load_obj3ds("obj2.3DS"))


@pytest.fixture(scope="module")
def obj_pair():
    return pair(*load_obj3ds("obj.3ds"))


@pytest.fixture(scope="module")
def primitives_pair():
    return pair(*load_obj3ds("obj.3ds"), prims=ptm.PRIMITIVES)


def target_of(mode):
    return aom.TRACE_NEAREST if mode == "bvh" else aom.TRACE_ROOT_TREE


def check_uncached(g, o, f, modes=("tree", "bvh"), extra_flags=0):
    """Uncached frames leave no state behind: one fresh model per trace semantics."""
    want = {}
    for m in modes:
        t = target_of(m)
        if t not in want:
            want[t] = aom.AoModel().render(o, f, t)
        got = gpu_rows(g, f, MODES[m], extra_flags)
        assert got.shape == want[t].shape
        assert int(np.count_nonzero(got != want[t])) == 0, m
    return want


def check_cached(g, o, model, f, mode="tree", extra_flags=0):
    """One cached frame on the scene's and the model's running caches: pixels and the whole cache, byte for byte."""
    want = model.render(o, f, target_of(mode))
    got = gpu_rows(g, f, MODES[mode], extra_flags)
    assert int(np.count_nonzero(got != want)) == 0
    assert int(np.count_nonzero(g.get_ao_cache() != model.cache3())) == 0
    return got


# ---- 1. uncached, no shading, every trace mode and both BVH builds ----
@pytest.mark.parametrize("structure", ["tree", "brute", "bvh_device", "bvh_host"])
def test_uncached_no_shading_in_every_mode(obj2_pair, structure):
    g, o = obj2_pair
    if structure == "bvh_host":
        g = pair(*load_obj3ds("obj2.3DS"), modes=(sa.MODE_BVH,), on_device=False)[0]
        assert g.bvh_stats()[3] == 0
    elif structure == "bvh_device":
        assert g.bvh_stats()[3] == 1
    mode = "bvh" if structure.startswith("bvh") else structure
    f = ao_frame(100, uncached=True)
    want = check_uncached(g, o, f, modes=(mode,))[target_of(mode)]
    plain, _ = g.render(as_sr(make_frame(100, shading=False), MODES[mode]))
    assert np.count_nonzero(plain.reshape(100, 100) != want) > 500            # the probes changed the image
    assert not g.get_ao_cache().any()                                          # nothing is stored


def test_uncached_on_a_larger_model(obj_pair):
    check_uncached(*obj_pair, ao_frame(96, 80, uncached=True, shading=True))


def test_bvh_probes_as_nearest_hit_walks(obj_pair):
    """SR_MODE_BVH probes are any-hit walks with the limit 2.0 by default; hook 34 runs them as nearest-hit walks: the same bytes."""
    g, o = obj_pair
    try:
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, 34)
        check_uncached(g, o, ao_frame(96, 80, uncached=True, shading=True), modes=("bvh",))
        g.reset_ao_cache()
        model = aom.AoModel()
        check_cached(g, o, model, ao_frame(96, 80, shading=True, sub_pixel_res=2), "bvh")
        assert model.generators > 1000
    finally:
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
        g.reset_ao_cache()


def test_bvh_any_hit_probes_with_extra_geometry(primitives_pair):
    """SR_MODE_BVH with extra geometry: the any-hit probe walk tests the primitives in front with the limit 2.0.  The oracle has no
    nearest-hit target that includes extra geometry, so the check is the library's own nearest-hit walk (hook 34): equal pixels and
    equal cache bytes, uncached and cached, with hit points outside the unit cube."""
    g, _ = primitives_pair
    results = {}
    try:
        for hook in (-1, 34):
            g.debug_set(sa._lib.DBG_KERNEL_SWITCH, hook)
            g.reset_ao_cache()
            unc = gpu_rows(g, ao_frame(100, 80, uncached=True, shading=True, depth=3.0), sa.MODE_BVH)
            cold = gpu_rows(g, ao_frame(100, 80, shading=True, depth=3.0), sa.MODE_BVH)
            gens = int(g.ray_stats()[4]) // 100
            results[hook] = (unc, cold, g.get_ao_cache(), gens)
    finally:
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
        g.reset_ao_cache()
    a, b = results[-1], results[34]
    assert a[3] == b[3] and a[3] > 1000
    assert int(np.count_nonzero(a[0] != b[0])) == 0 and int(np.count_nonzero(a[1] != b[1])) == 0
    assert int(np.count_nonzero(a[2] != b[2])) == 0 and a[2].any()
    plain = gpu_rows(g, make_frame(100, 80, shading=True, depth=3.0), sa.MODE_BVH)
    assert np.count_nonzero(plain != a[0]) > 500                                # the probes changed the image


# ---- 2. uncached with shading, sub-pixel samples, focal blur, row blocks and row windows ----
def test_uncached_shading_subsamples_focal_blur(obj2_pair):
    g, o = obj2_pair
    check_uncached(g, o, ao_frame(90, 67, uncached=True, shading=True))
    check_uncached(g, o, ao_frame(50, 50, uncached=True, shading=True, sub_pixel_res=2))
    check_uncached(g, o, ao_frame(50, 50, uncached=True, shading=True, sub_pixel_res=2, focal_blur=True, point_light=False, specular=False))
    check_uncached(g, o, ao_frame(50, 41, uncached=True, sub_pixel_res=3), modes=("tree", "brute", "bvh"))


@pytest.mark.parametrize("concurrency", [1, 3, 4, 0])
def test_uncached_row_blocks_restart_the_sequence(obj2_pair, concurrency):
    g, o = obj2_pair
    images = [check_uncached(g, o, ao_frame(90, 67, uncached=True, concurrency=concurrency))[aom.TRACE_ROOT_TREE]]
    check_uncached(g, o, ao_frame(50, 50, uncached=True, sub_pixel_res=2, concurrency=concurrency))
    check_uncached(g, o, ao_frame(90, 67, uncached=True, concurrency=concurrency, start_row=9, end_row=60))
    if concurrency == 1:
        other = aom.AoModel().render(o, ao_frame(90, 67, uncached=True, concurrency=4))
        assert not np.array_equal(images[0], other)                            # the blocks really move the random sequence


def test_uncached_row_window_moves_the_blocks(obj2_pair):
    g, o = obj2_pair
    for a, b in ((10, 57), (0, 0), (33, 99), (-5, 20), (50, 1000)):
        check_uncached(g, o, ao_frame(100, 100, uncached=True, start_row=a, end_row=b, concurrency=3), modes=("tree",))
    full = aom.AoModel().render(o, ao_frame(100, 100, uncached=True))
    part = aom.AoModel().render(o, ao_frame(100, 100, uncached=True, start_row=10, end_row=57))
    assert not np.array_equal(full[10:58], part)                               # the window is not a crop of the full frame


# ---- 3. with dynamic shadows (one sample per pixel, point light), split pipeline and SR_F_NO_SPLIT ----
# (an AO frame always runs as ONE pipeline -- include/softray.h -- so both variants take the same route; the flag must change nothing)
@pytest.mark.parametrize("no_split", [False, True], ids=["default_flags", "with_SR_F_NO_SPLIT"])
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_with_dynamic_shadows(obj_pair, mode, no_split):
    g, o = obj_pair
    extra = sa._lib.F_NO_SPLIT if no_split else 0
    f = ao_frame(100, 80, uncached=True, shading=True, shadows=True)
    want = check_uncached(g, o, f, modes=(mode,), extra_flags=extra)[target_of(mode)]
    shadowed, _ = o.render(make_frame(100, 80, shading=True, shadows=True), threads=min(16, os.cpu_count() or 1))
    assert np.count_nonzero(shadowed.reshape(80, 100) != want) > 500
    g.reset_ao_cache()
    model = aom.AoModel()
    fc = ao_frame(100, 80, shading=True, shadows=True)
    check_cached(g, o, model, fc, mode, extra)
    assert model.generators > 1000
    check_cached(g, o, model, fc, mode, extra)
    assert model.generators == 0


def test_with_dynamic_shadows_literal_tree_and_lanes(obj2_pair):
    """The shadow stage's other routes in front of the AO stage: the literal tree's per-lane shadow kernel (compact hit queue instead
    of the shaft path's tile-indexed one) and a directional light (every sample escapes: no shadow stage at all)."""
    g, o = obj2_pair
    f = ao_frame(70, 60, uncached=True, shading=True, shadows=True)
    check_uncached(g, o, f, modes=("tree",), extra_flags=sa._lib.F_LITERAL_SECONDARY)
    check_uncached(g, o, f, modes=("bvh",), extra_flags=sa._lib.F_PER_LANE_SHADOWS)
    check_uncached(g, o, ao_frame(70, 60, uncached=True, shading=True, shadows=True, point_light=False), modes=("tree", "bvh"))


# ---- 4. the cache, in order, on one scene ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_cache_life_cycle(mode):
    g, o = pair(*load_obj3ds("obj2.3DS"))
    model = aom.AoModel()
    fa = ao_frame(100, shading=True)
    fb = ao_frame(100, shading=True, yaw_deg=100.0)
    assert not g.get_ao_cache().any()
    a1 = check_cached(g, o, model, fa, mode)                                    # frame A: cold
    gen_a = model.generators
    assert gen_a > 1000 and int(g.ray_stats()[4]) == 100 * gen_a
    a2 = check_cached(g, o, model, fa, mode)                                    # frame A again: nothing to generate
    assert np.array_equal(a1, a2) and model.generators == 0 and int(g.ray_stats()[4]) == 0
    check_cached(g, o, model, fb, mode)                                         # frame B: only its new cells
    assert 0 < model.generators and int(g.ray_stats()[4]) == 100 * model.generators
    filled_ab = int(np.count_nonzero(model.cache))
    assert filled_ab == gen_a + model.generators
    g.reset_ao_cache()                                                          # a new Renderer
    model.reset()
    assert not g.get_ao_cache().any()
    a3 = check_cached(g, o, model, fa, mode)
    assert np.array_equal(a1, a3) and model.generators == gen_a
    # a loaded cache: every cell 128 -> every hit sample is modulated with 128 and nothing is generated
    g.set_ao_cache(np.full((128, 128, 128), 128, dtype=np.uint8))
    model.cache[:] = 128
    got = check_cached(g, o, model, fa, mode)
    assert model.generators == 0 and int(g.ray_stats()[4]) == 0
    plain, _ = g.render(as_sr(make_frame(100, shading=True), MODES[mode]))
    plain = plain.reshape(100, 100)
    hit = plain != 0xFFFF00FF
    assert np.array_equal(got[hit], aom.modulate(plain, np.full(plain.shape, 128))[hit]) and np.array_equal(got[~hit], plain[~hit])
    g.load_3ds(open(os.path.join(GOLDEN, "obj2.3DS"), "rb").read())             # a new model drops the cache
    assert not g.get_ao_cache().any()


def test_cached_with_subsamples_and_blocks(obj2_pair):
    g, o = obj2_pair
    for kw in (dict(sub_pixel_res=2), dict(sub_pixel_res=2, focal_blur=True, concurrency=3), dict(sub_pixel_res=3, concurrency=1)):
        for mode in ("tree", "bvh"):
            g.reset_ao_cache()
            model = aom.AoModel()
            check_cached(g, o, model, ao_frame(50, 50, shading=True, **kw), mode)
            assert model.generators > 500
            check_cached(g, o, model, ao_frame(50, 50, shading=True, yaw_deg=150.0, **kw), mode)
    g.reset_ao_cache()
    model = aom.AoModel()
    for conc, rows in ((1, (0, 99)), (3, (20, 70)), (4, (0, 99)), (0, (5, 95))):
        check_cached(g, o, model, ao_frame(100, 100, concurrency=conc, start_row=rows[0], end_row=rows[1], yaw_deg=135.0 + 10 * conc), "tree")
    g.reset_ao_cache()


# ---- 5. statistics ----
@pytest.mark.parametrize("uncached", [True, False], ids=["uncached", "cached"])
def test_statistics(obj2_pair, uncached):
    g, o = obj2_pair
    g.reset_ao_cache()
    for mode in ("tree", "brute", "bvh"):
        g.reset_ao_cache()
        model = aom.AoModel()
        f = ao_frame(90, 67, uncached=uncached, shading=True)
        model.render(o, f, target_of(mode))
        _, st = g.render(as_sr(f, MODES[mode]))
        rs = g.ray_stats().copy()
        assert int(rs[4]) == 100 * model.generators and model.generators > 1000
        assert np.array_equal(rs[:4], st)
        if mode != "brute":
            assert rs[6] > 0 and rs[7] > 0                                      # the probes' walks are counted
        assert rs[5] > 0
        _, st0 = g.render(as_sr(make_frame(90, 67, shading=True), MODES[mode]))
        assert np.array_equal(st0, st) and int(g.ray_stats()[4]) == 0           # [0..3] are those of the frame without AO
        g.reset_ao_cache()
        fp = as_sr(f, MODES[mode])
        fp.flags |= sa._lib.F_PRIMARY_STATS_ONLY
        _, st1 = g.render(fp)
        assert np.array_equal(st1, st) and not g.ray_stats()[4:8].any()
    g.reset_ao_cache()


# ---- 6. extra geometry outside the unit cube: the clamp ----
@pytest.mark.parametrize("mode", ["tree", "brute"])
def test_extra_geometry_outside_the_cube(primitives_pair, mode):
    g, o = primitives_pair
    f = ao_frame(100, 80, uncached=True, shading=True, depth=3.0)
    s, d = ptm.camera_samples(f)
    first = o.trace(aom.TRACE_ROOT_TREE, s, d)
    outside = (np.abs(first["pos"][first["hit"] > 0]) > 0.5).any(axis=1)
    assert outside.sum() > 1000                                                 # the clamp is exercised
    check_uncached(g, o, f, modes=(mode,))
    g.reset_ao_cache()
    model = aom.AoModel()
    fc = ao_frame(100, 80, shading=True, depth=3.0)
    check_cached(g, o, model, fc, mode)
    check_cached(g, o, model, ao_frame(100, 80, shading=True, depth=3.0, yaw_deg=160.0), mode)
    g.reset_ao_cache()


def test_sphere_only_scene():
    """No triangle is ever hit: the model is one far-away sliver, the picture is the spheres (rayFrac in distance units)."""
    v9 = np.array([[(0.49, 0.49, 0.49), (0.5, 0.49, 0.49), (0.49, 0.5, 0.49)]])
    g, o = pair(v9, np.array([0xFFFFFFFF], dtype=np.uint32), np.array([-0.5] * 3), np.array([0.5] * 3), prims=c1_spheres(), modes=(sa.MODE_REF_TREE,))
    for mode in ("tree", "brute"):
        check_uncached(g, o, ao_frame(100, 80, uncached=True, shading=True, depth=2.0), modes=(mode,))
        model = aom.AoModel()
        g.reset_ao_cache()
        check_cached(g, o, model, ao_frame(100, 80, shading=True, depth=2.0, sub_pixel_res=1), mode)
        assert model.generators > 500


# ---- 7. a frame in which every sample misses ----
@pytest.mark.parametrize("uncached", [True, False], ids=["uncached", "cached"])
def test_all_samples_miss(obj2_pair, uncached):
    g, o = obj2_pair
    g.reset_ao_cache()
    for conc in (4, 2 ** 31 - 1):
        for n in (1, 2):
            f = ao_frame(40, 30, uncached=uncached, shading=True, depth=-5.0, concurrency=conc, sub_pixel_res=n)    # the model is behind the camera
            assert not o.trace(aom.TRACE_ROOT_TREE, *ptm.camera_samples(f))["hit"].any()
            for mode in MODES.values():
                got = gpu_rows(g, f, mode)
                assert np.all(got == 0xFFFF00FF)
                assert int(g.ray_stats()[4]) == 0
    assert not g.get_ao_cache().any()


# ---- 8. refused combinations; a multi-device scene ----
def test_refused_combinations_leave_the_cache_alone(obj2_pair):
    g, o = obj2_pair
    g.reset_ao_cache()
    model = aom.AoModel()
    check_cached(g, o, model, ao_frame(60, 50), "tree")
    before = g.get_ao_cache()
    assert before.any()
    out = np.zeros(60 * 50, dtype=np.uint32)
    for change in (dict(flags=sa.F_PATH_TRACING), dict(flags=sa.F_VOXELS), dict(flags=sa.F_SHADOWS | sa.F_STATIC_SHADOWS), dict(max_bounces=1),
                   dict(flags=sa._lib.F_SINGLE_KERNEL), dict(strips=(16, 2, 0))):
        for uncached in (False, True):
            f = as_sr(ao_frame(60, 50, uncached=uncached, yaw_deg=90.0), sa.MODE_REF_TREE)
            f.flags |= change.get("flags", 0)
            f.max_bounces = change.get("max_bounces", 0)
            if "strips" in change:
                f.strip_rows, f.strip_count, f.strip_index = change["strips"]
            with pytest.raises(sa.SoftrayError) as e:
                g.render(f, out=out)
            assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED and "ambient occlusion" in str(e.value), change
    # a row range that does not fit one row band (test hook: tiny bands)
    try:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, 16 * 64)
        with pytest.raises(sa.SoftrayError) as e:
            g.render(as_sr(ao_frame(60, 50, yaw_deg=90.0), sa.MODE_REF_TREE), out=out)
        assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED and "one row band" in str(e.value)
    finally:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, -1)
    assert np.array_equal(g.get_ao_cache(), before)
    # the draw table's limit (test hook: 1200 bytes = one generator): refused once the generators are known, nothing stored, and the
    # scene renders again afterwards -- with and without kernel timing (the stage's event pair)
    try:
        g.debug_set(sa._lib.DBG_AO_TABLE_BYTES, 1200)
        for timing in (-1, 1):
            g.debug_set(sa._lib.DBG_KERNEL_TIMING, timing)
            for uncached in (False, True):
                with pytest.raises(sa.SoftrayError) as e:
                    g.render(as_sr(ao_frame(60, 50, uncached=uncached, yaw_deg=90.0), sa.MODE_REF_TREE), out=out)
                assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED and "random table" in str(e.value)
                assert np.array_equal(g.get_ao_cache(), before)
        g.kernel_times()
    finally:
        g.debug_set(sa._lib.DBG_AO_TABLE_BYTES, -1)
        g.debug_set(sa._lib.DBG_KERNEL_TIMING, -1)
    check_cached(g, o, model, ao_frame(60, 50, yaw_deg=90.0), "tree")           # the limit back to its default: the same frame renders
    assert model.generators > 0
    g.reset_ao_cache()


def test_rccl_render_refuses_ambient_occlusion(obj2_pair):
    """sr_rccl_render refuses an AO frame in its own right, before it makes strips of it: a one-rank communicator on one GPU."""
    import torch
    o = obj2_pair[1]
    g = pair(*load_obj3ds("obj2.3DS"))[0]
    g.rccl_init(sa.rccl_unique_id(), 1, 0)
    model = aom.AoModel()
    check_cached(g, o, model, ao_frame(60, 50), "tree")
    before = g.get_ao_cache()
    assert before.any()
    surface = torch.zeros(60 * 50, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for uncached in (False, True):
        with pytest.raises(sa.SoftrayError) as e:
            g.rccl_render(as_sr(ao_frame(60, 50, uncached=uncached, yaw_deg=90.0), sa.MODE_REF_TREE), surface.data_ptr(), stream)
        assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED and "ambient occlusion" in str(e.value) and "sr_rccl_render" in str(e.value)
    torch.cuda.synchronize()
    assert not surface.any().item() and np.array_equal(g.get_ao_cache(), before)
    g.rccl_render(as_sr(make_frame(60, 50), sa.MODE_REF_TREE), surface.data_ptr(), stream)     # other frames go through
    torch.cuda.synchronize()
    assert surface.any().item()


def test_multi_device_scene_renders_on_the_first_device(obj2_pair):
    g1, o = obj2_pair
    gm = pair(*load_obj3ds("obj2.3DS"), devices=[0, 0])[0]
    for uncached in (True, False):
        f = ao_frame(100, 90, uncached=uncached, shading=True)
        g1.reset_ao_cache()
        want = gpu_rows(g1, f, sa.MODE_REF_TREE)
        got = gpu_rows(gm, f, sa.MODE_REF_TREE)
        assert gm.last_frame_parts() == 1 and np.array_equal(got, want)
        assert np.array_equal(gm.ray_stats(), g1.ray_stats())
        assert int(np.count_nonzero(want != aom.AoModel().render(o, f))) == 0
    assert np.array_equal(gm.get_ao_cache(), g1.get_ao_cache()) and gm.get_ao_cache().any()
    gm.reset_ao_cache()
    assert not gm.get_ao_cache().any()
    gpu_rows(gm, make_frame(100, 90), sa.MODE_REF_TREE)
    assert gm.last_frame_parts() == 2                                           # other frames are split as before
    g1.reset_ao_cache()


# ---- 9. scene state ----
def test_repeated_uncached_frames_are_identical(obj_pair):
    g, _ = obj_pair
    f = ao_frame(96, 80, uncached=True, shading=True, shadows=True)
    for mode in ("tree", "bvh"):
        a = gpu_rows(g, f, MODES[mode])
        assert np.array_equal(a, gpu_rows(g, f, MODES[mode])) and np.array_equal(a, gpu_rows(g, f, MODES[mode]))


def test_other_frames_are_unchanged_by_an_ao_frame(obj2_pair):
    g, _ = obj2_pair
    g.reset_ao_cache()
    g.reset_shadow_cache()
    path = make_frame(80, 70, shading=False)
    path.flags |= ptm.F_PATH_TRACING
    others = [make_frame(80, 70), make_frame(80, 70, shadows=True), make_frame(50, 50, shadows=True, sub_pixel_res=2), path]
    static = make_frame(80, 70, shadows=True, static_shadows=True)
    for mode in (sa.MODE_REF_TREE, sa.MODE_BVH):
        before = [gpu_rows(g, f, mode) for f in others]
        g.reset_shadow_cache()
        static_before = [gpu_rows(g, static, mode), gpu_rows(g, static, mode)]     # cold, then warm
        for f in (ao_frame(80, 70, shading=True), ao_frame(80, 70, uncached=True, shadows=True, shading=True), ao_frame(50, 50, sub_pixel_res=2)):
            gpu_rows(g, f, mode)
        assert np.array_equal(gpu_rows(g, static, mode), static_before[1])          # the shadow cache was not touched
        for f, want in zip(others, before):
            assert np.array_equal(gpu_rows(g, f, mode), want)
        g.reset_shadow_cache()
        assert np.array_equal(gpu_rows(g, static, mode), static_before[0])
    g.reset_ao_cache()
    g.reset_shadow_cache()


# ---- 10. the C++ mirror ----
def test_cpp_mirror_matches_the_model(tmp_path, obj2_pair):
    o = obj2_pair[1]
    exe = str(tmp_path / "ao_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "ao_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    want = [aom.AoModel().render(o, ao_frame(100, uncached=True, shading=True)), aom.AoModel().render(o, ao_frame(100, shading=True))]
    expected = tmp_path / "expected.bin"
    np.concatenate([w.reshape(-1) for w in want]).astype(np.uint32).tofile(str(expected))
    r = subprocess.run([exe, GOLDEN, str(expected)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL OK" in r.stdout
    assert r.stdout.count("diff=0") == 4 and r.stdout.count("refused ok") == 4
