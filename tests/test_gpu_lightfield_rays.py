"""sr_light_field_rays on the device -- LightFieldColorMethod.IntersectRay for rays the caller supplies -- against the CPU model
(tests/lightfield_rays_model.py), against light-field frames and against the reference's goldens, bit for bit: every comparison is an exact
equality over every ray, every pixel and every table entry.  The ray sets are lightfield_rays_model's after its `usable` filter (the input
condition of the light-field tests; tests/test_lightfield_rays_model.py caps what it removes), the camera sets are frames of
lightfield_model.GPU_FRAMES.  (Extra geometry runs in tree mode: the oracle's nearest-hit target, the reference of SR_MODE_BVH, has none.)"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lightfield_interp_model as lim
import lightfield_model as lfm
import lightfield_rays_model as lrm
import lightfield_shadow_model as lsm
import pathtrace_model as ptm
import softray_amd as sa
from helpers import GOLDEN, load_obj3ds, make_frame, orc, read_bmp_rgb

pytestmark = pytest.mark.gpu
L = sa._lib
DEV = torch.device("cuda", 0)
MODES = {"tree": sa.MODE_REF_TREE, "brute": sa.MODE_BRUTE, "bvh": sa.MODE_BVH}
UNTOUCHED = 0x01020304
GUARD = 0x0BADBEEF


def target_of(mode):
    return lfm.TRACE_NEAREST if mode == "bvh" else lfm.TRACE_ROOT_TREE


def as_sr(frame, mode, extra_flags=0):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = MODES[mode]
    f.flags |= extra_flags
    return f


def pose_frame(shading=True, **kw):
    """A frame for its pose, lights and switches: the camera fields are validated and otherwise unused."""
    return make_frame(16, 16, shading=shading, yaw_deg=100.0, pitch_deg=-15.0, **kw)


_pairs = {}


def pair(model="obj.3ds", prims=(), devices=None):
    key = (model, bool(prims), tuple(devices or ()))
    if key not in _pairs:
        g, o = (sa.GpuScene(devices=devices) if devices else sa.GpuScene(0)), orc.Scene()
        for s in (g, o):
            s.set_triangles(*load_obj3ds(model))
            if prims:
                s.set_extra(list(prims))
        g.build((sa.MODE_REF_TREE, sa.MODE_BVH))
        assert o.build_tree() == 0
        _pairs[key] = (g, o)
    g, o = _pairs[key]
    g.light_field_interpolation = False
    g.light_field_shadows = False
    g.light_field_triangles = False
    return g, o


_sets = {}


def ray_set(name):
    """(starts, dirs) of a set after the filter, made once, read-only."""
    if name not in _sets:
        starts, dirs = getattr(lrm, name)()
        s, d, removed = lrm.usable(starts, dirs, lrm.RESOLUTIONS)
        assert removed <= 0.01 * starts.shape[0]
        s.setflags(write=False)
        d.setflags(write=False)
        _sets[name] = (s, d)
    return _sets[name]


def start(g, n, table=lfm.LightFieldModel):
    """The scene as a new Renderer with resolution n has it, and a model to match."""
    g.light_field_res = n
    g.reset_light_field()
    return lrm.LightFieldRaysModel(table(n))


def same_cache(g, table):
    got = g.get_light_field()
    assert got.size == lfm.cache_entries(table.n)
    filled = np.flatnonzero(got)
    want = np.array(sorted(table.cache), dtype=np.int64)
    return filled.size == want.size and np.array_equal(filled, want) and np.array_equal(got[filled], table.entries(want))


def walks(o, model, target):
    """What the oracle counts on the canonical rays the model's last call traced: (tests, node visits, leaf visits)."""
    u, v, s, t = lfm.decode(model.filled, model.n)
    a = model.table.points[u, v]
    d = model.table.points[s, t] - a
    real = ~np.isnan(a.sum(axis=1) + d.sum(axis=1))
    if not real.any():
        return [0, 0, 0]
    res = o.trace(target, np.ascontiguousarray(a[real]), np.ascontiguousarray(d[real]), counters=True)
    return [int(x) for x in res["counters"].sum(axis=0)]


def check(g, o, model, frame, mode, starts, dirs, whole_cache=True, shadowed=False, pinned_walks=False):
    """One call on the scene's and the model's running tables: colours, inside, filled, the statistics and the whole table."""
    want, want_inside, want_filled = model.rays(o, frame, starts, dirs, target_of(mode))
    out, inside, filled = g.light_field_rays(as_sr(frame, mode), starts, dirs)
    diff = int(np.count_nonzero(out != want))
    print("%d rays, %d inside, %d colours differ, filled %d (model %d)" % (want.size, int(want_inside.sum()), diff, filled, want_filled))
    assert diff == 0 and np.array_equal(inside, want_inside) and filled == want_filled
    rs = [int(x) for x in g.ray_stats()]
    assert rs[:4] == [want.size, 0, 0, 0]
    if shadowed:
        assert rs[4] >= model.traced()                                          # the canonical rays + what the shadow stage counts
    else:
        assert rs[4] == model.traced()
        if pinned_walks:
            assert rs[5:8] == walks(o, model, target_of(mode))
    if model.traced() == 0:
        assert rs[4:8] == [0, 0, 0, 0]
    else:
        assert rs[5] > 0
    if whole_cache:
        assert same_cache(g, model.table)
    return out


# ---- 1. the model ----
@pytest.mark.parametrize("mode", ["tree", "brute", "bvh"])
@pytest.mark.parametrize("n", [2, 4, 16])
@pytest.mark.parametrize("name", ["segments", "panorama", "irregular"])
def test_model_equality(name, n, mode):
    g, o = pair()
    starts, dirs = ray_set(name)
    for shading in (True, False):
        model = start(g, n)
        f = lfm.lf_frame(pose_frame(shading))
        first = check(g, o, model, f, mode, starts, dirs, pinned_walks=mode == "tree")
        if name != "irregular":
            assert model.filled.size >= 7
        again = check(g, o, model, f, mode, starts, dirs)                        # the table is warm: nothing is filled, the same colours
        assert model.filled.size == 0 and np.array_equal(first, again)


@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_resolution_one(mode):
    g, o = pair()
    starts, dirs = ray_set("segments")
    model = start(g, 1)
    f = lfm.lf_frame(pose_frame())
    out = check(g, o, model, f, mode, starts, dirs)
    assert model.filled.tolist() == [0] and model.traced() == 0                  # one cell, whose canonical ray is NaN
    assert np.all(out == model.background(f))
    assert g.get_light_field().tolist() == [model.background(f), 0, 0, 0]


@pytest.mark.parametrize("mode", ["tree", "brute"])
def test_extra_geometry(mode):
    g, o = pair("obj.3ds", prims=ptm.PRIMITIVES)
    starts, dirs = ray_set("segments")
    model = start(g, 4)
    f = lfm.lf_frame(pose_frame())
    check(g, o, model, f, mode, starts, dirs)
    plain = lrm.LightFieldRaysModel(lfm.LightFieldModel(4))
    plain.rays(pair()[1], f, starts, dirs)
    assert plain.table.cache != model.table.cache                               # the canonical rays see the spheres


def test_resolution_64_one_ray_per_cell():
    g, o = pair()
    starts, dirs = ray_set("segments")
    model = start(g, 64)
    f = lfm.lf_frame(pose_frame())
    check(g, o, model, f, "bvh", starts, dirs, whole_cache=False)
    assert model.filled.size == 10219 == model.touched.size
    table = g.get_light_field()
    assert np.array_equal(table[model.touched], model.table.entries(model.touched)) and int(np.count_nonzero(table)) == 10219
    g.reset_light_field()


def test_resolution_128_entries_beyond_2_to_the_29():
    g, o = pair()
    n, f, starts, dirs = lrm.camera("res128_high")
    starts, dirs, removed = lrm.usable(starts, dirs, (n,))
    assert removed == 0
    model = start(g, n)
    try:
        check(g, o, model, f, "tree", starts, dirs, whole_cache=False)
        assert model.filled.size > 1000 and int(model.filled.max()) > 2 ** 29    # byte offsets beyond 2^31
        got = np.array([int(g.get_light_field(int(i), 1)[0]) for i in model.filled], dtype=np.uint32)
        assert np.array_equal(got, model.table.entries(model.filled))
        check(g, o, model, f, "tree", starts, dirs, whole_cache=False)
        assert model.filled.size == 0
    finally:
        g.light_field_res = 64                                                   # (drops the 4 GiB)


# ---- 2. frames ----
def gpu_rows(g, frame, mode):
    f = as_sr(frame, mode)
    out = np.full(f.width * f.height, UNTOUCHED, dtype=np.uint32)
    g.render(f, out=out)
    a = min(max(0, f.start_row), f.height - 1)
    b = min(max(0, f.end_row), f.height - 1)
    return out.reshape(f.height, f.width)[a:b + 1].copy()


@pytest.mark.parametrize("name", ["contention", "small_blur", "far_primitives", "view0_n64"])
def test_camera_rays_give_the_frame_and_its_table(name):
    model_file, prims, n, f = lfm.gpu_frame(name)
    g, _ = pair(model_file, prims)
    _, _, starts, dirs = lrm.camera(name)
    g.light_field_res = n
    g.reset_light_field()
    col, _, filled = g.light_field_rays(as_sr(f, "tree"), starts, dirs)
    table = g.get_light_field()
    g.reset_light_field()
    want = gpu_rows(g, f, "tree")
    got = lrm.resolve(col, f)
    assert got.shape == want.shape and int(np.count_nonzero(got != want)) == 0
    assert np.array_equal(g.get_light_field(), table) and filled == int(np.count_nonzero(table)) > 0
    g.reset_light_field()


@pytest.mark.parametrize("name", ["noShading_lightFieldColor", "shading_lightFieldColor_focalBlurx4"])
def test_goldens(name):
    g, _ = pair()
    n, f, starts, dirs = lrm.camera(name)
    g.light_field_res = n
    g.reset_light_field()
    col, _, _ = g.light_field_rays(as_sr(f, "bvh"), starts, dirs)
    want = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))
    assert int(np.count_nonzero((lrm.resolve(col, f) & 0xFFFFFF) != want)) == 0
    g.reset_light_field()


# ---- 3. state ----
def test_split_batch_repeat_and_bake():
    g, o = pair()
    starts, dirs = ray_set("segments")
    n, cut = 4, 7333
    f = lfm.lf_frame(pose_frame())
    sf = as_sr(f, "bvh")
    g.light_field_res = n
    g.reset_light_field()
    whole, inside, filled = g.light_field_rays(sf, starts, dirs)
    table = g.get_light_field()
    assert filled == 441
    again, _, filled_again = g.light_field_rays(sf, starts, dirs)               # the same call again
    assert np.array_equal(again, whole) and filled_again == 0 and not g.ray_stats()[4:8].any()
    g.reset_light_field()
    a, ia, fa = g.light_field_rays(sf, starts[:cut], dirs[:cut])
    b, ib, fb = g.light_field_rays(sf, starts[cut:], dirs[cut:])
    assert np.array_equal(np.concatenate([a, b]), whole) and np.array_equal(np.concatenate([ia, ib]), inside)
    assert fa + fb == filled and fa > fb and np.array_equal(g.get_light_field(), table)
    g.reset_light_field()
    assert g.bake_light_field(sf) == lfm.cache_entries(n)                        # after a bake nothing is left to fill
    baked, _, filled_baked = g.light_field_rays(sf, starts, dirs)
    assert np.array_equal(baked, whole) and filled_baked == 0
    g.reset_light_field()


def test_a_call_and_a_frame_in_either_order():
    model_file, prims, n, f = lfm.gpu_frame("view0_n8")
    g, _ = pair()
    starts, dirs = ray_set("panorama")
    sf = as_sr(f, "bvh")
    g.light_field_res = n
    results = []
    for call_first in (True, False):
        g.reset_light_field()
        if call_first:
            col, _, filled = g.light_field_rays(sf, starts, dirs)
            px = gpu_rows(g, f, "bvh")
        else:
            px = gpu_rows(g, f, "bvh")
            col, _, filled = g.light_field_rays(sf, starts, dirs)
        results.append((col, px, g.get_light_field(), filled))
    assert all(np.array_equal(x, y) for x, y in zip(results[0][:3], results[1][:3]))
    assert results[0][3] >= results[1][3] > 0                                    # (the frame may have filled some of the panorama's cells)
    g.reset_light_field()


# ---- 4. shapes ----
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_batch_sizes(count):
    g, o = pair()
    starts, dirs = ray_set("segments")
    model = start(g, 4)
    check(g, o, model, lfm.lf_frame(pose_frame()), "bvh", starts[100:100 + count], dirs[100:100 + count])


@pytest.mark.parametrize("interpolate", [False, True], ids=["nearest", "interpolated"])
def test_small_passes_read_what_earlier_passes_filled(interpolate):
    g, _ = pair()
    starts, dirs = ray_set("segments")
    sf = as_sr(lfm.lf_frame(pose_frame()), "bvh")
    g.light_field_res = 4
    g.light_field_interpolation = interpolate
    g.reset_light_field()
    want, want_inside, want_filled = g.light_field_rays(sf, starts, dirs)
    table = g.get_light_field()
    g.reset_light_field()
    try:
        g.debug_set(L.DBG_BAND_SAMPLES, 1000)                                    # 20 passes
        got, inside, filled = g.light_field_rays(sf, starts, dirs)
    finally:
        g.debug_set(L.DBG_BAND_SAMPLES, -1)
    assert np.array_equal(got, want) and np.array_equal(inside, want_inside) and filled == want_filled
    assert np.array_equal(g.get_light_field(), table)
    g.reset_light_field()


# ---- 5. interpolation ----
def check_interpolated(g, o, model, frame, mode, starts, dirs, coords, inside, shadowed=False):
    want, want_filled = model.rays_interpolated(o, frame, coords, inside, target_of(mode))
    out, got_inside, filled = g.light_field_rays(as_sr(frame, mode), starts, dirs)
    diff = int(np.count_nonzero(out != want))
    print("%d rays, %d colours differ, %d cells read, filled %d (model %d)" % (want.size, diff, model.touched.size, filled, want_filled))
    assert diff == 0 and np.array_equal(got_inside, inside) and filled == want_filled
    rs = [int(x) for x in g.ray_stats()]
    assert rs[:4] == [want.size, 0, 0, 0] and (rs[4] >= model.traced() if shadowed else rs[4] == model.traced())
    assert same_cache(g, model.table)
    return out


@pytest.mark.parametrize("mode", ["tree", "bvh"])
@pytest.mark.parametrize("name,n", [("segments", 4), ("panorama", 2), ("segments", 16), ("irregular", 4)])
def test_interpolation_cold_and_warm(name, n, mode):
    g, o = pair()
    starts, dirs = ray_set(name)
    model = start(g, n)
    coords, inside = g.light_field_coords(starts, dirs)
    if name != "irregular":
        assert min(lim.wrap_counts(coords, inside.astype(bool), n)) > 0          # the set wraps on every axis
    g.light_field_interpolation = True
    f = lfm.lf_frame(pose_frame())
    cold = check_interpolated(g, o, model, f, mode, starts, dirs, coords, inside)
    assert model.filled.size > 0
    warm = check_interpolated(g, o, model, f, mode, starts, dirs, coords, inside)
    assert model.filled.size == 0 and np.array_equal(cold, warm) and not g.ray_stats()[4:8].any()
    g.light_field_interpolation = False
    g.reset_light_field()


# ---- 6. shadows ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
@pytest.mark.parametrize("interpolate", [False, True], ids=["nearest", "interpolated"])
def test_shadowed_table(interpolate, mode):
    g, o = pair()
    starts, dirs = ray_set("panorama")
    n = 4
    f = lsm.shadow_frame(lfm.lf_frame(pose_frame(shadow_samples=17)))
    with pytest.raises(sa.SoftrayError) as e:                                    # the scene's switch is off
        g.light_field_rays(as_sr(f, mode), starts, dirs)
    assert e.value.code == L.SR_ERR_UNSUPPORTED
    g.light_field_shadows = True
    model = start(g, n, lsm.LightFieldShadowModel)
    if interpolate:
        coords, inside = g.light_field_coords(starts, dirs)
        g.light_field_interpolation = True
        check_interpolated(g, o, model, f, mode, starts, dirs, coords, inside, shadowed=True)
    else:
        check(g, o, model, f, mode, starts, dirs, shadowed=True)
    plain = lrm.LightFieldRaysModel(lfm.LightFieldModel(n))
    plain.rays(o, f, starts, dirs, target_of(mode))
    assert plain.table.cache != model.table.cache and model.filled.size >= 72    # some canonical rays end in shadow
    g.reset_light_field()


# ---- 7. the device variant ----
def run_device(g, sf, starts, dirs, stream, want_inside=True):
    n = starts.shape[0]
    d_starts, d_dirs = torch.from_numpy(np.array(starts)).to(DEV), torch.from_numpy(np.array(dirs)).to(DEV)
    d_out = torch.full((64 + n + 64,), GUARD, dtype=torch.int32, device=DEV)
    d_inside = torch.full((64 + n + 64,), 9, dtype=torch.uint8, device=DEV)
    d_filled = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    d_stats = torch.full((24,), -1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize(DEV)
    g.light_field_rays_device(sf, n, d_starts.data_ptr(), d_dirs.data_ptr(), d_out.data_ptr() + 64 * 4, d_inside.data_ptr() + 64 if want_inside else 0,
                              stream=stream, d_filled_ptr=d_filled.data_ptr() + 8, d_stats_ptr=d_stats.data_ptr())
    stream.synchronize()
    torch.cuda.synchronize(DEV)
    raw, ins, fl = d_out.cpu().numpy().view(np.uint32), d_inside.cpu().numpy(), d_filled.cpu().numpy()
    assert np.all(raw[:64] == GUARD) and np.all(raw[-64:] == GUARD) and np.all(ins[:64] == 9) and np.all(ins[-64:] == 9)
    assert fl[0] == -1 and fl[2] == -1
    assert np.array_equal(d_starts.cpu().numpy().view(np.uint64), starts.view(np.uint64))
    assert np.array_equal(d_dirs.cpu().numpy().view(np.uint64), dirs.view(np.uint64))
    return raw[64:-64].copy(), ins[64:-64].copy(), int(fl[1]), d_stats.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("interpolate", [False, True], ids=["nearest", "interpolated"])
def test_device_variant_on_a_stream(interpolate):
    g, _ = pair()
    starts, dirs = ray_set("segments")
    sf = as_sr(lfm.lf_frame(pose_frame()), "bvh")
    g.light_field_res = 4
    g.light_field_interpolation = interpolate
    st = torch.cuda.Stream(DEV)
    for warm in (False, True):
        if not warm:
            g.reset_light_field()
        want, want_inside, want_filled = g.light_field_rays(sf, starts, dirs)
        want_stats = g.ray_stats().copy()
        table = g.get_light_field()
        if not warm:
            g.reset_light_field()
        got, inside, filled, stats = run_device(g, sf, starts, dirs, st)
        assert np.array_equal(got, want) and np.array_equal(inside, want_inside) and filled == want_filled
        assert np.array_equal(stats, want_stats) and stats[0] == starts.shape[0]
        assert np.array_equal(g.get_light_field(), table)
        assert (filled == 0) == warm
    got, inside, _, _ = run_device(g, sf, starts, dirs, st, want_inside=False)
    assert np.array_equal(got, want) and np.all(inside == 9)                     # d_inside may be NULL
    g.light_field_interpolation = False
    g.reset_light_field()


def test_a_frame_and_a_call_on_two_streams_keep_their_order():
    model_file, prims, n, f = lfm.gpu_frame("view0_n8")
    g, _ = pair()
    starts, dirs = ray_set("panorama")
    sf = as_sr(f, "bvh")
    g.light_field_res = n
    g.reset_light_field()
    want_px = gpu_rows(g, f, "bvh").reshape(-1)
    want, _, want_filled = g.light_field_rays(sf, starts, dirs)                  # after the frame: it fills what the frame left empty
    table = g.get_light_field()
    d_starts, d_dirs = torch.from_numpy(np.array(starts)).to(DEV), torch.from_numpy(np.array(dirs)).to(DEV)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    for _ in range(2):
        g.reset_light_field()
        d_out = torch.full((starts.shape[0],), GUARD, dtype=torch.int32, device=DEV)
        d_filled = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        px = torch.zeros(f.width * f.height, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize(DEV)
        g.render_device(sf, px.data_ptr(), s1.cuda_stream)
        g.light_field_rays_device(sf, starts.shape[0], d_starts.data_ptr(), d_dirs.data_ptr(), d_out.data_ptr(), stream=s2, d_filled_ptr=d_filled.data_ptr())
        torch.cuda.synchronize(DEV)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want) and int(d_filled.cpu()[0]) == want_filled
        assert np.array_equal(px.cpu().numpy().view(np.uint32), want_px)
        assert np.array_equal(g.get_light_field(), table)
    g.reset_light_field()


# ---- 8. refusals and forwarding ----
def raw_call(g, f, n, starts, dirs, out, inside, options):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)          # noqa: E731
    made = C.c_uint64(77)
    rc = L.lib().sr_light_field_rays(g._h, C.byref(f) if f is not None else None, n, p(starts), p(dirs), p(out), p(inside), options, C.byref(made))
    return rc, (L.lib().sr_last_error().decode() if rc else ""), made.value


def test_refusals_leave_everything_untouched():
    cpu = lrm
    g, o = pair()
    starts, dirs = (np.array(a[:64]) for a in ray_set("segments"))
    model = start(g, 4)
    good = as_sr(lfm.lf_frame(pose_frame()), "tree")
    check(g, o, model, good, "tree", starts, dirs)
    before = g.get_light_field()
    out = np.full(64, UNTOUCHED, dtype=np.uint32)
    inside = np.full(64, 9, dtype=np.uint8)
    cases = [((good, -1, starts, dirs, out, inside, 0), L.SR_ERR_INVALID_ARG, "bad argument to sr_light_field_rays"),
             ((good, 64, None, dirs, out, inside, 0), L.SR_ERR_INVALID_ARG, "bad argument to sr_light_field_rays"),
             ((good, 64, starts, dirs, None, inside, 0), L.SR_ERR_INVALID_ARG, "bad argument to sr_light_field_rays"),
             ((good, 64, starts, dirs, out, inside, 1), L.SR_ERR_INVALID_ARG, "bad argument to sr_light_field_rays"),
             ((None, 64, starts, dirs, out, inside, 0), L.SR_ERR_INVALID_ARG, "bad argument to sr_light_field_rays")]
    for kw, text in cpu.MESSAGES:
        cases.append(((cpu.changed(good, **kw), 64, starts, dirs, out, inside, 0), L.SR_ERR_UNSUPPORTED, text))
    cases.append(((cpu.changed(good, flags=L.F_SHADOWS), 64, starts, dirs, out, inside, 0), L.SR_ERR_UNSUPPORTED, cpu.SHADOWS_MESSAGE))
    cases.append(((cpu.changed(good, trace_mode=7), 64, starts, dirs, out, inside, 0), L.SR_ERR_INVALID_ARG, None))
    for args, code, text in cases:
        rc, msg, made = raw_call(g, *args)
        assert rc == code and (text is None or msg == text), (rc, msg)
        assert made == 77
    g.light_field_triangles = True
    rc, msg, _ = raw_call(g, good, 64, starts, dirs, out, inside, 0)
    assert rc == L.SR_ERR_UNSUPPORTED and msg == cpu.TRIANGLES_MESSAGE
    g.light_field_triangles = False
    unbuilt = sa.GpuScene(0)
    unbuilt.set_triangles(*load_obj3ds("obj.3ds"))
    assert raw_call(unbuilt, good, 64, starts, dirs, out, inside, 0)[0] == L.SR_ERR_NOT_BUILT
    assert np.all(out == UNTOUCHED) and np.all(inside == 9)
    assert np.array_equal(g.get_light_field(), before)
    rc, _, made = raw_call(g, good, 0, None, None, None, None, 0)              # an empty batch: nothing is touched, *filled = 0
    assert rc == L.SR_OK and made == 0 and np.array_equal(g.get_light_field(), before)
    check(g, o, model, good, "tree", starts, dirs)                              # and the scene works as before
    assert model.filled.size == 0


def test_multi_device_scene_answers_like_a_single_one():
    g1, o = pair()
    g, _ = pair(devices=[0, 0])
    assert g.device_count() == 2
    starts, dirs = ray_set("segments")
    f = lfm.lf_frame(pose_frame())
    for interpolate in (False, True):
        for s in (g1, g):
            s.light_field_res = 4
            s.light_field_interpolation = interpolate
            s.reset_light_field()
        want = g1.light_field_rays(as_sr(f, "bvh"), starts, dirs)
        got = g.light_field_rays(as_sr(f, "bvh"), starts, dirs)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] > 0
        assert np.array_equal(g.get_light_field(), g1.get_light_field())
        assert np.array_equal(g.ray_stats(), g1.ray_stats())                    # the first part's, reported by the multi-device scene
    for s in (g1, g):
        s.light_field_interpolation = False
        s.reset_light_field()
