"""Any-hit ray batches with a distance limit (sr_occluded_rays) on the GPU.  Every comparison is an exact equality over every ray: the call
against sr_trace_rays of the same rays plus hit & (ray_frac <= limit), for regular rays against the oracle's model, the schedules against
each other, passes against one pass, the device variant against the host variant, the decorator's count against sr_shadow_points, and
frames around the call against themselves.  Scenes, ray sets and limits: tests/occluded_rays_cases.py (their occluded counts are checked on
the CPU in tests/test_occluded_rays_model.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ao_model
import gbuffer_cases as gbc
import mesh_cases as mc
import occluded_rays_cases as occ
import shadow_points_model as spm
import softray_amd as sa
from helpers import edge_light_frame, make_frame, orc, unit_cube_scene

pytestmark = pytest.mark.gpu
L = sa._lib
DEV = torch.device("cuda", 0)
MODES = {"tree": sa.MODE_REF_TREE, "brute": sa.MODE_BRUTE, "bvh": sa.MODE_BVH}
GUARD = 0x5A
EDGE = gbc.EDGE


class Scene:
    """One scene on the device (host-built and device-built own BVH) and in the oracle."""

    def __init__(self, name):
        self.name = name
        self.tris, self.prims = gbc.scene_data(name)
        self.tree, self.brute = gbc.oracle_scenes(name)
        self.gpus = {}

    def gpu(self, on_device=None, devices=None):
        key = (on_device, None if devices is None else tuple(devices))
        if key not in self.gpus:
            g = sa.GpuScene(devices=devices) if devices else sa.GpuScene(0)
            g.set_triangles(*self.tris)
            if self.prims:
                g.set_extra(list(self.prims))
            g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=on_device)
            self.gpus[key] = g
        return self.gpus[key]

    def builds(self):
        return (None,) if self.name == "small" else (False, True)       # (at most 64 triangles: the library builds on the host by itself)


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Scene(name)
        return made[name]
    return get


def call(g, target, rs, variant, **kw):
    return g.occluded(target, rs.starts, rs.dirs, limits=rs.limits[variant], endpoints=rs.endpoints, **kw)


def by_trace(g, target, rs, variant):
    """GpuScene.trace(...) plus the comparison."""
    return occ.model(g.trace(target, rs.starts, rs.D), rs.limit_array(variant))


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


# ---- 1. equals sr_trace_rays plus the comparison, and for regular rays the oracle's model ----
@pytest.mark.parametrize("scene", occ.SCENES)
def test_equals_trace_rays_and_the_oracle(scenes, scene):
    sc = scenes(scene)
    some = 0
    for name in occ.SETS:
        rs = occ.ray_set(scene, name)
        for variant in rs.limits:
            reg = rs.regular(variant)
            lim = rs.limit_array(variant)
            for mode in MODES:
                for root in (False, True):
                    target = MODES[mode] | (L.TARGET_ROOT if root else 0)
                    res = occ.oracle_trace(sc.tree, sc.brute, mode, root, sc.prims, np.ascontiguousarray(rs.starts[reg]), np.ascontiguousarray(rs.D[reg]))
                    model = None if res is None else occ.model(res, lim[reg])
                    for on_device in sc.builds():
                        g = sc.gpu(on_device)
                        got = call(g, target, rs, variant)
                        assert set(np.unique(got)) <= {0, 1}
                        assert same(got, by_trace(g, target, rs, variant)), (name, variant, mode, root, on_device)
                        if model is not None:
                            assert same(got[reg], model), (name, variant, mode, root, on_device)
                        some += int(got.sum())
    assert some > 1000


# ---- 2. the schedules agree ----
@pytest.mark.parametrize("scene", occ.SCENES)
def test_schedules_agree(scenes, scene):
    sc = scenes(scene)
    for on_device in sc.builds():
        g = sc.gpu(on_device)
        for name in ("segments", "probes", "far", "n65", "irregular", "irregular_ends"):
            rs = occ.ray_set(scene, name)
            for target in (sa.MODE_BVH, sa.MODE_BVH | L.TARGET_ROOT):
                base = call(g, target, rs, "rot")
                assert same(call(g, target, rs, "rot", coherent=True), base), (name, "coherent")
                for hook in (46, 47, 100, 124, 163):              # input order, nearest-hit walks, persistent lanes refilled at 0 / 24 / 63 busy ones
                    g.debug_set(L.DBG_KERNEL_SWITCH, hook)
                    try:
                        for coherent in (False, True):
                            assert same(call(g, target, rs, "rot", coherent=coherent), base), (name, hook, coherent)
                    finally:
                        g.debug_set(L.DBG_KERNEL_SWITCH, -1)
                assert same(call(g, target, rs, "rot"), base)


@pytest.mark.parametrize("mode", ["bvh", "tree", "brute"])
def test_four_passes_equal_one_pass(scenes, mode):
    sc = scenes("cube")
    g = sc.gpu(True)
    rs = occ.ray_set("cube", "n449")
    target = MODES[mode] | L.TARGET_ROOT
    whole, whole_stats = call(g, target, rs, "rot", stats=True)
    assert same(whole, by_trace(g, target, rs, "rot"))
    for coherent in (False, True):
        g.debug_set(L.DBG_BAND_SAMPLES, 128)
        g.reset_kernel_times()
        g.debug_set(L.DBG_KERNEL_TIMING, 1)
        try:
            banded, stats = call(g, target, rs, "rot", coherent=coherent, stats=True)
            times = g.kernel_times()
        finally:
            g.debug_set(L.DBG_BAND_SAMPLES, -1)
            g.debug_set(L.DBG_KERNEL_TIMING, -1)
        assert times["k_occluded"][1] == 4                                    # 3 x 128 + 65
        if mode == "bvh":                                                     # ... and the same four passes on persistent lanes
            g.debug_set(L.DBG_BAND_SAMPLES, 128)
            g.debug_set(L.DBG_KERNEL_SWITCH, 108)
            try:
                refilled, rstats = call(g, target, rs, "rot", coherent=coherent, stats=True)
            finally:
                g.debug_set(L.DBG_BAND_SAMPLES, -1)
                g.debug_set(L.DBG_KERNEL_SWITCH, -1)
            assert same(refilled, whole) and rstats[0] == 449
        assert ("k_occl_sort" in times) == (mode == "bvh") and (mode != "bvh" or times["k_occl_sort"][1] == 4)
        assert same(banded, whole), coherent
        assert stats[0] == 449
        if mode != "bvh":
            assert np.array_equal(stats, whole_stats)


def test_no_limits_is_a_limit_of_one(scenes):
    for scene in occ.SCENES:
        sc = scenes(scene)
        g = sc.gpu(sc.builds()[-1])
        for name in ("segments", "shadow", "irregular_ends"):
            rs = occ.ray_set(scene, name)
            ones = np.full(rs.n, 1.0)
            for mode in MODES.values():
                a = g.occluded(mode, rs.starts, rs.dirs, limits=None, endpoints=True)
                assert same(a, g.occluded(mode, rs.starts, rs.dirs, limits=ones, endpoints=True))
                # ... and end points are the directions end - start
                assert same(a, g.occluded(mode, rs.starts, rs.D, limits=ones))
                assert 0 < a.sum() < rs.n


# ---- 3. the decorator's answer: ShadowMethod's escape count from the call ----
def as_sr(frame, mode="bvh", extra_flags=0):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = MODES[mode]
    f.flags |= extra_flags
    return f


def test_escape_counts_reproduce_sr_shadow_points(scenes):
    sc = scenes("cube")
    S = 3
    table = np.ascontiguousarray(orc.area_light_offsets(24680, S) * np.array([1.5, 0.75, 1.0]))
    f = orc.Frame.from_buffer_copy(bytes(edge_light_frame(EDGE, 48, 40)))
    f.shadow_samples = S
    f.area_light_offsets = table.ctypes.data
    assert f.flags & orc.F_POINT_LIGHT
    for on_device in sc.builds():
        g = sc.gpu(on_device)
        hits = g.render_hits(as_sr(f))
        idx = np.flatnonzero(hits["hit"])[:1500]
        pos, nrm = np.ascontiguousarray(hits["pos"][idx]), np.ascontiguousarray(hits["normal"][idx])
        n = pos.shape[0]
        assert n > 300
        end = spm.probe_ends(pos, nrm)
        src, dirs = spm.sample_rays(f, end)                                   # [n, S, 3]: the light's samples, end - sample
        ends = np.ascontiguousarray(np.broadcast_to(end[:, None, :], (n, S, 3))).reshape(-1, 3)
        assert np.array_equal(ends - src.reshape(-1, 3), dirs.reshape(-1, 3))
        target = sa.MODE_BVH | L.TARGET_ROOT
        blocked = g.occluded(target, src.reshape(-1, 3), ends, endpoints=True)
        esc = S - blocked.reshape(n, S).astype(np.int64).sum(axis=1)
        want = g.shadow_points(as_sr(f), pos, nrm, None)
        got = ao_model.modulate(np.full(n, spm.WHITE, dtype=np.uint32), spm.light_bytes(esc, S))
        assert np.array_equal(got, want)
        assert len(set(esc.tolist())) >= 3                                    # lit, shadowed and penumbra points


# ---- 4. the device variant on a stream of the caller's: guards, inputs, statistics ----
def run_device(g, target, rs, variant, stream=None, stats=False, coherent=False):
    n = rs.n
    lim = rs.limits[variant]
    d_starts, d_dirs = torch.from_numpy(rs.starts).to(DEV), torch.from_numpy(rs.dirs).to(DEV)
    d_lim = torch.from_numpy(lim).to(DEV) if lim is not None else None
    d_out = torch.full((64 + n + 64,), GUARD, dtype=torch.uint8, device=DEV)
    d_stats = torch.full((24,), -1, dtype=torch.int64, device=DEV) if stats else None
    torch.cuda.synchronize(DEV)
    g.occluded_device(target, n, d_starts.data_ptr(), d_dirs.data_ptr(), d_lim.data_ptr() if d_lim is not None else 0, d_out.data_ptr() + 64,
                      endpoints=rs.endpoints, coherent=coherent, stream=stream if stream is not None else 0, d_stats_ptr=d_stats.data_ptr() if stats else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize(DEV)
    raw = d_out.cpu().numpy()
    guards_ok = bool(np.all(raw[:64] == GUARD) and np.all(raw[-64:] == GUARD))
    inputs_ok = (np.array_equal(d_starts.cpu().numpy().view(np.uint64), rs.starts.view(np.uint64)) and
                 np.array_equal(d_dirs.cpu().numpy().view(np.uint64), rs.dirs.view(np.uint64)) and
                 (d_lim is None or np.array_equal(d_lim.cpu().numpy().view(np.uint64), lim.view(np.uint64))))
    return raw[64:-64].copy(), guards_ok, inputs_ok, (d_stats.cpu().numpy().view(np.uint64) if stats else None)


@pytest.mark.parametrize("mode", ["tree", "brute", "bvh"])
@pytest.mark.parametrize("name", ["irregular", "irregular_ends", "n65"])
def test_device_variant_on_a_stream_guards_and_statistics(scenes, mode, name):
    sc = scenes("cube")
    g = sc.gpu(True)
    rs = occ.ray_set("cube", name)
    target = MODES[mode] | L.TARGET_ROOT
    st = torch.cuda.Stream(DEV)
    for variant in rs.limits:
        host, host_stats = call(g, target, rs, variant, stats=True)
        last = g.ray_stats()
        assert np.array_equal(last[:4], host_stats) and not last[4:].any() and host_stats[0] == rs.n
        got, guards_ok, inputs_ok, stats = run_device(g, target, rs, variant, stream=st, stats=True)
        assert guards_ok and inputs_ok
        assert set(np.unique(got)) <= {0, 1} and same(got, host)
        assert stats[0] == rs.n and not stats[4:].any()
        if mode != "bvh":
            assert np.array_equal(stats, last)
            cnt = g.trace(target, rs.starts, rs.D, counters=True)["counters"].astype(np.uint64)
            assert np.array_equal(stats[1:4], cnt.sum(axis=0))
        else:
            # the own BVH's counters are what the walks fetched, the same walks in both variants
            assert np.array_equal(stats, last)
        got2, guards_ok, inputs_ok, none = run_device(g, target, rs, variant, coherent=True)
        assert guards_ok and inputs_ok and none is None and same(got2, host)


# ---- 5. refusals ----
def raw_call(h, target, n, starts, dirs, limits, out, options, stats=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)          # noqa: E731
    rc = L.lib().sr_occluded_rays(h, target, n, p(starts), p(dirs), p(limits), p(out), options, p(stats))
    return rc, (L.lib().sr_last_error().decode() if rc else "")


def raw_call_device(h, target, n, starts, dirs, limits, out, options):
    v = lambda t: None if t is None else C.c_void_p(t.data_ptr())              # noqa: E731
    rc = L.lib().sr_occluded_rays_device(h, target, n, v(starts), v(dirs), v(limits), v(out), options, None, None)
    return rc, (L.lib().sr_last_error().decode() if rc else "")


def test_refusals_in_the_headers_order(scenes):
    sc = scenes("cube")
    g = sc.gpu(True)
    s = np.zeros((4, 3)); d = np.ones((4, 3)); out = np.full(4, GUARD, dtype=np.uint8)
    bare = sa.GpuScene(0)                                                    # no model
    unbuilt = sa.GpuScene(0)                                                 # a model, no tree
    unbuilt.set_triangles(*sc.tris)
    host = sa.GpuScene(-1)                                                   # a model and its reference tree, no device
    host.set_triangles(*sc.tris)
    host.build((sa.MODE_REF_TREE,))
    bvh, vox = sa.MODE_BVH, L.TARGET_VOXELS
    # every row breaks the rule it names and every later one it can: the earliest refusal is the one reported
    table = [
        ((None, vox, -1, None, None, None, None, 4), L.SR_ERR_INVALID_ARG, "sr_occluded_rays: the scene is NULL"),
        ((bare._h, vox, -1, None, None, None, None, 4), L.SR_ERR_INVALID_ARG, "sr_occluded_rays: n is negative"),
        ((bare._h, vox, 4, None, d, None, out, 4), L.SR_ERR_INVALID_ARG, "sr_occluded_rays: starts, dirs and occluded must not be NULL when n > 0"),
        ((bare._h, vox, 4, s, None, None, out, 4), L.SR_ERR_INVALID_ARG, "sr_occluded_rays: starts, dirs and occluded must not be NULL when n > 0"),
        ((bare._h, vox, 4, s, d, None, None, 4), L.SR_ERR_INVALID_ARG, "sr_occluded_rays: starts, dirs and occluded must not be NULL when n > 0"),
        ((bare._h, vox, 4, s, d, None, out, 4), L.SR_ERR_INVALID_ARG, "sr_occluded_rays: unknown option bits (SR_RAYS_COHERENT and SR_RAYS_ENDPOINTS are the options)"),
        ((bare._h, vox, 0, None, None, None, None, 1 << 31), L.SR_ERR_INVALID_ARG, "sr_occluded_rays: unknown option bits (SR_RAYS_COHERENT and SR_RAYS_ENDPOINTS are the options)"),
        ((bare._h, vox | bvh, 4, s, d, None, out, 3), L.SR_ERR_UNSUPPORTED,
         "sr_occluded_rays: a hit on the voxel grid (SR_TARGET_VOXELS) has rayFrac 0, so a distance limit decides nothing; use sr_trace_rays"),
        ((bare._h, bvh, 4, s, d, None, out, 0), L.SR_ERR_NO_MODEL, "sr_occluded_rays: the scene has no model (sr_set_triangles, sr_load_3ds)"),
        ((unbuilt._h, bvh, 4, s, d, None, out, 0), L.SR_ERR_NOT_BUILT, "SR_MODE_BVH needs sr_build(1 << SR_MODE_BVH)"),
        ((unbuilt._h, sa.MODE_REF_TREE | L.TARGET_ROOT, 4, s, d, None, out, 0), L.SR_ERR_NOT_BUILT, "SR_MODE_REF_TREE needs sr_build(1 << SR_MODE_REF_TREE)"),
        ((host._h, bvh, 4, s, d, None, out, 0), L.SR_ERR_NOT_BUILT, "SR_MODE_BVH needs sr_build(1 << SR_MODE_BVH)"),
        ((host._h, sa.MODE_REF_TREE, 4, s, d, None, out, 0), L.SR_ERR_NO_DEVICE,
         "sr_occluded_rays: a host-only scene has no HIP device to walk on (compute is never emulated on the CPU)"),
        ((host._h, sa.MODE_REF_TREE, 0, None, None, None, None, 0), L.SR_ERR_NO_DEVICE,
         "sr_occluded_rays: a host-only scene has no HIP device to walk on (compute is never emulated on the CPU)"),
    ]
    for args, code, message in table:
        assert raw_call(*args) == (code, message), message
        assert np.all(out == GUARD)
    # the device variant refuses the same way
    d_s, d_d = torch.zeros((4, 3), dtype=torch.float64, device=DEV), torch.ones((4, 3), dtype=torch.float64, device=DEV)
    d_out = torch.full((4,), GUARD, dtype=torch.uint8, device=DEV)
    for h, target, n, a, b, o, options, code in ((None, bvh, 4, d_s, d_d, d_out, 0, L.SR_ERR_INVALID_ARG), (g._h, bvh, -1, d_s, d_d, d_out, 0, L.SR_ERR_INVALID_ARG),
                                                 (g._h, bvh, 4, d_s, None, d_out, 0, L.SR_ERR_INVALID_ARG), (g._h, bvh, 4, d_s, d_d, d_out, 8, L.SR_ERR_INVALID_ARG),
                                                 (g._h, vox, 4, d_s, d_d, d_out, 0, L.SR_ERR_UNSUPPORTED), (bare._h, bvh, 4, d_s, d_d, d_out, 0, L.SR_ERR_NO_MODEL),
                                                 (unbuilt._h, bvh, 4, d_s, d_d, d_out, 0, L.SR_ERR_NOT_BUILT), (host._h, sa.MODE_REF_TREE, 4, d_s, d_d, d_out, 0, L.SR_ERR_NO_DEVICE)):
        assert raw_call_device(h, target, n, a, b, None, o, options)[0] == code
    torch.cuda.synchronize(DEV)
    assert bool((d_out == GUARD).all())
    # n == 0 that passes every check: SR_OK, nothing is touched -- with arrays and without
    stats = np.full(4, 77, dtype=np.uint64)
    before = g.ray_stats().copy()
    for target in (bvh, sa.MODE_REF_TREE | L.TARGET_ROOT, sa.MODE_BRUTE):
        assert raw_call(g._h, target, 0, s, d, None, out, 3, stats) == (0, "")
        assert raw_call(g._h, target, 0, None, None, None, None, 0) == (0, "")
        assert raw_call_device(g._h, target, 0, None, None, None, None, 0) == (0, "")
    assert np.all(out == GUARD) and np.all(stats == 77) and np.array_equal(g.ray_stats(), before)
    with pytest.raises(sa.SoftrayError):
        g.occluded(bvh | vox, s, d)


# ---- 6. state ----
def test_a_shadowed_frame_before_and_after_the_call_is_the_same_frame(scenes):
    sc = scenes("cube")
    g = sa.GpuScene(0)                                                       # a scene of its own: the frames' hints stay here
    g.set_triangles(*sc.tris)
    g.set_extra(list(sc.prims))
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=True)
    f = as_sr(gbc.frame_of(("cube", "out", 200, 160, None, 1, False), shadows=True))
    rs = occ.ray_set("cube", "irregular")
    target = sa.MODE_BVH | L.TARGET_ROOT
    want = by_trace(g, target, rs, "rot")
    first = np.asarray(g.render(f)[0]).view(np.uint32).ravel().copy()
    assert same(call(g, target, rs, "rot"), want)
    for _ in range(2):
        assert np.array_equal(np.asarray(g.render(f)[0]).view(np.uint32).ravel(), first)
        assert same(call(g, target, rs, "rot", coherent=True), want)
    assert len(set(first.tolist())) > 100


def test_frame_call_frame_on_three_streams_is_bit_stable(scenes):
    """A frame on one stream, the call on another at once, a frame behind it on a third: the call reads the records a frame's set-up moves."""
    sc = scenes("cube")
    g = sc.gpu(True)
    f = as_sr(gbc.frame_of(("cube", "out", 200, 160, None, 1, False), shadows=True))
    f2 = as_sr(gbc.frame_of(("cube", "in", 200, 160, None, 1, False), shadows=True))      # another camera: its set-up moves the records again
    rs = occ.ray_set("cube", "segments")
    target = sa.MODE_BVH | L.TARGET_ROOT
    want = call(g, target, rs, "rot")
    want_px = [np.asarray(g.render(fr)[0]).view(np.uint32).ravel().copy() for fr in (f, f2)]
    d_starts, d_dirs = torch.from_numpy(rs.starts).to(DEV), torch.from_numpy(rs.dirs).to(DEV)
    d_lim = torch.from_numpy(rs.limits["rot"]).to(DEV)
    s1, s2, s3 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    for _ in range(3):
        d_out = torch.full((rs.n,), GUARD, dtype=torch.uint8, device=DEV)
        px = [torch.zeros(200 * 160, dtype=torch.int32, device=DEV) for _ in range(2)]
        torch.cuda.synchronize(DEV)
        g.render_device(f, px[0].data_ptr(), s1.cuda_stream)
        g.occluded_device(target, rs.n, d_starts.data_ptr(), d_dirs.data_ptr(), d_lim.data_ptr(), d_out.data_ptr(), endpoints=rs.endpoints, stream=s2)
        g.render_device(f2, px[1].data_ptr(), s3.cuda_stream)
        torch.cuda.synchronize(DEV)
        assert same(d_out.cpu().numpy(), want)
        for p, w in zip(px, want_px):
            assert np.array_equal(p.cpu().numpy().view(np.uint32), w)


def test_multi_device_scene_gives_the_single_device_answer(scenes):
    sc = scenes("cube")
    g1 = sc.gpu(True)
    g = sc.gpu(None, devices=[0, 0])
    assert g.device_count() == 2
    for name in ("segments", "irregular"):
        rs = occ.ray_set("cube", name)
        for mode in MODES.values():
            target = mode | L.TARGET_ROOT
            got, stats = call(g, target, rs, "rot", stats=True)
            assert same(got, call(g1, target, rs, "rot"))
            assert stats[0] == rs.n and np.array_equal(g.ray_stats()[:4], stats)          # the first part's, reported by the multi-device scene
            dev, guards_ok, inputs_ok, _ = run_device(g, target, rs, "rot")
            assert guards_ok and inputs_ok and same(dev, got)


def test_after_a_refit_the_call_equals_trace_rays_on_the_refit_scene():
    v9, argb, lo, hi = unit_cube_scene(1500, seed=4242)
    g = sa.GpuScene(0)
    g.set_triangles(v9, argb, lo, hi)
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=True)
    rs = occ.ray_set("cube", "segments")                                      # (the same box)
    before = call(g, sa.MODE_BVH, rs, "rot")
    assert same(before, by_trace(g, sa.MODE_BVH, rs, "rot"))
    moved = np.ascontiguousarray(v9.reshape(-1, 3, 3) * np.array([0.9, 0.8, 0.95]) + np.array([0.02, -0.03, 0.01])).reshape(v9.shape)
    g.refit_triangles_device(torch.from_numpy(moved.reshape(-1, 3, 3)).to(DEV), None, lo, hi)
    torch.cuda.synchronize(DEV)
    for variant in rs.limits:
        after = call(g, sa.MODE_BVH, rs, variant)
        assert same(after, by_trace(g, sa.MODE_BVH, rs, variant))
        assert 0 < after.sum() < rs.n
    assert not same(call(g, sa.MODE_BVH, rs, "rot"), before)
    fresh = sa.GpuScene(0)
    fresh.set_triangles(moved, argb, lo, hi)
    fresh.build((sa.MODE_BVH,), on_device=True)
    assert same(call(g, sa.MODE_BVH, rs, "rot"), call(fresh, sa.MODE_BVH, rs, "rot"))


# ---- 7. structured meshes: segments in the plates' planes, ending on vertices ----
def in_plane_segments(name, count=1536, seed=606):
    """Segments that end on distinct mesh vertices.  edge_on: the start lies in the vertex's plate plane (x = k / 8 or y = k / 8, dyadic
    coordinates: the segment lies in that plane exactly); slivers: the start is a seeded point of the box above the vertex."""
    v9 = mc.scene(name)[0]
    verts, _ = mc.mesh_vertices(v9)
    rng = np.random.default_rng(seed)
    if name == "edge_on":
        on_x = np.isin(verts[:, 0], np.arange(-2, 3) * mc.PLATE_STEP) & (np.abs(verts[:, 1]) <= 0.3125)
        on_y = np.isin(verts[:, 1], np.arange(-2, 3) * mc.PLATE_STEP) & (np.abs(verts[:, 0]) <= 0.3125)
        ends, starts = [], []
        for mask, axis in ((on_x, 0), (on_y, 1)):
            v = verts[mask][rng.permutation(int(mask.sum()))[:count // 2]]
            s = np.round(rng.uniform(-0.45, 0.45, size=v.shape) * 256.0) / 256.0
            s[:, axis] = v[:, axis]
            ends.append(v); starts.append(s)
        return np.ascontiguousarray(np.concatenate(starts)), np.ascontiguousarray(np.concatenate(ends))
    v = verts[rng.permutation(verts.shape[0])[:count]]
    s = v + rng.uniform(-0.3, 0.3, size=v.shape) * np.array([1.0, 0.0, 1.0]) + np.array([0.0, 1.0, 0.0]) * rng.uniform(0.02, 0.5, size=(v.shape[0], 1))
    return np.ascontiguousarray(np.clip(s, -0.49, 0.49)), np.ascontiguousarray(v)


@pytest.mark.parametrize("name", ["slivers", "edge_on"])
def test_segments_in_plate_planes_ending_on_vertices_equal_trace_rays(name):
    v9, argb, lo, hi = mc.scene(name)
    starts, ends = in_plane_segments(name)
    assert starts.shape[0] > 1000
    D = np.ascontiguousarray(ends - starts)
    if name == "edge_on":
        assert np.all((D[:, 0] == 0.0) | (D[:, 1] == 0.0))                    # every segment lies in a plate plane
    some = 0
    for on_device in (True, False):
        g = sa.GpuScene(0)
        g.set_triangles(v9, argb, lo, hi)
        g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=on_device)
        for mode in MODES.values():
            res = g.trace(mode, starts, D)
            f = np.where(res["hit"].astype(bool), res["ray_frac"], 1.0)
            for limits in (None, occ.rotated_limits(f), np.full(f.shape[0], 1.0 + 2.0 ** -20)):
                want = occ.model(res, np.full(f.shape[0], 1.0) if limits is None else limits)
                got = g.occluded(mode, starts, ends, limits=limits, endpoints=True)
                assert same(got, want), (name, on_device, mode)
                some += int(got.sum())
    assert some > 100
