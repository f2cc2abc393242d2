"""The closest point of the mesh for a batch of points (sr_closest_points) on the GPU.  Every comparison is an exact equality over every point
and every output, and every output of every call lies between guard bytes (0x5A, 64 before and 64 behind) that are checked afterwards: the
own BVH's walk against brute force against the model of tests/closest_points_model.py on host-built and device-built trees, limits of every
kind, the schedules and passes against each other, any subset of the outputs, the device variant against the host variant, brute-force
statistics, a refit against a fresh build, a two-part scene against the single scene, and frames around the call against themselves.
Scenes and point sets: tests/closest_points_cases.py (what they hold is pinned on the CPU in tests/test_closest_points_model.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import closest_points_cases as cpc
import closest_points_model as cpm
import gbuffer_cases as gbc
import softray_amd as sa

pytestmark = pytest.mark.gpu
L = sa._lib
DEV = torch.device("cuda", 0)
GUARD = 0x5A
PAD = 64
KEYS = ("tri_index", "dist", "pos", "uv")
NP_TYPES = dict(tri_index=np.int32, dist=np.float64, pos=np.float64, uv=np.float64)
MODES = (sa.MODE_BVH, sa.MODE_BRUTE)


def shapes(n):
    return dict(tri_index=(n,), dist=(n,), pos=(n, 3), uv=(n, 2))


class Scene:
    """One scene on the device (host-built and device-built own BVH), its points and the model's answers (computed once, left unchanged)."""

    def __init__(self, name):
        self.name = name
        self.tris = cpc.scene(name)
        self.points = cpc.points(name)
        self.n = self.points.shape[0]
        self.answers = cpm.Answers(self.points, self.tris[0])
        self.gpus = {}

    def gpu(self, on_device=None, devices=None):
        key = (on_device, None if devices is None else tuple(devices))
        if key not in self.gpus:
            g = sa.GpuScene(0) if devices is None else sa.GpuScene(devices=devices)
            g.set_triangles(*self.tris)
            g.build((sa.MODE_BVH,), on_device=on_device)
            self.gpus[key] = g
        return self.gpus[key]

    def builds(self):
        return (None,) if self.name in cpc.HOST_BUILT_ONLY else (False, True)

    def any_gpu(self):
        return self.gpu(self.builds()[-1])


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Scene(name)
        return made[name]
    return get


def guarded(shape, dtype):
    return np.full(PAD + int(np.prod(shape)) * np.dtype(dtype).itemsize + PAD, GUARD, dtype=np.uint8)


def view(raw, shape, dtype):
    return raw[PAD:raw.size - PAD].view(dtype).reshape(shape)


def guards_ok(raw):
    return bool(np.all(raw[:PAD] == GUARD) and np.all(raw[-PAD:] == GUARD))


def call(g, target, points, limits=None, want=KEYS, coherent=False, stats=None):
    """sr_closest_points with the outputs of `want` between guard bytes (the others NULL): a dict of copies."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    n = points.shape[0]
    raws = {k: guarded(shapes(n)[k], NP_TYPES[k]) for k in want}
    ptr = lambda k: C.c_void_p(raws[k].ctypes.data + PAD) if k in raws else None          # noqa: E731
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                      # noqa: E731
    rc = L.lib().sr_closest_points(g._h, target, n, p(points), p(limits), ptr("tri_index"), ptr("dist"), ptr("pos"), ptr("uv"),
                                   L.POINTS_COHERENT if coherent else 0, p(stats))
    assert rc == 0, L.lib().sr_last_error().decode()
    assert all(guards_ok(r) for r in raws.values()), "guard bytes"
    return {k: view(raws[k], shapes(n)[k], NP_TYPES[k]).copy() for k in raws}


def same(got, want):
    return set(got) <= set(want) and all(cpm.same_bits(got[k], want[k]) for k in got)


def with_hook(g, hook, fn):
    g.debug_set(L.DBG_KERNEL_SWITCH, hook)
    try:
        return fn()
    finally:
        g.debug_set(L.DBG_KERNEL_SWITCH, -1)


def with_pass(g, points_per_pass, fn):
    g.debug_set(L.DBG_BAND_SAMPLES, points_per_pass)
    try:
        return fn()
    finally:
        g.debug_set(L.DBG_BAND_SAMPLES, -1)


# ---- 1. the walk, brute force and the model, on every scene and build ----
@pytest.mark.parametrize("scene", cpc.SCENES)
def test_bvh_equals_brute_equals_the_model(scenes, scene):
    sc = scenes(scene)
    want = sc.answers.outputs(None)
    for on_device in sc.builds():
        g = sc.gpu(on_device)
        for mode in MODES:
            got = call(g, mode, sc.points)
            for k in KEYS:
                bad = np.flatnonzero(~np.all((got[k] == want[k]).reshape(sc.n, -1), axis=1))
                assert cpm.same_bits(got[k], want[k]), (scene, on_device, mode, k, bad[:8], got[k][bad[:4]], want[k][bad[:4]])
    assert (want["tri_index"] >= 0).sum() > 2000 and (want["tri_index"] < 0).sum() >= 3


# ---- 2. limits of every kind ----
@pytest.mark.parametrize("scene", cpc.SCENES)
def test_limits_of_every_kind(scenes, scene):
    sc = scenes(scene)
    g = sc.any_gpu()
    lim, kind = cpc.limit_kinds(sc.answers.dist)
    rolled = np.ascontiguousarray(np.roll(lim, 3))                            # another point's distance as the limit: cuts some, keeps others
    half = np.ascontiguousarray(sc.answers.dist * 0.5)
    for v, limits in enumerate((lim, rolled, half, np.full(sc.n, np.inf))):
        want = sc.answers.outputs(limits)
        for mode in MODES:
            assert same(call(g, mode, sc.points, limits=limits), want), (scene, v, mode)
        if v < 2:
            kept = want["tri_index"] >= 0
            assert kept.any() and not kept.all()


# ---- 3. schedules: sorted, the caller's promise, the two hooks ----
@pytest.mark.parametrize("scene", ("small", "layers", "slivers", "limit", "far_probe"))
def test_schedules_give_the_same_answers(scenes, scene):
    sc = scenes(scene)
    g = sc.any_gpu()
    lim, _ = cpc.limit_kinds(sc.answers.dist)
    for limits in (None, lim):
        want = sc.answers.outputs(limits)
        assert same(call(g, sa.MODE_BVH, sc.points, limits=limits), want)
        assert same(call(g, sa.MODE_BVH, sc.points, limits=limits, coherent=True), want)
        assert same(with_hook(g, 52, lambda: call(g, sa.MODE_BVH, sc.points, limits=limits)), want)          # input order
        assert same(with_hook(g, 53, lambda: call(g, sa.MODE_BVH, sc.points, limits=limits)), want)          # the per-record loop for every point
        assert same(with_hook(g, 53, lambda: call(g, sa.MODE_BVH, sc.points, limits=limits, coherent=True)), want)


# ---- 4. passes ----
@pytest.mark.parametrize("scene", ("layers", "degenerate"))
def test_passes_of_100_and_257_points(scenes, scene):
    sc = scenes(scene)
    g = sc.any_gpu()
    lim, _ = cpc.limit_kinds(sc.answers.dist)
    want = sc.answers.outputs(lim)
    for per_pass in (100, 257):
        for mode in MODES:
            for coherent in (False, True):
                stats = np.zeros(4, dtype=np.uint64)
                got = with_pass(g, per_pass, lambda: call(g, mode, sc.points, limits=lim, coherent=coherent, stats=stats))
                assert same(got, want), (per_pass, mode, coherent)
                assert stats[0] == sc.n
    # the walk and the sort are recorded once per pass; brute force sorts nothing
    for mode in MODES:
        g.reset_kernel_times()
        g.debug_set(L.DBG_KERNEL_TIMING, 1)
        try:
            with_pass(g, 100, lambda: call(g, mode, sc.points, limits=lim))
            times = g.kernel_times()
        finally:
            g.debug_set(L.DBG_KERNEL_TIMING, -1)
        passes = (sc.n + 99) // 100
        assert times["k_closest"][1] == passes, mode
        if mode == sa.MODE_BVH:
            assert times["k_closest_sort"][1] == passes
        else:
            assert "k_closest_sort" not in times


# ---- 5. any subset of the outputs ----
def test_any_subset_of_the_outputs(scenes):
    sc = scenes("layers")
    g = sc.any_gpu()
    lim, _ = cpc.limit_kinds(sc.answers.dist)
    want = sc.answers.outputs(lim)
    for r in range(len(KEYS) + 1):
        for subset in itertools.combinations(KEYS, r):
            for mode in MODES:
                stats = np.zeros(4, dtype=np.uint64)
                got = call(g, mode, sc.points, limits=lim, want=subset, stats=stats)
                assert set(got) == set(subset) and same(got, want), (subset, mode)
                assert stats[0] == sc.n                                       # (all NULL: the call runs for the statistics)
    res = g.closest_points(sa.MODE_BVH, sc.points, max_dist=lim, want=("tri_index", "uv"), stats=True)
    assert res["dist"] is None and res["pos"] is None and same({k: res[k] for k in ("tri_index", "uv")}, want) and res["stats"][0] == sc.n


# ---- 6. the device variant ----
def run_device(g, target, points, limits=None, coherent=False, stream=None, want=KEYS):
    n = points.shape[0]
    d_points = torch.from_numpy(np.array(points, dtype=np.float64)).to(DEV)
    d_lim = None if limits is None else torch.from_numpy(np.ascontiguousarray(limits)).to(DEV)
    outs = {}
    for k in want:
        raw = torch.full((PAD + int(np.prod(shapes(n)[k])) * np.dtype(NP_TYPES[k]).itemsize + PAD,), GUARD, dtype=torch.uint8, device=DEV)
        outs[k] = raw
    d_stats = torch.full((24,), 77, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize(DEV)
    ptr = lambda k: outs[k].data_ptr() + PAD if k in outs else 0               # noqa: E731
    g.closest_points_device(target, n, d_points.data_ptr(), 0 if d_lim is None else d_lim.data_ptr(), ptr("tri_index"), ptr("dist"), ptr("pos"), ptr("uv"),
                            coherent=coherent, stream=stream if stream is not None else 0, d_stats_ptr=d_stats.data_ptr())
    torch.cuda.synchronize(DEV)
    raws = {k: v.cpu().numpy() for k, v in outs.items()}
    assert all(guards_ok(r) for r in raws.values()), "guard bytes"
    assert cpm.same_bits(d_points.cpu().numpy(), np.ascontiguousarray(points))
    return {k: view(raws[k], shapes(n)[k], NP_TYPES[k]).copy() for k in raws}, d_stats.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("scene", ("cube", "duplicates"))
def test_the_device_variant_equals_the_host_variant(scenes, scene):
    sc = scenes(scene)
    g = sc.any_gpu()
    lim, _ = cpc.limit_kinds(sc.answers.dist)
    st = torch.cuda.Stream(DEV)
    for mode in MODES:
        for limits in (None, lim):
            host_stats = np.zeros(4, dtype=np.uint64)
            host = call(g, mode, sc.points, limits=limits, stats=host_stats)
            assert same(host, sc.answers.outputs(limits))
            for stream, coherent in ((None, False), (st, True)):
                dev, stats = run_device(g, mode, sc.points, limits, coherent=coherent, stream=stream)
                assert same(dev, host), (mode, coherent)
                assert stats[0] == sc.n and not stats[4:].any()
                if mode == sa.MODE_BRUTE:
                    assert np.array_equal(stats[:4], host_stats)
    dev, _ = run_device(g, sa.MODE_BVH, sc.points, lim, want=("dist",))
    assert same(dev, sc.answers.outputs(lim))


# ---- 7. statistics ----
def test_brute_force_statistics_are_pinned(scenes):
    sc = scenes("layers")
    g = sc.any_gpu()
    T = sc.tris[0].shape[0]
    stats = np.full(4, 77, dtype=np.uint64)
    call(g, sa.MODE_BRUTE, sc.points, stats=stats)
    assert list(stats) == [sc.n, sc.n * T, 0, 0]
    assert np.array_equal(g.ray_stats()[:4], stats) and not g.ray_stats()[4:].any()
    call(g, sa.MODE_BVH, sc.points, stats=stats)
    reg = int(cpm.regular(sc.points, sc.tris[2], sc.tris[3]).sum())
    assert stats[0] == sc.n and stats[2] >= reg and stats[3] >= reg          # every regular point fetches the root and a leaf
    assert (sc.n - reg) * T <= stats[1] < sc.n * T                           # the walk tests fewer triangles than the loop; the irregular tail tests all
    with_hook(g, 53, lambda: call(g, sa.MODE_BVH, sc.points, stats=stats))
    assert list(stats) == [sc.n, sc.n * T, 0, 0]


# ---- 8. refusals with a device (the rest: tests/test_closest_points_mirror.py) and the empty batch ----
def test_refusals_and_the_empty_batch_on_a_device(scenes):
    sc = scenes("cube")
    g = sc.any_gpu()
    q = np.zeros((4, 3))
    tri = np.full(4, 7, dtype=np.int32); dist = np.full(4, 7.0); pos = np.full((4, 3), 7.0); uv = np.full((4, 2), 7.0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)          # noqa: E731
    untouched = lambda: bool(np.all(tri == 7) and np.all(dist == 7.0) and np.all(pos == 7.0) and np.all(uv == 7.0))      # noqa: E731

    def raw(h, target, n, a, options, stats=None):
        rc = L.lib().sr_closest_points(h, target, n, p(a), None, p(tri), p(dist), p(pos), p(uv), options, p(stats))
        return rc, (L.lib().sr_last_error().decode() if rc else "")

    d_q = torch.zeros((4, 3), dtype=torch.float64, device=DEV)
    d_tri = torch.full((4,), 7, dtype=torch.int32, device=DEV)

    def raw_device(h, target, n, a, options):
        rc = L.lib().sr_closest_points_device(h, target, n, None if a is None else C.c_void_p(a.data_ptr()), None, C.c_void_p(d_tri.data_ptr()), None, None, None,
                                              options, None, None)
        return rc, (L.lib().sr_last_error().decode() if rc else "")

    bare = sa.GpuScene(0)
    unbuilt = sa.GpuScene(0)
    unbuilt.set_triangles(*sc.tris)
    bvh, vox, root, tree, brute = sa.MODE_BVH, L.TARGET_VOXELS, L.TARGET_ROOT, sa.MODE_REF_TREE, sa.MODE_BRUTE
    tree_text = ("sr_closest_points: SR_MODE_REF_TREE has no distance query (a triangle lives in several leaves of the reference tree); use SR_MODE_BVH or "
                 "SR_MODE_BRUTE")
    table = [
        ((None, bvh, 4, 0), L.SR_ERR_INVALID_ARG, "sr_closest_points: the scene is NULL"),
        ((g._h, bvh, -1, 0), L.SR_ERR_INVALID_ARG, "sr_closest_points: n is negative"),
        ((g._h, bvh, 4, 2), L.SR_ERR_INVALID_ARG, "sr_closest_points: unknown option bits (SR_POINTS_COHERENT is the only option)"),
        ((g._h, vox, 4, 0), L.SR_ERR_UNSUPPORTED, "sr_closest_points: the voxel grid (SR_TARGET_VOXELS) has no triangles to measure a distance to"),
        ((g._h, root | bvh, 4, 0), L.SR_ERR_UNSUPPORTED,
         "sr_closest_points: the closest points of the extra geometry (SR_TARGET_ROOT) are not part of the call; pass the mode alone"),
        ((g._h, tree, 4, 0), L.SR_ERR_UNSUPPORTED, tree_text),
        ((bare._h, bvh, 4, 0), L.SR_ERR_NO_MODEL, "sr_closest_points: the scene has no model (sr_set_triangles, sr_load_3ds)"),
        ((unbuilt._h, bvh, 4, 0), L.SR_ERR_NOT_BUILT, "SR_MODE_BVH needs sr_build(1 << SR_MODE_BVH)"),
    ]
    for (h, target, n, options), code, message in table:
        assert raw(h, target, n, q, options) == (code, message), message
        assert raw_device(h, target, n, d_q, options) == (code, message), message
        assert untouched()
    assert raw(g._h, bvh, 4, None, 0)[0] == L.SR_ERR_INVALID_ARG and raw_device(g._h, bvh, 4, None, 0)[0] == L.SR_ERR_INVALID_ARG
    torch.cuda.synchronize(DEV)
    assert bool((d_tri == 7).all())
    stats = np.full(4, 77, dtype=np.uint64)
    before = g.ray_stats().copy()
    for target in MODES:
        assert raw(g._h, target, 0, q, 1, stats) == (0, "")
        assert raw(g._h, target, 0, None, 0) == (0, "")
        assert raw_device(g._h, target, 0, None, 0) == (0, "")
    assert untouched() and np.all(stats == 77) and np.array_equal(g.ray_stats(), before)
    # brute force on a model without a tree is fine
    assert same(call(unbuilt, brute, sc.points[:300]), {k: v[:300] for k, v in sc.answers.outputs(None).items()})


# ---- 9. a refit, and a two-part scene ----
def test_after_a_refit_the_answers_equal_a_fresh_build(scenes):
    sc = scenes("cube")
    v9, argb, lo, hi = sc.tris
    g = sa.GpuScene(0)
    g.set_triangles(v9, argb, lo, hi)
    g.build((sa.MODE_BVH,), on_device=True)
    before = call(g, sa.MODE_BVH, sc.points)
    assert same(before, sc.answers.outputs(None))
    moved = np.ascontiguousarray(v9 * np.array([0.9, 0.8, 0.95]) + np.array([0.02, -0.03, 0.01]))
    g.refit_triangles_device(torch.from_numpy(moved).to(DEV), None, lo, hi)
    torch.cuda.synchronize(DEV)
    fresh = sa.GpuScene(0)
    fresh.set_triangles(moved, argb, lo, hi)
    fresh.build((sa.MODE_BVH,), on_device=True)
    lim, _ = cpc.limit_kinds(sc.answers.dist)
    for limits in (None, lim):
        after = call(g, sa.MODE_BVH, sc.points, limits=limits)
        assert same(after, call(fresh, sa.MODE_BVH, sc.points, limits=limits))
        assert same(after, call(fresh, sa.MODE_BRUTE, sc.points, limits=limits))
        assert same(after, call(g, sa.MODE_BRUTE, sc.points, limits=limits))
    assert not same(call(g, sa.MODE_BVH, sc.points), before)
    assert same(call(g, sa.MODE_BVH, sc.points), cpm.Answers(sc.points, moved).outputs(None))


def test_a_two_part_scene_gives_the_single_scene_answer(scenes):
    sc = scenes("cube")
    g1 = sc.gpu(True)
    g = sc.gpu(None, devices=[0, 0])
    assert g.device_count() == 2
    lim, _ = cpc.limit_kinds(sc.answers.dist)
    for mode in MODES:
        stats = np.zeros(4, dtype=np.uint64)
        got = call(g, mode, sc.points, limits=lim, stats=stats)
        assert same(got, call(g1, mode, sc.points, limits=lim)) and same(got, sc.answers.outputs(lim))
        assert stats[0] == sc.n and np.array_equal(g.ray_stats()[:4], stats)
        dev, _ = run_device(g, mode, sc.points, lim)
        assert same(dev, got)


# ---- 10. state: frames around the call ----
def as_sr(frame):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = sa.MODE_BVH
    return f


def test_a_shadowed_frame_before_and_after_the_call_is_the_same_frame(scenes):
    sc = scenes("cube")
    g = sa.GpuScene(0)                                                       # a scene of its own: the frames' hints stay here
    g.set_triangles(*sc.tris)
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=True)
    f = as_sr(gbc.frame_of(("cube", "out", 200, 160, None, 1, False), shadows=True))
    want = sc.answers.outputs(None)
    first = np.asarray(g.render(f)[0]).view(np.uint32).ravel().copy()
    assert same(call(g, sa.MODE_BVH, sc.points), want)
    for _ in range(2):
        assert np.array_equal(np.asarray(g.render(f)[0]).view(np.uint32).ravel(), first)
        assert same(call(g, sa.MODE_BVH, sc.points, coherent=True), want)
    assert len(set(first.tolist())) > 100


def test_the_call_between_two_frames_from_different_cameras_is_unchanged(scenes):
    """A frame on one stream, the call on another at once, a frame behind it on a third: the call reads the records a frame's set-up moves."""
    sc = scenes("cube")
    g = sa.GpuScene(0)
    g.set_triangles(*sc.tris)
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=True)
    f = as_sr(gbc.frame_of(("cube", "out", 200, 160, None, 1, False), shadows=True))
    f2 = as_sr(gbc.frame_of(("cube", "in", 200, 160, None, 1, False), shadows=True))      # another camera: its set-up moves the records again
    want = sc.answers.outputs(None)
    want_px = [np.asarray(g.render(fr)[0]).view(np.uint32).ravel().copy() for fr in (f, f2)]
    n = sc.n
    d_points = torch.from_numpy(np.array(sc.points, dtype=np.float64)).to(DEV)
    s1, s2, s3 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    for _ in range(3):
        d_tri = torch.full((n,), 7, dtype=torch.int32, device=DEV)
        d_dist = torch.full((n,), 7.0, dtype=torch.float64, device=DEV)
        d_pos = torch.full((n, 3), 7.0, dtype=torch.float64, device=DEV)
        d_uv = torch.full((n, 2), 7.0, dtype=torch.float64, device=DEV)
        px = [torch.zeros(200 * 160, dtype=torch.int32, device=DEV) for _ in range(2)]
        torch.cuda.synchronize(DEV)
        g.render_device(f, px[0].data_ptr(), s1.cuda_stream)
        g.closest_points_device(sa.MODE_BVH, n, d_points.data_ptr(), 0, d_tri.data_ptr(), d_dist.data_ptr(), d_pos.data_ptr(), d_uv.data_ptr(), stream=s2)
        g.render_device(f2, px[1].data_ptr(), s3.cuda_stream)
        torch.cuda.synchronize(DEV)
        got = dict(tri_index=d_tri.cpu().numpy(), dist=d_dist.cpu().numpy(), pos=d_pos.cpu().numpy(), uv=d_uv.cpu().numpy())
        assert same(got, want)
        for q, w in zip(px, want_px):
            assert np.array_equal(q.cpu().numpy().view(np.uint32), w)
