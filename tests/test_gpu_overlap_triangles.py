"""The triangles of the model that cross a batch of triangles (sr_overlap_triangles) on the GPU.  Every comparison is an exact equality over
every query, slot and output, and every output of every call lies between guard bytes (0x5A, 64 before and 64 behind) that are checked
afterwards: the own BVH's walk against brute force against the model of tests/overlap_model.py on host-built and device-built trees for K
in (0, 1, 4, 64), with and without `count`; SR_OVERLAP_ANY against count > 0; any subset of the outputs; the device variant against the
host variant; the schedules and passes against each other; brute-force statistics; refusals and the empty batch; a refit against a fresh
build; a two-part scene against the single scene; a frame around the call against itself.
Scenes and queries: tests/overlap_cases.py (what they hold is pinned on the CPU in tests/test_overlap_model.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import closest_points_cases as cpc
import gbuffer_cases as gbc
import overlap_cases as oc
import overlap_model as om
import softray_amd as sa

pytestmark = pytest.mark.gpu
L = sa._lib
DEV = torch.device("cuda", 0)
GUARD = 0x5A
PAD = 64
KEYS = om.KEYS
ROWS = ("index", "mask")
MODES = (sa.MODE_BVH, sa.MODE_BRUTE)


class Scene:
    """One scene on the device (host-built and device-built own BVH) and the model's answers (computed once, left unchanged)."""

    def __init__(self, name):
        self.name = name
        self.tris = cpc.scene(name)
        self.model = oc.model(name)
        self.queries = self.model.queries
        self.n = self.queries.shape[0]
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


def call(g, target, queries, k, want=KEYS, coherent=False, any_hit=False, stats=None):
    """sr_overlap_triangles with the outputs of `want` between guard bytes (the others NULL): a dict of copies."""
    queries = np.ascontiguousarray(queries, dtype=np.float64)
    n = queries.shape[0]
    shp = om.shapes(n, k)
    raws = {key: guarded(shp[key], om.NP_TYPES[key]) for key in want}
    ptr = lambda key: C.c_void_p(raws[key].ctypes.data + PAD) if key in raws else None      # noqa: E731
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    options = (L.POINTS_COHERENT if coherent else 0) | (L.OVERLAP_ANY if any_hit else 0)
    rc = L.lib().sr_overlap_triangles(g._h, target, n, p(queries), k, ptr("count"), ptr("index"), ptr("mask"), options, p(stats))
    assert rc == 0, L.lib().sr_last_error().decode()
    assert all(guards_ok(r) for r in raws.values()), "guard bytes"
    return {key: view(raws[key], shp[key], om.NP_TYPES[key]).copy() for key in raws}


def same(got, want):
    return set(got) <= set(want) and all(om.same_bits(got[k], want[k]) for k in got)


def explain(got, want):
    for k in got:
        if not om.same_bits(got[k], want[k]):
            bad = np.flatnonzero(~np.all((got[k] == want[k]).reshape(got[k].shape[0], -1), axis=1))
            return k, bad[:8], got[k][bad[:2]], want[k][bad[:2]]
    return None


def with_hook(g, hook, fn):
    g.debug_set(L.DBG_KERNEL_SWITCH, hook)
    try:
        return fn()
    finally:
        g.debug_set(L.DBG_KERNEL_SWITCH, -1)


def with_pass(g, per_pass, fn):
    g.debug_set(L.DBG_BAND_SAMPLES, per_pass)
    try:
        return fn()
    finally:
        g.debug_set(L.DBG_BAND_SAMPLES, -1)


# ---- 1. the walk, brute force and the model, on every scene and build, with and without the count ----
@pytest.mark.parametrize("scene", oc.SCENES)
def test_bvh_equals_brute_equals_the_model(scenes, scene):
    sc = scenes(scene)
    runs = [(sc.gpu(b), sa.MODE_BVH, b) for b in sc.builds()] + [(sc.any_gpu(), sa.MODE_BRUTE, "brute")]
    for k in oc.KS:
        want = sc.model.want(k)
        for g, mode, label in runs:
            for out in (KEYS, ROWS):
                got = call(g, mode, sc.queries, k, want=out)
                assert set(got) == set(out) and same(got, want), (scene, k, label, out, explain(got, want))
    assert (sc.model.rows.count == 0).sum() > 100 and (sc.model.rows.count > 0).sum() > 100


# ---- 2. SR_OVERLAP_ANY is count > 0 ----
@pytest.mark.parametrize("scene", oc.SCENES)
def test_any_equals_a_positive_count(scenes, scene):
    sc = scenes(scene)
    want = sc.model.any()
    assert 0 < want["count"].sum() < sc.n
    for g, mode in [(sc.gpu(b), sa.MODE_BVH) for b in sc.builds()] + [(sc.any_gpu(), sa.MODE_BRUTE)]:
        for coherent in (False, True):
            got = call(g, mode, sc.queries, 0, want=("count",), coherent=coherent, any_hit=True)
            assert same(got, want), (scene, mode, coherent, explain(got, want))
    g = sc.any_gpu()
    assert call(g, sa.MODE_BVH, sc.queries, 0, want=(), any_hit=True) == {}
    # the walk stops at the first one: fewer pairs are tested than by the counting call
    counted, stopped = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    call(g, sa.MODE_BVH, sc.queries, 0, stats=counted)
    call(g, sa.MODE_BVH, sc.queries, 0, any_hit=True, stats=stopped)
    assert stopped[0] == counted[0] == sc.n and stopped[1] < counted[1]


# ---- 3. any subset of the outputs (an index row that the masks need and the caller did not ask for lives in the scene's scratch) ----
def test_any_subset_of_the_outputs(scenes):
    sc = scenes("layers")
    g = sc.any_gpu()
    for k in (4, 64):
        want = sc.model.want(k)
        for r in range(len(KEYS) + 1):
            for subset in itertools.combinations(KEYS, r):
                for mode in MODES:
                    stats = np.zeros(4, dtype=np.uint64)
                    got = call(g, mode, sc.queries, k, want=subset, stats=stats)
                    assert set(got) == set(subset) and same(got, want), (k, subset, mode)
                    assert stats[0] == sc.n                                   # (all NULL: the call runs for the statistics)
    res = g.overlap_triangles(sa.MODE_BVH, sc.queries, max_hits=4, want=("count", "mask"), stats=True)
    assert res["index"] is None and res["stats"][0] == sc.n
    assert same({k: res[k] for k in ("count", "mask")}, sc.model.want(4))
    res = g.overlap_triangles(sa.MODE_BRUTE, sc.queries, max_hits=0)
    assert same({"count": res["count"]}, sc.model.want(0)) and res["index"].shape == (sc.n, 0)
    res = g.overlap_triangles(sa.MODE_BVH, sc.queries, max_hits=0, want=("count",), any_hit=True)
    assert same({"count": res["count"]}, sc.model.any())


# ---- 4. the device variant ----
def run_device(g, target, queries, k, coherent=False, any_hit=False, stream=None, want=KEYS):
    n = queries.shape[0]
    shp = om.shapes(n, k)
    d_q = torch.from_numpy(np.array(queries, dtype=np.float64)).to(DEV)
    outs = {}
    for key in want:
        outs[key] = torch.full((PAD + int(np.prod(shp[key])) * np.dtype(om.NP_TYPES[key]).itemsize + PAD,), GUARD, dtype=torch.uint8, device=DEV)
    d_stats = torch.full((24,), 77, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize(DEV)
    ptr = lambda key: outs[key].data_ptr() + PAD if key in outs else 0                       # noqa: E731
    g.overlap_triangles_device(target, n, d_q.data_ptr(), k, ptr("count"), ptr("index"), ptr("mask"), coherent=coherent, any_hit=any_hit,
                               stream=stream if stream is not None else 0, d_stats_ptr=d_stats.data_ptr())
    torch.cuda.synchronize(DEV)
    raws = {key: v.cpu().numpy() for key, v in outs.items()}
    assert all(guards_ok(r) for r in raws.values()), "guard bytes"
    assert om.same_bits(d_q.cpu().numpy(), np.ascontiguousarray(queries))
    return {key: view(raws[key], shp[key], om.NP_TYPES[key]).copy() for key in raws}, d_stats.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("scene", ("cube", "duplicates"))
def test_the_device_variant_equals_the_host_variant(scenes, scene):
    sc = scenes(scene)
    g = sc.any_gpu()
    st = torch.cuda.Stream(DEV)
    for mode in MODES:
        for k in (4, 64, 0):
            host_stats = np.zeros(4, dtype=np.uint64)
            host = call(g, mode, sc.queries, k, stats=host_stats)
            assert same(host, sc.model.want(k))
            for stream, coherent in ((None, False), (st, True)):
                dev, stats = run_device(g, mode, sc.queries, k, coherent=coherent, stream=stream)
                assert same(dev, host), (mode, k, coherent)
                assert stats[0] == sc.n and not stats[4:].any()
                if mode == sa.MODE_BRUTE:
                    assert np.array_equal(stats[:4], host_stats)
        dev, _ = run_device(g, mode, sc.queries, 0, any_hit=True, stream=st, want=("count",))
        assert same(dev, sc.model.any())
    dev, _ = run_device(g, sa.MODE_BVH, sc.queries, 4, want=("mask",), stream=st)
    assert same(dev, sc.model.want(4))


# ---- 5. schedules: sorted, the caller's promise, the two hooks ----
@pytest.mark.parametrize("scene", ("small", "layers", "slivers", "limit", "far_probe"))
def test_schedules_give_the_same_answers(scenes, scene):
    sc = scenes(scene)
    g = sc.any_gpu()
    for k, out, any_hit in ((4, ROWS, False), (4, KEYS, False), (64, KEYS, False), (0, KEYS, False), (0, ("count",), True)):
        want = sc.model.any() if any_hit else sc.model.want(k)
        run = lambda coherent=False: call(g, sa.MODE_BVH, sc.queries, k, want=out, coherent=coherent, any_hit=any_hit)      # noqa: E731
        assert same(run(), want)
        assert same(run(True), want)
        assert same(with_hook(g, 56, run), want)                              # input order
        assert same(with_hook(g, 57, run), want)                              # the per-record loop for every query
        assert same(with_hook(g, 57, lambda: run(True)), want)


# ---- 6. passes ----
@pytest.mark.parametrize("scene", ("layers", "degenerate"))
def test_passes_of_64_queries(scenes, scene):
    sc = scenes(scene)
    g = sc.any_gpu()
    for per_pass in (64, 257):
        for mode in MODES:
            for k, out, coherent in ((4, KEYS, False), (4, ("count", "mask"), True), (64, ROWS, False)):
                stats = np.zeros(4, dtype=np.uint64)
                got = with_pass(g, per_pass, lambda: call(g, mode, sc.queries, k, want=out, coherent=coherent, stats=stats))
                assert same(got, sc.model.want(k)), (per_pass, mode, k, out)
                assert stats[0] == sc.n
            got = with_pass(g, per_pass, lambda: call(g, mode, sc.queries, 0, want=("count",), any_hit=True))
            assert same(got, sc.model.any())
    # the walk and the sort are recorded once per pass; brute force sorts nothing
    for mode in MODES:
        g.reset_kernel_times()
        g.debug_set(L.DBG_KERNEL_TIMING, 1)
        try:
            with_pass(g, 64, lambda: call(g, mode, sc.queries, 4))
            times = g.kernel_times()
        finally:
            g.debug_set(L.DBG_KERNEL_TIMING, -1)
        passes = (sc.n + 63) // 64
        assert times["k_overlap"][1] == passes, mode
        if mode == sa.MODE_BVH:
            assert times["k_overlap_sort"][1] == passes
        else:
            assert "k_overlap_sort" not in times
        assert "k_near" not in times and "k_closest_sort" not in times


# ---- 7. statistics ----
def test_brute_force_statistics_are_pinned(scenes):
    sc = scenes("layers")
    g = sc.any_gpu()
    T = sc.tris[0].shape[0]
    for k, out in ((4, KEYS), (0, ("count",)), (64, ROWS), (4, ())):
        stats = np.full(4, 77, dtype=np.uint64)
        call(g, sa.MODE_BRUTE, sc.queries, k, want=out, stats=stats)
        assert list(stats) == [sc.n, sc.n * T, 0, 0]
        assert np.array_equal(g.ray_stats()[:4], stats) and not g.ray_stats()[4:].any()
    stats = np.full(4, 77, dtype=np.uint64)
    call(g, sa.MODE_BVH, sc.queries, 4, stats=stats)
    reg = int(oc.regular(sc.queries, sc.tris[2], sc.tris[3]).sum())
    assert stats[0] == sc.n and stats[2] >= reg                              # every regular query fetches the root
    assert (sc.n - reg) * T <= stats[1] < sc.n * T                           # the walk tests fewer pairs than the loop; the irregular tail tests all
    with_hook(g, 57, lambda: call(g, sa.MODE_BVH, sc.queries, 4, stats=stats))
    assert list(stats) == [sc.n, sc.n * T, 0, 0]


# ---- 8. refusals with a device (the rest: tests/test_overlap_mirror.py) and the empty batch ----
def test_refusals_and_the_empty_batch_on_a_device(scenes):
    sc = scenes("cube")
    g = sc.any_gpu()
    q = np.zeros((4, 3, 3))
    cnt = np.full(4, 7, dtype=np.uint32); idx = np.full((4, 2), 7, dtype=np.int32); msk = np.full((4, 2), 7, dtype=np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)          # noqa: E731
    untouched = lambda: bool(np.all(cnt == 7) and np.all(idx == 7) and np.all(msk == 7))      # noqa: E731

    def raw(h, target, n, a, k, options, stats=None):
        rc = L.lib().sr_overlap_triangles(h, target, n, p(a), k, p(cnt), p(idx), p(msk), options, p(stats))
        return rc, (L.lib().sr_last_error().decode() if rc else "")

    d_q = torch.zeros((4, 3, 3), dtype=torch.float64, device=DEV)
    d_idx = torch.full((4, 2), 7, dtype=torch.int32, device=DEV)

    def raw_device(h, target, n, a, k, options):
        rc = L.lib().sr_overlap_triangles_device(h, target, n, None if a is None else C.c_void_p(a.data_ptr()), k, None, C.c_void_p(d_idx.data_ptr()), None, options,
                                                 None, None)
        return rc, (L.lib().sr_last_error().decode() if rc else "")

    bare = sa.GpuScene(0)
    unbuilt = sa.GpuScene(0)
    unbuilt.set_triangles(*sc.tris)
    bvh, vox, root, tree, brute = sa.MODE_BVH, L.TARGET_VOXELS, L.TARGET_ROOT, sa.MODE_REF_TREE, sa.MODE_BRUTE
    tree_text = ("sr_overlap_triangles: SR_MODE_REF_TREE has no overlap query (a triangle lives in several leaves of the reference tree and would be listed twice); "
                 "use SR_MODE_BVH or SR_MODE_BRUTE")
    table = [
        ((None, bvh, 4, 2, 0), L.SR_ERR_INVALID_ARG, "sr_overlap_triangles: the scene is NULL"),
        ((g._h, bvh, -1, 2, 0), L.SR_ERR_INVALID_ARG, "sr_overlap_triangles: n is negative"),
        ((g._h, bvh, 4, -1, 0), L.SR_ERR_INVALID_ARG, "sr_overlap_triangles: max_hits must be 0 .. SR_HITS_MAX (64)"),
        ((g._h, bvh, 4, 65, 0), L.SR_ERR_INVALID_ARG, "sr_overlap_triangles: max_hits must be 0 .. SR_HITS_MAX (64)"),
        ((g._h, bvh, 4, 2, 2), L.SR_ERR_INVALID_ARG, "sr_overlap_triangles: unknown option bits (SR_POINTS_COHERENT and SR_OVERLAP_ANY are the options)"),
        ((g._h, bvh, 4, 2, 4), L.SR_ERR_INVALID_ARG, "sr_overlap_triangles: SR_OVERLAP_ANY answers with a count of 0 or 1 and keeps no rows: max_hits must be 0"),
        ((g._h, vox, 4, 2, 0), L.SR_ERR_UNSUPPORTED, "sr_overlap_triangles: the voxel grid (SR_TARGET_VOXELS) has no triangles to cross"),
        ((g._h, root | bvh, 4, 2, 0), L.SR_ERR_UNSUPPORTED,
         "sr_overlap_triangles: the extra geometry (SR_TARGET_ROOT) is not made of triangles with indices; pass the mode alone"),
        ((g._h, tree, 4, 2, 0), L.SR_ERR_UNSUPPORTED, tree_text),
        ((bare._h, bvh, 4, 2, 0), L.SR_ERR_NO_MODEL, "sr_overlap_triangles: the scene has no model (sr_set_triangles, sr_load_3ds)"),
        ((unbuilt._h, bvh, 4, 2, 0), L.SR_ERR_NOT_BUILT, "SR_MODE_BVH needs sr_build(1 << SR_MODE_BVH)"),
    ]
    for (h, target, n, k, options), code, message in table:
        assert raw(h, target, n, q, k, options) == (code, message), message
        assert raw_device(h, target, n, d_q, k, options) == (code, message), message
        assert untouched()
    assert raw(g._h, bvh, 4, None, 2, 0)[0] == L.SR_ERR_INVALID_ARG and raw_device(g._h, bvh, 4, None, 2, 0)[0] == L.SR_ERR_INVALID_ARG
    torch.cuda.synchronize(DEV)
    assert bool((d_idx == 7).all())
    stats = np.full(4, 77, dtype=np.uint64)
    before = g.ray_stats().copy()
    for target in MODES:
        assert raw(g._h, target, 0, q, 2, 1, stats) == (0, "")
        assert raw(g._h, target, 0, None, 0, 4) == (0, "")
        assert raw_device(g._h, target, 0, None, 2, 0) == (0, "")
    assert untouched() and np.all(stats == 77) and np.array_equal(g.ray_stats(), before)
    # brute force on a model without a tree is fine
    got = call(unbuilt, brute, sc.queries[:300], 4)
    assert same(got, {k: v[:300] for k, v in sc.model.want(4).items()})


# ---- 9. a refit, and a two-part scene ----
def test_after_a_refit_the_answers_equal_a_fresh_build(scenes):
    sc = scenes("torus")
    v9, argb, lo, hi = sc.tris
    g = sa.GpuScene(0)
    g.set_triangles(v9, argb, lo, hi)
    g.build((sa.MODE_BVH,), on_device=True)
    before = call(g, sa.MODE_BVH, sc.queries, 4)
    assert same(before, sc.model.want(4))
    moved = np.ascontiguousarray(v9 + (hi - lo) * 0.01)                      # the torus moved by 1 % of the box
    g.refit_triangles_device(torch.from_numpy(moved).to(DEV), None, lo, hi)
    torch.cuda.synchronize(DEV)
    fresh = sa.GpuScene(0)
    fresh.set_triangles(moved, argb, lo, hi)
    fresh.build((sa.MODE_BVH,), on_device=True)
    for k, out, any_hit in ((4, KEYS, False), (64, KEYS, False), (4, ROWS, False), (0, ("count",), True)):
        after = call(g, sa.MODE_BVH, sc.queries, k, want=out, any_hit=any_hit)
        assert same(after, call(fresh, sa.MODE_BVH, sc.queries, k, want=out, any_hit=any_hit))
        assert same(after, call(fresh, sa.MODE_BRUTE, sc.queries, k, want=out, any_hit=any_hit))
        assert same(after, call(g, sa.MODE_BRUTE, sc.queries, k, want=out, any_hit=any_hit))
    assert not same(call(g, sa.MODE_BVH, sc.queries, 4), before)
    want = om.overlap_rows(sc.queries[:512], moved).rows(4)
    assert same(call(g, sa.MODE_BVH, sc.queries[:512], 4), want)
    assert (want["count"] > 0).sum() > 40                                    # (the unmoved `self` queries now cross the moved mesh)


def test_a_two_part_scene_gives_the_single_scene_answer(scenes):
    sc = scenes("cube")
    g1 = sc.gpu(True)
    g = sc.gpu(None, devices=[0, 0])
    assert g.device_count() == 2
    for mode in MODES:
        stats = np.zeros(4, dtype=np.uint64)
        got = call(g, mode, sc.queries, 4, stats=stats)
        assert same(got, call(g1, mode, sc.queries, 4)) and same(got, sc.model.want(4))
        assert stats[0] == sc.n and np.array_equal(g.ray_stats()[:4], stats)
        dev, _ = run_device(g, mode, sc.queries, 4)
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
    want = sc.model.want(4)
    first = np.asarray(g.render(f)[0]).view(np.uint32).ravel().copy()
    assert same(call(g, sa.MODE_BVH, sc.queries, 4), want)
    for _ in range(2):
        assert np.array_equal(np.asarray(g.render(f)[0]).view(np.uint32).ravel(), first)
        assert same(call(g, sa.MODE_BVH, sc.queries, 4, want=ROWS, coherent=True), want)
    assert len(set(first.tolist())) > 100
