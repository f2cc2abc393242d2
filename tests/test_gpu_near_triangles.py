"""The triangles within reach of a point, nearest first, with a count (sr_near_triangles) on the GPU.  Every comparison is an exact equality
over every point, slot and output, and every output of every call lies between guard bytes (0x5A, 64 before and 64 behind) that are checked
afterwards: the own BVH's walk against brute force against the model of tests/near_triangles_model.py on host-built and device-built trees
for K in (0, 1, 4, 64); the K-nearest form (count NULL) against the counted rows; slot 0 against sr_closest_points; the schedules and passes
against each other; any subset of the outputs; the device variant against the host variant; brute-force statistics; refusals and the empty
batch; a refit against a fresh build; a two-part scene against the single scene; a frame around the call against itself.
Scenes, points and radii: tests/near_triangles_cases.py (what they hold is pinned on the CPU in tests/test_near_triangles_model.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import closest_points_cases as cpc
import closest_points_model as cpm
import gbuffer_cases as gbc
import near_triangles_cases as ntc
import near_triangles_model as ntm
import softray_amd as sa

pytestmark = pytest.mark.gpu
L = sa._lib
DEV = torch.device("cuda", 0)
GUARD = 0x5A
PAD = 64
KEYS = ntm.KEYS
ROWS = ("index", "dist", "pos", "uv")
MODES = (sa.MODE_BVH, sa.MODE_BRUTE)
SETS = ("none", "radii")


class Scene:
    """One scene on the device (host-built and device-built own BVH) and the model's answers (computed once, left unchanged)."""

    def __init__(self, name):
        self.name = name
        self.tris = cpc.scene(name)
        self.model = ntc.model(name)
        self.points = self.model.points
        self.n = self.points.shape[0]
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


def call(g, target, points, limits, k, want=KEYS, coherent=False, stats=None):
    """sr_near_triangles with the outputs of `want` between guard bytes (the others NULL): a dict of copies."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    n = points.shape[0]
    shp = ntm.shapes(n, k)
    raws = {key: guarded(shp[key], ntm.NP_TYPES[key]) for key in want}
    ptr = lambda key: C.c_void_p(raws[key].ctypes.data + PAD) if key in raws else None      # noqa: E731
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    rc = L.lib().sr_near_triangles(g._h, target, n, p(points), p(limits), k, ptr("count"), ptr("index"), ptr("dist"), ptr("pos"), ptr("uv"),
                                   L.POINTS_COHERENT if coherent else 0, p(stats))
    assert rc == 0, L.lib().sr_last_error().decode()
    assert all(guards_ok(r) for r in raws.values()), "guard bytes"
    return {key: view(raws[key], shp[key], ntm.NP_TYPES[key]).copy() for key in raws}


def same(got, want):
    return set(got) <= set(want) and all(ntm.same_bits(got[k], want[k]) for k in got)


def explain(got, want):
    for k in got:
        if not ntm.same_bits(got[k], want[k]):
            bad = np.flatnonzero(~np.all((got[k] == want[k]).reshape(got[k].shape[0], -1), axis=1))
            return k, bad[:8], got[k][bad[:2]], want[k][bad[:2]]
    return None


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


# ---- 1. the walk, brute force and the model, on every scene and build, with the count ----
@pytest.mark.parametrize("scene", ntc.SCENES)
def test_bvh_equals_brute_equals_the_model(scenes, scene):
    sc = scenes(scene)
    runs = [(sc.gpu(b), sa.MODE_BVH, b) for b in sc.builds()] + [(sc.any_gpu(), sa.MODE_BRUTE, "brute")]
    for which in SETS:
        limits = sc.model.limit(which)
        for k in ntc.KS:
            want = sc.model.want(which, k)
            for g, mode, label in runs:
                got = call(g, mode, sc.points, limits, k)
                assert same(got, want), (scene, which, k, label, explain(got, want))
    assert (sc.model.sets["radii"].count == 0).sum() > 500 and (sc.model.sets["radii"].count > 4).sum() > 200


# ---- 2. the K-nearest form: count NULL, the walk culls at the K-th entry, the rows stay the same ----
@pytest.mark.parametrize("scene", ntc.SCENES)
def test_the_k_nearest_form_equals_the_counted_rows(scenes, scene):
    sc = scenes(scene)
    g = sc.any_gpu()
    for which in SETS:
        limits = sc.model.limit(which)
        for k in (1, 4, 64):
            want = sc.model.want(which, k)
            for mode in MODES:
                got = call(g, mode, sc.points, limits, k, want=ROWS)
                assert set(got) == set(ROWS) and same(got, want), (scene, which, k, mode, explain(got, want))
    # the cull is at work: fewer triangles are tested without the count
    with_count, without = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    call(g, sa.MODE_BVH, sc.points, None, 4, stats=with_count)
    call(g, sa.MODE_BVH, sc.points, None, 4, want=ROWS, stats=without)
    assert without[0] == with_count[0] == sc.n and without[1] < with_count[1]


# ---- 3. slot 0 is sr_closest_points' answer, bit for bit in all four outputs ----
@pytest.mark.parametrize("scene", ntc.SCENES)
def test_slot_0_equals_closest_points(scenes, scene):
    sc = scenes(scene)
    g = sc.any_gpu()
    for which in SETS:
        limits = sc.model.limit(which)
        for mode in MODES:
            cp = g.closest_points(mode, sc.points, max_dist=limits)
            for k, want in ((1, KEYS), (1, ROWS), (4, ROWS), (64, KEYS)):
                got = call(g, mode, sc.points, limits, k, want=want)
                slot0 = dict(tri_index=got["index"][:, 0], dist=got["dist"][:, 0], pos=got["pos"][:, 0], uv=got["uv"][:, 0])
                for key in slot0:
                    assert cpm.same_bits(np.ascontiguousarray(slot0[key]), cp[key]), (scene, which, mode, k, want, key)


# ---- 4. schedules: sorted, the caller's promise, the two hooks ----
@pytest.mark.parametrize("scene", ("small", "layers", "slivers", "limit", "far_probe"))
def test_schedules_give_the_same_answers(scenes, scene):
    sc = scenes(scene)
    g = sc.any_gpu()
    for which, k, out in (("none", 4, ROWS), ("radii", 4, KEYS), ("radii", 64, KEYS), ("radii", 0, KEYS)):
        limits = sc.model.limit(which)
        want = sc.model.want(which, k)
        assert same(call(g, sa.MODE_BVH, sc.points, limits, k, want=out), want)
        assert same(call(g, sa.MODE_BVH, sc.points, limits, k, want=out, coherent=True), want)
        assert same(with_hook(g, 54, lambda: call(g, sa.MODE_BVH, sc.points, limits, k, want=out)), want)          # input order
        assert same(with_hook(g, 55, lambda: call(g, sa.MODE_BVH, sc.points, limits, k, want=out)), want)          # the per-record loop for every point
        assert same(with_hook(g, 55, lambda: call(g, sa.MODE_BVH, sc.points, limits, k, want=out, coherent=True)), want)


# ---- 5. passes ----
@pytest.mark.parametrize("scene", ("layers", "degenerate"))
def test_passes_of_100_and_257_points(scenes, scene):
    sc = scenes(scene)
    g = sc.any_gpu()
    lim = sc.model.limit("radii")
    for per_pass in (100, 257):
        for mode in MODES:
            for k, out, coherent in ((4, KEYS, False), (4, ("count", "pos"), True), (64, ROWS, False)):
                stats = np.zeros(4, dtype=np.uint64)
                got = with_pass(g, per_pass, lambda: call(g, mode, sc.points, lim, k, want=out, coherent=coherent, stats=stats))
                assert same(got, sc.model.want("radii", k)), (per_pass, mode, k, out)
                assert stats[0] == sc.n
    # the walk and the sort are recorded once per pass; brute force sorts nothing
    for mode in MODES:
        g.reset_kernel_times()
        g.debug_set(L.DBG_KERNEL_TIMING, 1)
        try:
            with_pass(g, 100, lambda: call(g, mode, sc.points, lim, 4))
            times = g.kernel_times()
        finally:
            g.debug_set(L.DBG_KERNEL_TIMING, -1)
        passes = (sc.n + 99) // 100
        assert times["k_near"][1] == passes, mode
        if mode == sa.MODE_BVH:
            assert times["k_near_sort"][1] == passes
        else:
            assert "k_near_sort" not in times
        assert "k_closest" not in times and "k_closest_sort" not in times


# ---- 6. any subset of the outputs (the rows the walk needs and the caller did not ask for live in the scene's scratch) ----
def test_any_subset_of_the_outputs(scenes):
    sc = scenes("layers")
    g = sc.any_gpu()
    lim = sc.model.limit("radii")
    for k in (4, 64):
        want = sc.model.want("radii", k)
        for r in range(len(KEYS) + 1):
            for subset in itertools.combinations(KEYS, r):
                for mode in MODES:
                    stats = np.zeros(4, dtype=np.uint64)
                    got = call(g, mode, sc.points, lim, k, want=subset, stats=stats)
                    assert set(got) == set(subset) and same(got, want), (k, subset, mode)
                    assert stats[0] == sc.n                                   # (all NULL: the call runs for the statistics)
    res = g.near_triangles(sa.MODE_BVH, sc.points, max_dist=lim, max_hits=4, want=("count", "uv"), stats=True)
    assert res["index"] is None and res["dist"] is None and res["pos"] is None and res["stats"][0] == sc.n
    assert same({k: res[k] for k in ("count", "uv")}, sc.model.want("radii", 4))
    res = g.near_triangles(sa.MODE_BRUTE, sc.points, max_hits=0)
    assert same({"count": res["count"]}, sc.model.want("none", 0)) and res["index"].shape == (sc.n, 0)


# ---- 7. the device variant ----
def run_device(g, target, points, limits, k, coherent=False, stream=None, want=KEYS):
    n = points.shape[0]
    shp = ntm.shapes(n, k)
    d_points = torch.from_numpy(np.array(points, dtype=np.float64)).to(DEV)
    d_lim = None if limits is None else torch.from_numpy(np.array(limits, dtype=np.float64)).to(DEV)
    outs = {}
    for key in want:
        outs[key] = torch.full((PAD + int(np.prod(shp[key])) * np.dtype(ntm.NP_TYPES[key]).itemsize + PAD,), GUARD, dtype=torch.uint8, device=DEV)
    d_stats = torch.full((24,), 77, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize(DEV)
    ptr = lambda key: outs[key].data_ptr() + PAD if key in outs else 0                       # noqa: E731
    g.near_triangles_device(target, n, d_points.data_ptr(), 0 if d_lim is None else d_lim.data_ptr(), k, ptr("count"), ptr("index"), ptr("dist"), ptr("pos"),
                            ptr("uv"), coherent=coherent, stream=stream if stream is not None else 0, d_stats_ptr=d_stats.data_ptr())
    torch.cuda.synchronize(DEV)
    raws = {key: v.cpu().numpy() for key, v in outs.items()}
    assert all(guards_ok(r) for r in raws.values()), "guard bytes"
    assert cpm.same_bits(d_points.cpu().numpy(), np.ascontiguousarray(points))
    return {key: view(raws[key], shp[key], ntm.NP_TYPES[key]).copy() for key in raws}, d_stats.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("scene", ("cube", "duplicates"))
def test_the_device_variant_equals_the_host_variant(scenes, scene):
    sc = scenes(scene)
    g = sc.any_gpu()
    st = torch.cuda.Stream(DEV)
    for mode in MODES:
        for which, k in (("none", 4), ("radii", 64), ("radii", 0)):
            limits = sc.model.limit(which)
            host_stats = np.zeros(4, dtype=np.uint64)
            host = call(g, mode, sc.points, limits, k, stats=host_stats)
            assert same(host, sc.model.want(which, k))
            for stream, coherent in ((None, False), (st, True)):
                dev, stats = run_device(g, mode, sc.points, limits, k, coherent=coherent, stream=stream)
                assert same(dev, host), (mode, which, k, coherent)
                assert stats[0] == sc.n and not stats[4:].any()
                if mode == sa.MODE_BRUTE:
                    assert np.array_equal(stats[:4], host_stats)
    dev, _ = run_device(g, sa.MODE_BVH, sc.points, sc.model.limit("radii"), 4, want=("dist", "uv"), stream=st)
    assert same(dev, sc.model.want("radii", 4))


# ---- 8. statistics ----
def test_brute_force_statistics_are_pinned(scenes):
    sc = scenes("layers")
    g = sc.any_gpu()
    T = sc.tris[0].shape[0]
    for k, out in ((4, KEYS), (0, ("count",)), (64, ROWS), (4, ())):
        stats = np.full(4, 77, dtype=np.uint64)
        call(g, sa.MODE_BRUTE, sc.points, sc.model.limit("radii"), k, want=out, stats=stats)
        assert list(stats) == [sc.n, sc.n * T, 0, 0]
        assert np.array_equal(g.ray_stats()[:4], stats) and not g.ray_stats()[4:].any()
    stats = np.full(4, 77, dtype=np.uint64)
    call(g, sa.MODE_BVH, sc.points, sc.model.limit("extent8"), 4, stats=stats)
    reg = int(cpm.regular(sc.points, sc.tris[2], sc.tris[3]).sum())
    assert stats[0] == sc.n and stats[2] >= reg                              # every regular point fetches the root
    assert (sc.n - reg) * T <= stats[1] < sc.n * T                           # the walk tests fewer triangles than the loop; the irregular tail tests all
    with_hook(g, 55, lambda: call(g, sa.MODE_BVH, sc.points, None, 4, stats=stats))
    assert list(stats) == [sc.n, sc.n * T, 0, 0]


# ---- 9. refusals with a device (the rest: tests/test_near_triangles_mirror.py) and the empty batch ----
def test_refusals_and_the_empty_batch_on_a_device(scenes):
    sc = scenes("cube")
    g = sc.any_gpu()
    q = np.zeros((4, 3))
    cnt = np.full(4, 7, dtype=np.uint32); idx = np.full((4, 2), 7, dtype=np.int32); dist = np.full((4, 2), 7.0); pos = np.full((4, 2, 3), 7.0); uv = np.full((4, 2, 2), 7.0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)          # noqa: E731
    untouched = lambda: bool(np.all(cnt == 7) and np.all(idx == 7) and np.all(dist == 7.0) and np.all(pos == 7.0) and np.all(uv == 7.0))      # noqa: E731

    def raw(h, target, n, a, k, options, stats=None):
        rc = L.lib().sr_near_triangles(h, target, n, p(a), None, k, p(cnt), p(idx), p(dist), p(pos), p(uv), options, p(stats))
        return rc, (L.lib().sr_last_error().decode() if rc else "")

    d_q = torch.zeros((4, 3), dtype=torch.float64, device=DEV)
    d_idx = torch.full((4, 2), 7, dtype=torch.int32, device=DEV)

    def raw_device(h, target, n, a, k, options):
        rc = L.lib().sr_near_triangles_device(h, target, n, None if a is None else C.c_void_p(a.data_ptr()), None, k, None, C.c_void_p(d_idx.data_ptr()), None, None,
                                              None, options, None, None)
        return rc, (L.lib().sr_last_error().decode() if rc else "")

    bare = sa.GpuScene(0)
    unbuilt = sa.GpuScene(0)
    unbuilt.set_triangles(*sc.tris)
    bvh, vox, root, tree, brute = sa.MODE_BVH, L.TARGET_VOXELS, L.TARGET_ROOT, sa.MODE_REF_TREE, sa.MODE_BRUTE
    tree_text = ("sr_near_triangles: SR_MODE_REF_TREE has no distance query (a triangle lives in several leaves of the reference tree and would be listed twice); "
                 "use SR_MODE_BVH or SR_MODE_BRUTE")
    table = [
        ((None, bvh, 4, 2, 0), L.SR_ERR_INVALID_ARG, "sr_near_triangles: the scene is NULL"),
        ((g._h, bvh, -1, 2, 0), L.SR_ERR_INVALID_ARG, "sr_near_triangles: n is negative"),
        ((g._h, bvh, 4, -1, 0), L.SR_ERR_INVALID_ARG, "sr_near_triangles: max_hits must be 0 .. SR_HITS_MAX (64)"),
        ((g._h, bvh, 4, 65, 0), L.SR_ERR_INVALID_ARG, "sr_near_triangles: max_hits must be 0 .. SR_HITS_MAX (64)"),
        ((g._h, bvh, 4, 2, 2), L.SR_ERR_INVALID_ARG, "sr_near_triangles: unknown option bits (SR_POINTS_COHERENT is the only option)"),
        ((g._h, vox, 4, 2, 0), L.SR_ERR_UNSUPPORTED, "sr_near_triangles: the voxel grid (SR_TARGET_VOXELS) has no triangles to be near to"),
        ((g._h, root | bvh, 4, 2, 0), L.SR_ERR_UNSUPPORTED,
         "sr_near_triangles: the extra geometry (SR_TARGET_ROOT) has no triangle indices to list; pass the mode alone"),
        ((g._h, tree, 4, 2, 0), L.SR_ERR_UNSUPPORTED, tree_text),
        ((bare._h, bvh, 4, 2, 0), L.SR_ERR_NO_MODEL, "sr_near_triangles: the scene has no model (sr_set_triangles, sr_load_3ds)"),
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
        assert raw(g._h, target, 0, None, 0, 0) == (0, "")
        assert raw_device(g._h, target, 0, None, 2, 0) == (0, "")
    assert untouched() and np.all(stats == 77) and np.array_equal(g.ray_stats(), before)
    # brute force on a model without a tree is fine
    got = call(unbuilt, brute, sc.points[:300], None, 4)
    assert same(got, {k: v[:300] for k, v in sc.model.want("none", 4).items()})


# ---- 10. a refit, and a two-part scene ----
def test_after_a_refit_the_answers_equal_a_fresh_build(scenes):
    sc = scenes("cube")
    v9, argb, lo, hi = sc.tris
    g = sa.GpuScene(0)
    g.set_triangles(v9, argb, lo, hi)
    g.build((sa.MODE_BVH,), on_device=True)
    before = call(g, sa.MODE_BVH, sc.points, None, 4)
    assert same(before, sc.model.want("none", 4))
    moved = np.ascontiguousarray(v9 * np.array([0.9, 0.8, 0.95]) + np.array([0.02, -0.03, 0.01]))
    g.refit_triangles_device(torch.from_numpy(moved).to(DEV), None, lo, hi)
    torch.cuda.synchronize(DEV)
    fresh = sa.GpuScene(0)
    fresh.set_triangles(moved, argb, lo, hi)
    fresh.build((sa.MODE_BVH,), on_device=True)
    for limits, k, out in ((None, 4, KEYS), (sc.model.limit("extent8"), 64, KEYS), (sc.model.limit("radii"), 4, ROWS)):
        after = call(g, sa.MODE_BVH, sc.points, limits, k, want=out)
        assert same(after, call(fresh, sa.MODE_BVH, sc.points, limits, k, want=out))
        assert same(after, call(fresh, sa.MODE_BRUTE, sc.points, limits, k, want=out))
        assert same(after, call(g, sa.MODE_BRUTE, sc.points, limits, k, want=out))
    assert not same(call(g, sa.MODE_BVH, sc.points, None, 4), before)
    want = ntm.near_sets(sc.points[:512], moved)["none"].rows(4)
    assert same(call(g, sa.MODE_BVH, sc.points[:512], None, 4), want)


def test_a_two_part_scene_gives_the_single_scene_answer(scenes):
    sc = scenes("cube")
    g1 = sc.gpu(True)
    g = sc.gpu(None, devices=[0, 0])
    assert g.device_count() == 2
    lim = sc.model.limit("radii")
    for mode in MODES:
        stats = np.zeros(4, dtype=np.uint64)
        got = call(g, mode, sc.points, lim, 4, stats=stats)
        assert same(got, call(g1, mode, sc.points, lim, 4)) and same(got, sc.model.want("radii", 4))
        assert stats[0] == sc.n and np.array_equal(g.ray_stats()[:4], stats)
        dev, _ = run_device(g, mode, sc.points, lim, 4)
        assert same(dev, got)


# ---- 11. state: frames around the call ----
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
    want = sc.model.want("radii", 4)
    lim = sc.model.limit("radii")
    first = np.asarray(g.render(f)[0]).view(np.uint32).ravel().copy()
    assert same(call(g, sa.MODE_BVH, sc.points, lim, 4), want)
    for _ in range(2):
        assert np.array_equal(np.asarray(g.render(f)[0]).view(np.uint32).ravel(), first)
        assert same(call(g, sa.MODE_BVH, sc.points, lim, 4, want=ROWS, coherent=True), want)
    assert len(set(first.tolist())) > 100
