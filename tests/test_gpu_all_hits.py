"""All hits along a ray, nearest first, with a count (sr_all_hits_rays) on the GPU.  Every comparison is an exact equality over every ray and
every output, and every output of every call lies between guard bytes (0x5A, 64 before and 64 behind) that are checked afterwards: the call
against the model of tests/all_hits_model.py (the oracle's one-triangle and one-primitive scenes), limits of every kind, the K-nearest form
(count == NULL) against the counting form, the schedules and passes against each other, the device variant against the host variant, the
relations to sr_occluded_rays and sr_nearest_rays, irregular rays against the library's literal walk on one-triangle scenes, the refusals, and
frames around the call against themselves.  Scenes and ray sets: tests/all_hits_cases.py (what they hold is pinned on the CPU in
tests/test_all_hits_model.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import all_hits_cases as ahc
import all_hits_model as ahm
import gbuffer_cases as gbc
import occluded_rays_cases as occ
import softray_amd as sa

pytestmark = pytest.mark.gpu
L = sa._lib
DEV = torch.device("cuda", 0)
GUARD = 0x5A
PAD = 64
KS = (1, 2, 5, 64)
NP_TYPES = dict(count=np.uint32, index=np.int32, ray_frac=np.float64)
KEYS = ("count", "index", "ray_frac")


class Scene:
    """One scene on the device (host-built and device-built own BVH) and its model."""

    def __init__(self, name):
        self.name = name
        self.tris, self.prims = ahc.scene_data(name)
        self.gpus = {}
        self.cands = {}

    def gpu(self, on_device=None):
        if on_device not in self.gpus:
            g = sa.GpuScene(0)
            g.set_triangles(*self.tris)
            if self.prims:
                g.set_extra(list(self.prims))
            g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=on_device)
            self.gpus[on_device] = g
        return self.gpus[on_device]

    def builds(self):
        return (None,) if self.name == "small" else (False, True)           # (at most 64 triangles: the library builds on the host by itself)

    def any_gpu(self):
        return self.gpu(self.builds()[-1])

    def model(self, name, brute, root):
        """(the candidates of the set's regular rays, computed once and left unchanged; the mask of those rays)."""
        rs = ahc.ray_set(self.name, name)
        reg = ahc.regular(rs, None)
        a, b = np.ascontiguousarray(rs.starts[reg]), np.ascontiguousarray(rs.D[reg])
        key = (name, brute, root)
        if key not in self.cands:
            if root:                                                          # (the triangles' and the elements' answers are shared between the targets)
                if (name, "extra") not in self.cands:
                    empty = (np.zeros((0, 9)), np.zeros(0, dtype=np.uint32), self.tris[2], self.tris[3])
                    self.cands[(name, "extra")] = ahm.Candidates(empty, self.prims, a, b, True)
                self.cands[key] = ahm.merged(self.cands[(name, "extra")], self.model(name, brute, False)[0])
            else:
                self.cands[key] = ahm.Candidates(self.tris, (), a, b, brute)
        return self.cands[key], reg


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Scene(name)
        return made[name]
    return get


def guarded(shape, dtype):
    raw = np.full(PAD + int(np.prod(shape)) * np.dtype(dtype).itemsize + PAD, GUARD, dtype=np.uint8)
    return raw


def view(raw, shape, dtype):
    return raw[PAD:raw.size - PAD].view(dtype).reshape(shape)


def guards_ok(raw):
    return bool(np.all(raw[:PAD] == GUARD) and np.all(raw[-PAD:] == GUARD))


def options_of(rs, coherent=False):
    return (L.RAYS_ENDPOINTS if rs.endpoints else 0) | (L.RAYS_COHERENT if coherent else 0)


def call(g, target, rs, K, limits=None, want=KEYS, coherent=False, stats=None):
    """sr_all_hits_rays with the outputs of `want` between guard bytes (the others NULL): a dict of copies."""
    n = rs.n
    shapes = dict(count=(n,), index=(n, K), ray_frac=(n, K))
    raws = {k: guarded(shapes[k], NP_TYPES[k]) for k in want if not (K == 0 and k != "count")}
    ptr = lambda k: C.c_void_p(raws[k].ctypes.data + PAD) if k in raws else None          # noqa: E731
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                      # noqa: E731
    rc = L.lib().sr_all_hits_rays(g._h, target, n, p(rs.starts), p(rs.dirs), p(limits), K, ptr("count"), ptr("index"), ptr("ray_frac"),
                                  options_of(rs, coherent), p(stats))
    assert rc == 0, L.lib().sr_last_error().decode()
    assert all(guards_ok(r) for r in raws.values()), "guard bytes"
    return {k: view(raws[k], shapes[k], NP_TYPES[k]).copy() for k in raws}


def take(res, mask):
    return {k: v[mask] for k, v in res.items()}


def want_rows(lists, K, keys=KEYS):
    r = ahm.rows(lists, K)
    return {k: r[k] for k in keys if not (K == 0 and k != "count")}


def same(got, want):
    return set(got) == set(want) and ahm.same_rows(got, want, tuple(got))


def with_hook(g, hook, fn):
    g.debug_set(L.DBG_KERNEL_SWITCH, hook)
    try:
        return fn()
    finally:
        g.debug_set(L.DBG_KERNEL_SWITCH, -1)


def targets_of(sc):
    roots = (False, True) if sc.prims else (False,)
    return [(brute, root) for brute in (False, True) for root in roots]


def target_of(brute, root):
    return (sa.MODE_BRUTE if brute else sa.MODE_BVH) | (L.TARGET_ROOT if root else 0)


# ---- 1. the model, for the regular rays of every set ----
@pytest.mark.parametrize("scene", ahc.SCENES)
def test_equals_the_model(scenes, scene):
    sc = scenes(scene)
    hits = over = extra = 0
    for name in ahc.sets_of(scene):
        rs = ahc.ray_set(scene, name)
        for brute, root in targets_of(sc):
            cand, reg = sc.model(name, brute, root)
            lists = cand.lists()
            for on_device in ((sc.builds()[-1],) if brute else sc.builds()):
                g = sc.gpu(on_device)
                for K in (0,) + KS:
                    got = call(g, target_of(brute, root), rs, K)
                    assert same(take(got, reg), want_rows(lists, K)), (name, brute, root, on_device, K)
                    if K == 64:
                        hits += int(got["count"].sum())
                        extra += int((got["index"] <= -2).sum())
                    over += int((got["count"] > K).sum()) if K else 0
    assert hits > 1000 and over > 100
    assert (extra > 50) == (scene == "cube")


# ---- 2. limits ----
def rotated(lists):
    """The twelve kinds of limit in rotation around every ray's first ray_frac (1.0 where it has none)."""
    return occ.rotated_limits(np.array([f[0] if f.shape[0] else 1.0 for f, _ in lists]))


@pytest.mark.parametrize("scene", ahc.SCENES)
def test_limits_of_every_kind(scenes, scene):
    sc = scenes(scene)
    names = {"small": ("segments", "far", "probes"), "cube": ("segments", "far", "shadow"), "layers": ahc.LAYER_SETS}[scene]
    cut = 0
    for name in names:
        rs = ahc.ray_set(scene, name)
        for brute, root in targets_of(sc):
            cand, reg = sc.model(name, brute, root)
            assert reg.all()
            free = cand.lists()
            variants = [rotated(free)]
            if rs.endpoints:
                variants.append(np.full(rs.n, 1.0))                           # "up to the end point"
            if scene == "layers":                                             # the middle hit of every ray, and just below it
                mid = np.array([f[(f.shape[0] + 1) // 2 - 1] if f.shape[0] else 1.0 for f, _ in free])
                variants += [mid, np.nextafter(mid, -np.inf)]
            g = sc.any_gpu()
            for v, lim in enumerate(variants):
                lists = cand.lists(lim)
                for K in (0, 2, 64):
                    got = call(g, target_of(brute, root), rs, K, limits=lim)
                    assert same(got, want_rows(lists, K)), (name, brute, root, v, K)
                cut += sum(a[0].shape[0] - b[0].shape[0] for a, b in zip(free, lists))
            if scene == "layers":                                             # the middle hit counts, the one below it does not
                a, b = (np.array([f.shape[0] for f, _ in cand.lists(x)]) for x in variants[-2:])
                has = np.array([f.shape[0] > 0 for f, _ in free])
                assert (a[has] > b[has]).all()
    assert cut > 500


# ---- 3. count == NULL (the walk may cull at the K-th hit) against count != NULL: the same rows ----
@pytest.mark.parametrize("scene", ahc.SCENES)
def test_without_count_the_rows_are_the_same(scenes, scene):
    sc = scenes(scene)
    names = {"small": ("segments", "far", "irregular"), "cube": ("segments", "far", "irregular_ends"), "layers": ahc.LAYER_SETS}[scene]
    for name in names:
        rs = ahc.ray_set(scene, name)
        lim = rs.limits.get("rot")
        for brute, root in targets_of(sc):
            for on_device in ((sc.builds()[-1],) if brute else sc.builds()):
                g = sc.gpu(on_device)
                for limits in (None, lim) if lim is not None else (None,):
                    for K in KS:
                        full = call(g, target_of(brute, root), rs, K, limits=limits)
                        rows = call(g, target_of(brute, root), rs, K, limits=limits, want=("index", "ray_frac"))
                        assert same(rows, {k: full[k] for k in ("index", "ray_frac")}), (name, brute, root, on_device, K)
                        one = call(g, target_of(brute, root), rs, K, limits=limits, want=("index",))      # ray_frac rows in the scene's scratch
                        assert same(one, {"index": full["index"]}), (name, brute, root, on_device, K)
                    st = np.full(4, 77, dtype=np.uint64)
                    assert call(g, target_of(brute, root), rs, 5, limits=limits, want=(), stats=st) == {}      # all NULL: runs for the statistics
                    assert st[0] == rs.n


def test_the_k_nearest_form_walks_less(scenes):
    sc = scenes("layers")
    g = sc.any_gpu()
    rs = ahc.ray_set("layers", "through")
    a, b = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    call(g, sa.MODE_BVH, rs, 2, stats=a)
    call(g, sa.MODE_BVH, rs, 2, want=("index", "ray_frac"), stats=b)
    assert a[0] == b[0] == rs.n and b[1] < a[1] and b[2] < a[2]               # fewer records and fewer nodes fetched


# ---- 4. order and pass independence ----
@pytest.mark.parametrize("scene", ahc.SCENES)
def test_schedules_and_passes_agree(scenes, scene):
    sc = scenes(scene)
    names = {"small": ("segments", "irregular", "n1", "n63", "n64", "n65", "n449"), "cube": ("probes", "irregular_ends", "n1", "n63", "n64", "n65", "n449"),
             "layers": ("through", "oblique", "edges")}[scene]
    for name in names:
        rs = ahc.ray_set(scene, name)
        lim = rs.limits.get("rot")
        for root in ((False, True) if sc.prims else (False,)):
            target = target_of(False, root)
            for on_device in sc.builds():
                g = sc.gpu(on_device)
                for K, want in ((5, KEYS), (5, ("index", "ray_frac")), (0, ("count",))):
                    base = call(g, target, rs, K, limits=lim, want=want)
                    assert same(call(g, target, rs, K, limits=lim, want=want, coherent=True), base), (name, "coherent")
                    for hook in (50, 51):                                     # input order; every ray through the per-record loop
                        assert same(with_hook(g, hook, lambda: call(g, target, rs, K, limits=lim, want=want)), base), (name, hook)
                    for band in (64, 100):
                        g.debug_set(L.DBG_BAND_SAMPLES, band)
                        try:
                            assert same(call(g, target, rs, K, limits=lim, want=want), base), (name, band)
                            assert same(call(g, target, rs, K, limits=lim, want=want, coherent=True), base), (name, band, "coherent")
                        finally:
                            g.debug_set(L.DBG_BAND_SAMPLES, -1)
    g = sc.any_gpu()
    rs = ahc.ray_set(scene, names[0])
    g.debug_set(L.DBG_BAND_SAMPLES, 100)
    g.reset_kernel_times()
    g.debug_set(L.DBG_KERNEL_TIMING, 1)
    try:
        call(g, sa.MODE_BVH, rs, 5)
        times = g.kernel_times()
    finally:
        g.debug_set(L.DBG_BAND_SAMPLES, -1)
        g.debug_set(L.DBG_KERNEL_TIMING, -1)
    passes = (rs.n + 99) // 100
    assert times["k_all_hits"][1] == passes and times["k_all_hits_sort"][1] == passes


# ---- 5. the device variant on a stream of the caller's ----
def run_device(g, target, rs, K, limits, want=KEYS, stream=None, stats=False, coherent=False):
    n = rs.n
    shapes = dict(count=(n,), index=(n, K), ray_frac=(n, K))
    d_starts, d_dirs = torch.from_numpy(rs.starts).to(DEV), torch.from_numpy(rs.dirs).to(DEV)
    d_lim = torch.from_numpy(limits).to(DEV) if limits is not None else None
    d_out = {k: torch.full((PAD + int(np.prod(shapes[k])) * np.dtype(NP_TYPES[k]).itemsize + PAD,), GUARD, dtype=torch.uint8, device=DEV) for k in want}
    d_stats = torch.full((24,), -1, dtype=torch.int64, device=DEV) if stats else None
    torch.cuda.synchronize(DEV)
    ptr = {k: (d_out[k].data_ptr() + PAD if k in d_out else 0) for k in KEYS}
    g.all_hits_device(target, n, d_starts.data_ptr(), d_dirs.data_ptr(), d_lim.data_ptr() if d_lim is not None else 0, K, ptr["count"], ptr["index"],
                      ptr["ray_frac"], endpoints=rs.endpoints, coherent=coherent, stream=stream if stream is not None else 0,
                      d_stats_ptr=d_stats.data_ptr() if stats else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize(DEV)
    res = {}
    for k in want:
        raw = d_out[k].cpu().numpy()
        assert guards_ok(raw), "guard bytes"
        res[k] = view(raw, shapes[k], NP_TYPES[k]).copy()
    assert np.array_equal(d_starts.cpu().numpy().view(np.uint64), rs.starts.view(np.uint64))
    assert np.array_equal(d_dirs.cpu().numpy().view(np.uint64), rs.dirs.view(np.uint64))
    return res, (d_stats.cpu().numpy().view(np.uint64) if stats else None)


@pytest.mark.parametrize("scene,name", [("cube", "irregular"), ("cube", "n65"), ("layers", "far_through"), ("layers", "edges")])
def test_device_variant_on_a_stream_guards_and_statistics(scenes, scene, name):
    sc = scenes(scene)
    g = sc.any_gpu()
    rs = ahc.ray_set(scene, name)
    lim = rs.limits.get("rot")
    st = torch.cuda.Stream(DEV)
    for brute, root in targets_of(sc):
        target = target_of(brute, root)
        for K in (3, 64):
            stats4 = np.zeros(4, dtype=np.uint64)
            host = call(g, target, rs, K, limits=lim, stats=stats4)
            last = g.ray_stats()
            assert np.array_equal(last[:4], stats4) and not last[4:].any() and stats4[0] == rs.n
            got, stats = run_device(g, target, rs, K, lim, stream=st, stats=True)
            assert same(got, host), (brute, root, K)
            assert np.array_equal(stats, last)
            used = np.arange(K)[None, :] < np.minimum(host["count"], K)[:, None]
            assert np.all(got["index"][~used] == -1) and np.all(got["ray_frac"][~used].view(np.uint64) == 0)      # unused slots: -1 and +0.0
            assert np.all(got["index"][used] != -1)
            rows, none = run_device(g, target, rs, K, lim, want=("index", "ray_frac"), coherent=True)
            assert none is None and same(rows, {k: host[k] for k in ("index", "ray_frac")})
            cnt, _ = run_device(g, target, rs, 0, lim, want=("count",), stream=st)
            assert same(cnt, {"count": host["count"]})


# ---- 6. relations to the sibling calls ----
@pytest.mark.parametrize("scene", ahc.SCENES)
def test_relations_to_occluded_and_nearest(scenes, scene):
    sc = scenes(scene)
    g = sc.any_gpu()
    untied_checked = 0
    for name in ahc.sets_of(scene):
        rs = ahc.ray_set(scene, name)
        for brute, root in targets_of(sc):
            target = target_of(brute, root)
            variants = [rs.limits["rot"]] if "rot" in rs.limits else [np.full(rs.n, 1.0), np.full(rs.n, np.inf)]
            for lim in variants:
                got = call(g, target, rs, 2, limits=lim)
                occluded = g.occluded(target, rs.starts, rs.dirs, limits=lim, endpoints=rs.endpoints)
                assert np.array_equal(got["count"] > 0, occluded.astype(bool)), (name, brute, root, "occluded")
                near = g.nearest(target, rs.starts, rs.dirs, limits=lim, endpoints=rs.endpoints)
                hit = near["hit"].astype(bool)
                assert np.array_equal(got["count"] > 0, hit), (name, brute, root, "hit")
                assert np.array_equal(got["ray_frac"][:, 0].view(np.uint64), near["ray_frac"].view(np.uint64)), (name, brute, root, "ray_frac")
                untied = hit & ~((got["count"] > 1) & (got["ray_frac"][:, 0] == got["ray_frac"][:, 1]))
                on_tri = got["index"][:, 0] >= 0
                assert np.array_equal(got["index"][untied & on_tri, 0], near["tri_index"][untied & on_tri]), (name, brute, root, "tri_index")
                assert np.all(near["tri_index"][untied & ~on_tri & hit] == -1)
                untied_checked += int((untied & on_tri).sum())
    assert untied_checked > 500


# ---- 7. irregular rays: the library's literal walk on one-triangle scenes is the same predicate with no fp32 stage ----
def test_irregular_rays_equal_the_literal_walk_on_one_triangle_scenes(scenes):
    sc = scenes("small")
    g = sc.any_gpu()
    v9, argb, lo, hi = sc.tris
    v9 = np.ascontiguousarray(v9, dtype=np.float64).reshape(-1, 9)
    singles = []
    for j in range(v9.shape[0]):
        one = sa.GpuScene(0)
        one.set_triangles(v9[j:j + 1], argb[j:j + 1], lo, hi)
        one.build((sa.MODE_REF_TREE,))
        singles.append(one)
    seen = 0
    for name in ("irregular", "irregular_ends"):
        rs = ahc.ray_set("small", name)
        irregular = ~ahc.regular(rs, None)
        assert irregular.sum() >= 40
        for brute in (False, True):
            mode = sa.MODE_BRUTE if brute else sa.MODE_REF_TREE
            res = [one.trace(mode, rs.starts, rs.D) for one in singles]
            cand = ahm.Candidates.__new__(ahm.Candidates)
            cand.n = rs.n
            cand.hit = np.array([r["hit"].astype(bool) for r in res])
            cand.frac = np.array([r["ray_frac"] for r in res])
            cand.index = np.arange(len(res), dtype=np.int64)
            cand.key = cand.index + 2 ** 31
            for lim in (None, rs.limits["rot"]):
                lists = cand.lists(lim)
                for K in (0, 2, 64):
                    for want in (KEYS, ("index", "ray_frac")):
                        got = call(g, target_of(brute, False), rs, K, limits=lim, want=want)
                        assert same(got, want_rows(lists, K, want)), (name, brute, K, want)      # every ray of the set, the regular ones too
                seen += sum(lists[i][0].shape[0] for i in np.flatnonzero(irregular))
    assert seen > 0


# ---- 8. refusals ----
def test_refusals_in_the_headers_order(scenes):
    sc = scenes("cube")
    g = sc.any_gpu()
    s = np.zeros((4, 3)); d = np.ones((4, 3))
    cnt = np.full(4, 7, dtype=np.uint32); idx = np.full((4, 4), 7, dtype=np.int32); rf = np.full((4, 4), 7.0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)          # noqa: E731
    untouched = lambda: bool(np.all(cnt == 7) and np.all(idx == 7) and np.all(rf == 7.0))      # noqa: E731

    def raw(h, target, n, a, b, k, options, stats=None):
        rc = L.lib().sr_all_hits_rays(h, target, n, p(a), p(b), None, k, p(cnt), p(idx), p(rf), options, p(stats))
        return rc, (L.lib().sr_last_error().decode() if rc else "")

    bare = sa.GpuScene(0)                                                    # no model
    unbuilt = sa.GpuScene(0)                                                 # a model, no tree
    unbuilt.set_triangles(*sc.tris)
    bvh, vox, tree, brute = sa.MODE_BVH, L.TARGET_VOXELS, sa.MODE_REF_TREE, sa.MODE_BRUTE
    options_text = "sr_all_hits_rays: unknown option bits (SR_RAYS_COHERENT and SR_RAYS_ENDPOINTS are the options)"
    k_text = "sr_all_hits_rays: max_hits must be 0 .. SR_HITS_MAX (64)"
    vox_text = "sr_all_hits_rays: the voxel grid (SR_TARGET_VOXELS) has no tree to walk and its hits have rayFrac 0; use sr_trace_rays"
    tree_text = ("sr_all_hits_rays: SR_MODE_REF_TREE has no notion of all hits (the literal walk ends in the first leaf that holds a hit inside its box, "
                 "and a triangle lives in several leaves); use SR_MODE_BVH or SR_MODE_BRUTE")
    table = [
        ((None, vox, -1, None, None, 65, 4), L.SR_ERR_INVALID_ARG, "sr_all_hits_rays: the scene is NULL"),
        ((bare._h, vox, -1, None, None, 65, 4), L.SR_ERR_INVALID_ARG, "sr_all_hits_rays: n is negative"),
        ((bare._h, vox, 4, None, d, 65, 4), L.SR_ERR_INVALID_ARG, "sr_all_hits_rays: starts and dirs must not be NULL when n > 0"),
        ((bare._h, vox, 4, s, d, 65, 4), L.SR_ERR_INVALID_ARG, k_text),
        ((bare._h, vox, 4, s, d, 4, 4), L.SR_ERR_INVALID_ARG, options_text),
        ((bare._h, vox | tree, 4, s, d, 4, 3), L.SR_ERR_UNSUPPORTED, vox_text),
        ((bare._h, tree | L.TARGET_ROOT, 4, s, d, 4, 0), L.SR_ERR_UNSUPPORTED, tree_text),
        ((g._h, tree, 4, s, d, 4, 0), L.SR_ERR_UNSUPPORTED, tree_text),
        ((bare._h, bvh, 4, s, d, 4, 0), L.SR_ERR_NO_MODEL, "sr_all_hits_rays: the scene has no model (sr_set_triangles, sr_load_3ds)"),
        ((unbuilt._h, bvh, 4, s, d, 4, 0), L.SR_ERR_NOT_BUILT, "SR_MODE_BVH needs sr_build(1 << SR_MODE_BVH)"),
    ]
    for args, code, message in table:
        assert raw(*args) == (code, message), message
        assert untouched()
    # the device variant refuses the same way, with the same messages
    d_s, d_d = torch.zeros((4, 3), dtype=torch.float64, device=DEV), torch.ones((4, 3), dtype=torch.float64, device=DEV)
    d_cnt = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    d_idx = torch.full((4, 4), 7, dtype=torch.int32, device=DEV)
    d_rf = torch.full((4, 4), 7.0, dtype=torch.float64, device=DEV)
    v = lambda t: None if t is None else C.c_void_p(t.data_ptr())              # noqa: E731

    def raw_device(h, target, n, a, b, k, options):
        rc = L.lib().sr_all_hits_rays_device(h, target, n, v(a), v(b), None, k, v(d_cnt), v(d_idx), v(d_rf), options, None, None)
        return rc, (L.lib().sr_last_error().decode() if rc else "")

    for args, code, message in (
            ((None, bvh, 4, d_s, d_d, 4, 0), L.SR_ERR_INVALID_ARG, "sr_all_hits_rays: the scene is NULL"),
            ((g._h, bvh, -1, d_s, d_d, 4, 0), L.SR_ERR_INVALID_ARG, "sr_all_hits_rays: n is negative"),
            ((g._h, bvh, 4, d_s, None, 4, 0), L.SR_ERR_INVALID_ARG, "sr_all_hits_rays: starts and dirs must not be NULL when n > 0"),
            ((g._h, bvh, 4, d_s, d_d, -1, 0), L.SR_ERR_INVALID_ARG, k_text),
            ((g._h, bvh, 4, d_s, d_d, 4, 8), L.SR_ERR_INVALID_ARG, options_text),
            ((g._h, vox, 4, d_s, d_d, 4, 0), L.SR_ERR_UNSUPPORTED, vox_text),
            ((g._h, tree, 4, d_s, d_d, 4, 0), L.SR_ERR_UNSUPPORTED, tree_text),
            ((bare._h, bvh, 4, d_s, d_d, 4, 0), L.SR_ERR_NO_MODEL, "sr_all_hits_rays: the scene has no model (sr_set_triangles, sr_load_3ds)"),
            ((unbuilt._h, bvh, 4, d_s, d_d, 4, 0), L.SR_ERR_NOT_BUILT, "SR_MODE_BVH needs sr_build(1 << SR_MODE_BVH)")):
        assert raw_device(*args) == (code, message), message
    torch.cuda.synchronize(DEV)
    assert bool((d_cnt == 7).all()) and bool((d_idx == 7).all()) and bool((d_rf == 7.0).all())
    # n == 0 that passes every check: SR_OK, nothing is touched -- with arrays and without
    stats = np.full(4, 77, dtype=np.uint64)
    before = g.ray_stats().copy()
    for target in (bvh, bvh | L.TARGET_ROOT, brute):
        assert raw(g._h, target, 0, s, d, 4, 3, stats) == (0, "")
        assert raw(g._h, target, 0, None, None, 0, 0) == (0, "")
        assert raw_device(g._h, target, 0, None, None, 64, 0) == (0, "")
    assert untouched() and np.all(stats == 77) and np.array_equal(g.ray_stats(), before)
    with pytest.raises(sa.SoftrayError):
        g.all_hits(bvh, s, d, max_hits=65)
    res = g.all_hits(bvh, s, d)                                              # the wrapper's defaults: K = 8, with the count
    assert res["index"].shape == (4, 8) and res["ray_frac"].shape == (4, 8) and res["count"].shape == (4,)


# ---- 9. state ----
def as_sr(frame):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = sa.MODE_BVH
    return f


def test_a_shadowed_frame_before_and_after_the_call_is_the_same_frame(scenes):
    sc = scenes("cube")
    g = sa.GpuScene(0)                                                       # a scene of its own: the frames' hints stay here
    g.set_triangles(*sc.tris)
    g.set_extra(list(sc.prims))
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=True)
    f = as_sr(gbc.frame_of(("cube", "out", 200, 160, None, 1, False), shadows=True))
    rs = ahc.ray_set("cube", "segments")
    target = sa.MODE_BVH | L.TARGET_ROOT
    cand, reg = sc.model("segments", False, True)
    want = want_rows(cand.lists(rs.limits["rot"]), 5)
    first = np.asarray(g.render(f)[0]).view(np.uint32).ravel().copy()
    assert same(call(g, target, rs, 5, limits=rs.limits["rot"]), want)
    for _ in range(2):
        assert np.array_equal(np.asarray(g.render(f)[0]).view(np.uint32).ravel(), first)
        assert same(call(g, target, rs, 5, limits=rs.limits["rot"], coherent=True), want)
    assert len(set(first.tolist())) > 100


def test_frame_call_frame_on_three_streams_is_bit_stable(scenes):
    """A frame on one stream, the call on another at once, a frame behind it on a third: the call reads the records a frame's set-up moves."""
    sc = scenes("cube")
    g = sc.gpu(True)
    f = as_sr(gbc.frame_of(("cube", "out", 200, 160, None, 1, False), shadows=True))
    f2 = as_sr(gbc.frame_of(("cube", "in", 200, 160, None, 1, False), shadows=True))      # another camera: its set-up moves the records again
    rs = ahc.ray_set("cube", "segments")
    target = sa.MODE_BVH | L.TARGET_ROOT
    lim = rs.limits["rot"]
    want = call(g, target, rs, 5, limits=lim)
    want_px = [np.asarray(g.render(fr)[0]).view(np.uint32).ravel().copy() for fr in (f, f2)]
    d_starts, d_dirs, d_lim = torch.from_numpy(rs.starts).to(DEV), torch.from_numpy(rs.dirs).to(DEV), torch.from_numpy(lim).to(DEV)
    s1, s2, s3 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    for _ in range(3):
        d_cnt = torch.full((rs.n,), 7, dtype=torch.int32, device=DEV)
        d_idx = torch.full((rs.n, 5), 7, dtype=torch.int32, device=DEV)
        d_rf = torch.full((rs.n, 5), 7.0, dtype=torch.float64, device=DEV)
        px = [torch.zeros(200 * 160, dtype=torch.int32, device=DEV) for _ in range(2)]
        torch.cuda.synchronize(DEV)
        g.render_device(f, px[0].data_ptr(), s1.cuda_stream)
        g.all_hits_device(target, rs.n, d_starts.data_ptr(), d_dirs.data_ptr(), d_lim.data_ptr(), 5, d_cnt.data_ptr(), d_idx.data_ptr(), d_rf.data_ptr(),
                          endpoints=rs.endpoints, stream=s2)
        g.render_device(f2, px[1].data_ptr(), s3.cuda_stream)
        torch.cuda.synchronize(DEV)
        got = dict(count=d_cnt.cpu().numpy().view(np.uint32), index=d_idx.cpu().numpy(), ray_frac=d_rf.cpu().numpy())
        assert same(got, want)
        for q, w in zip(px, want_px):
            assert np.array_equal(q.cpu().numpy().view(np.uint32), w)


# ---- 10. inside / outside on a closed mesh (the recipe of INTEGRATION.md) ----
class Rays:
    def __init__(self, starts, dirs, endpoints):
        self.starts, self.dirs, self.endpoints, self.n = np.ascontiguousarray(starts), np.ascontiguousarray(dirs), endpoints, starts.shape[0]


@pytest.mark.parametrize("mode", ["bvh", "brute"])
def test_inside_outside_on_the_torus(mode):
    import mesh_cases as mc
    g = sa.GpuScene(0)
    g.set_triangles(*mc.scene("torus"))
    g.build((sa.MODE_BVH,), on_device=True)
    target = sa.MODE_BVH if mode == "bvh" else sa.MODE_BRUTE
    p, d, inside = ahc.torus_points()
    far = p + ahc.TORUS_REACH * d
    entries = call(g, target, Rays(p, d, False), 0)["count"].astype(np.int64)
    exits = call(g, target, Rays(far, p, True), 0, limits=np.ones(p.shape[0]))["count"].astype(np.int64)
    assert np.array_equal(exits - entries, inside.astype(np.int64))
    assert (entries > 0).sum() > 20
