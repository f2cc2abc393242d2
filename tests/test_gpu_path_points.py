"""sr_path_points on the GPU against the CPU model (tests/path_points_model.py, which tests/test_path_points_model.py pins to the frame
model of the path-traced frames and to the reference's goldens): every comparison is an exact equality over every point.  The point sets
are those of tests/test_gpu_ao_points.py -- camera hit points in scan order, points on the extra geometry outside the cube, free points
inside and outside, zero / non-unit / reversed normals and 40 copies of one point."""
import os

import numpy as np
import pytest
import torch

import path_points_model as ppm
import pathtrace_model as ptm
import shadow_points_model as spm
import softray_amd as sa
import test_gpu_ao_points as tap
import test_gpu_shadow_points as tsp
from helpers import GOLDEN, edge_light_frame, load_obj3ds, make_frame, orc, read_bmp_rgb

pytestmark = pytest.mark.gpu
L = sa._lib
DEV = torch.device("cuda", 0)
MODES = tap.MODES
GUARD32, GUARD64 = 0x01020304, -12345.678
SEED = 1234567890
# the implementation's constants (softray_amd/csrc/sr_pipeline.hip): a chunk of the draw table is 19 200 draws = 6 400 points, one
# workgroup of the state kernel makes the start states of 64 chunks = 409 600 points, a pass holds at most 2^22 points
CHUNK_POINTS, STATE_GROUP_POINTS, MAX_PASS = 6400, 64 * 6400, 1 << 22


def path_frame(mode="tree", shading=False, extra_flags=0, seed=SEED):
    f = sa.Frame.from_buffer_copy(bytes(make_frame(16, shading=shading)))
    f.trace_mode = MODES[mode]
    f.random_seed = seed
    f.flags |= extra_flags
    return f


class Case(tap.Case):
    """The scenes and point sets of the AO points test with this call's model."""

    def geometry(self, mode):
        """(scene, target) whose trace answers a second ray as the frame's root geometry in `mode` does."""
        if mode == "brute":
            return self.brute, ppm.TRACE_ROOT_TREE
        if mode == "tree":
            return self.o, ppm.TRACE_ROOT_TREE
        if self.prims:
            return ppm.NearestWithExtras(self.o, self.extras_only), ppm.TRACE_NEAREST
        return self.o, ppm.TRACE_NEAREST

    def model(self, mode, shading, pos, nrm, color, first=0, info=None):
        scene, target = self.geometry(mode)
        return ppm.path_points(scene, target, path_frame(mode, shading), pos, nrm, color, first_sample=first, inf_scene=self.o, info=info)

    def want(self, mode, shading, first=0):
        """The model's (out, incoming, dirs, info) for the whole set, read-only."""
        k = ("path", mode, shading, first)
        if k not in self.wants:
            info = {}
            o, i, d = self.model(mode, shading, self.pos, self.nrm, self.color, first, info)
            for x in (o, i, d):
                x.setflags(write=False)
            self.wants[k] = (o, i, d, info)
        return self.wants[k]


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name)
            c = made[name]
            print("%s: %d points, %d of them camera hits" % (name, c.n, c.camera_hits))
            assert 600 <= c.n <= 1300 and c.camera_hits >= 200
        return made[name]
    return get


def run_device(g, f, pos, nrm, color=None, first=0, out=True, incoming=True, dirs=True, alias=False, stats=True, stream=None, pad=64):
    """The device variant on torch tensors: dict(out, incoming, dirs, stats) with the guard words checked."""
    n = pos.shape[0]
    d_pos = torch.from_numpy(np.ascontiguousarray(pos)).to(DEV)
    d_nrm = torch.from_numpy(np.ascontiguousarray(nrm)).to(DEV)
    d_out = torch.full((n + pad,), GUARD32, dtype=torch.int32, device=DEV) if out else None
    d_inc = torch.full((n + pad,), GUARD32, dtype=torch.int32, device=DEV) if incoming else None
    d_dir = torch.full((n + pad, 3), GUARD64, dtype=torch.float64, device=DEV) if dirs else None
    d_col = None
    if color is not None:
        if alias:
            d_out[:n] = torch.from_numpy(color.view(np.int32)).to(DEV)
            d_col = d_out
        else:
            d_col = torch.from_numpy(color.view(np.int32).copy()).to(DEV)
    d_stats = torch.full((25,), -1, dtype=torch.int64, device=DEV) if stats else None
    torch.cuda.synchronize(DEV)
    ptr = lambda t: t.data_ptr() if t is not None else 0
    g.path_points_device(f, n, d_pos.data_ptr(), d_nrm.data_ptr(), ptr(d_col), ptr(d_out), ptr(d_inc), ptr(d_dir), first_sample=first,
                         stream=stream if stream is not None else 0, d_stats_ptr=ptr(d_stats) or None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize(DEV)
    res = dict(out=None, incoming=None, dirs=None, stats=None)
    for key, t in (("out", d_out), ("incoming", d_inc)):
        if t is not None:
            a = t.cpu().numpy().view(np.uint32)
            assert np.all(a[n:] == GUARD32), key
            res[key] = a[:n]
    if dirs:
        a = d_dir.cpu().numpy()
        assert np.all(a[n:] == GUARD64)
        res["dirs"] = a[:n]
    if color is not None and not alias:
        assert np.array_equal(d_col.cpu().numpy().view(np.uint32), color)               # the inputs are read only
    assert np.array_equal(d_pos.cpu().numpy(), pos, equal_nan=True) and np.array_equal(d_nrm.cpu().numpy(), nrm, equal_nan=True)
    if stats:
        s = d_stats.cpu().numpy()
        assert s[24] == -1
        res["stats"] = s[:24].view(np.uint64)
    return res


def same(got, want):
    """Bit for bit (a NaN equals the same NaN)."""
    if got.shape != want.shape:
        return False
    if got.dtype == np.float64:
        return np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64))
    return int(np.count_nonzero(got != want)) == 0


def same3(d, w):
    return same(d["out"], w[0]) and same(d["incoming"], w[1]) and same(d["dirs"], w[2])


def stats_shape(st, mode, n):
    """[0..3] 0, [4] one ray per point, [5..7] the walks'; SR_MODE_BVH repeats them in [20..23]; nothing else."""
    ok = not st[:4].any() and int(st[4]) == n and not st[8:20].any()
    if mode == "bvh":
        return ok and np.array_equal(st[20:24], st[4:8])
    return ok and not st[20:].any()


# ---- 1. every trace mode, shading on and off, host and device variant ----
@pytest.mark.parametrize("shading", [False, True], ids=["plain", "shaded"])
@pytest.mark.parametrize("mode", ["tree", "brute", "bvh"])
@pytest.mark.parametrize("name", ["cube", "obj"])
def test_modes(cases, name, mode, shading):
    c = cases(name)
    w_out, w_inc, w_dirs, info = c.want(mode, shading)
    # the set exercises something: second rays that hit and that miss, and a point whose colour is normalised
    assert info["hit"].mean() >= 0.2 and (~info["hit"]).mean() >= 0.2 and info["normalised"].sum() >= 1
    assert len(np.unique(w_inc)) > 1 and not same(w_out, c.color)
    g, f = c.gpu(), path_frame(mode, shading)
    out, incoming, dirs = g.path_points(f, c.pos, c.nrm, c.color)
    assert same(out, w_out) and same(incoming, w_inc) and same(dirs, w_dirs)
    host_stats = g.ray_stats().copy()
    d = run_device(g, f, c.pos, c.nrm, c.color)
    assert same3(d, (w_out, w_inc, w_dirs))
    for st in (host_stats, d["stats"]):
        assert stats_shape(st, mode, c.n), st
    if mode == "tree":
        assert np.array_equal(host_stats, d["stats"]) and host_stats[5] > 0 and host_stats[6] > 0 and host_stats[7] > 0
    d = run_device(g, path_frame(mode, shading, extra_flags=L.F_PRIMARY_STATS_ONLY), c.pos, c.nrm, c.color)
    assert same3(d, (w_out, w_inc, w_dirs)) and not d["stats"].any()


# ---- 2. optional outputs and aliasing ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_outputs_are_optional_and_out_may_alias_color(cases, mode):
    c = cases("obj")
    g, f = c.gpu(), path_frame(mode, True)
    w_out, w_inc, w_dirs, _ = c.want(mode, True)
    d = run_device(g, f, c.pos, c.nrm, c.color, alias=True)
    assert same3(d, (w_out, w_inc, w_dirs))
    d = run_device(g, f, c.pos, c.nrm, c.color, incoming=False, dirs=False)
    assert same(d["out"], w_out) and d["incoming"] is None and d["dirs"] is None and int(d["stats"][4]) == c.n
    d = run_device(g, f, c.pos, c.nrm, c.color, out=False, dirs=False)
    assert same(d["incoming"], w_inc) and int(d["stats"][4]) == c.n
    d = run_device(g, f, c.pos, c.nrm, c.color, out=False, incoming=False)
    assert same(d["dirs"], w_dirs) and not d["stats"].any()                            # nothing was traced
    white = c.model(mode, True, c.pos, c.nrm, None)[0]
    d = run_device(g, f, c.pos, c.nrm, None)                                           # no colours: every point is white
    assert same(d["out"], white) and not same(white, w_out)
    out, incoming, dirs = g.path_points(f, c.pos, c.nrm, c.color, want_incoming=False, want_dirs=False)
    assert incoming is None and dirs is None and same(out, w_out)
    out, incoming, dirs = g.path_points(f, c.pos, c.nrm, None, want_out=False, want_incoming=False)
    assert out is None and same(dirs, w_dirs) and not g.ray_stats().any()
    out, incoming, dirs = g.path_points(f, c.pos, c.nrm, None, want_out=False, want_dirs=False)
    assert same(incoming, w_inc)


# ---- 3. passes ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
@pytest.mark.parametrize("band", [64, 100, 257])
def test_passes(cases, band, mode):
    c = cases("cube")
    g, f = c.gpu(), path_frame(mode, True)
    w = c.want(mode, True)
    g.debug_set(L.DBG_BAND_SAMPLES, band)
    try:
        d = run_device(g, f, c.pos, c.nrm, c.color)
        out, incoming, dirs = g.path_points(f, c.pos, c.nrm, c.color)
    finally:
        g.debug_set(L.DBG_BAND_SAMPLES, -1)
    assert same3(d, w) and same(out, w[0]) and same(incoming, w[1]) and same(dirs, w[2]) and int(d["stats"][4]) == c.n


# ---- 4. the random sequence, through dirs alone ----
def model_dirs(seed, first, nrm):
    return ppm.directions(ppm.draws(seed, first, nrm.shape[0]), nrm)


@pytest.mark.parametrize("first", [0, 1, 63, 64, 12345, CHUNK_POINTS - 1, CHUNK_POINTS, CHUNK_POINTS + 1])
def test_first_sample(cases, first):
    c = cases("obj")
    g = c.gpu()
    d = run_device(g, path_frame("tree"), c.pos, c.nrm, first=first, out=False, incoming=False)
    want = model_dirs(SEED, first, c.nrm)
    assert same(d["dirs"], want)
    assert first == 0 or not same(want, c.want("tree", False)[2])                      # the sequence really moved
    other = run_device(g, path_frame("tree", seed=4711), c.pos, c.nrm, first=first, out=False, incoming=False)
    assert same(other["dirs"], model_dirs(4711, first, c.nrm)) and not same(other["dirs"], want)


def test_a_batch_across_chunks_state_groups_and_passes(cases):
    """n = 2 (409 600 + 6 400 + 100) + 777 points in passes of 416 100: every pass crosses 65 chunks of the table, so its later chunks start
    from states the second workgroup of the state kernel makes, and the passes start inside a chunk of the sequence."""
    band = STATE_GROUP_POINTS + CHUNK_POINTS + 100
    n = 2 * band + 777
    assert band < MAX_PASS
    g = cases("obj").gpu()
    nrm = np.random.default_rng(3).normal(size=(n, 3))
    pos = np.zeros((n, 3))
    want = model_dirs(SEED, 5, nrm)
    g.debug_set(L.DBG_BAND_SAMPLES, band)
    try:
        d = run_device(g, path_frame("bvh"), pos, nrm, first=5, out=False, incoming=False, stats=False)
    finally:
        g.debug_set(L.DBG_BAND_SAMPLES, -1)
    assert same(d["dirs"], want)
    one = run_device(g, path_frame("bvh"), pos, nrm, first=5, out=False, incoming=False, stats=False)      # one pass
    assert same(one["dirs"], want)


def test_first_sample_beyond_what_can_be_drawn(cases):
    first, n = 2 ** 33 + 7, 18
    g = cases("obj").gpu()
    ints = sa.net_random_jump(SEED, 3 * first)[:54]
    nrm = np.random.default_rng(4).normal(size=(n, 3))
    d = run_device(g, path_frame("tree"), np.zeros((n, 3)), nrm, first=first, out=False, incoming=False)
    assert same(d["dirs"], ppm.directions(ints, nrm))


# ---- 5. chained calls, and the host's table ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_one_call_equals_three_chained_calls(cases, mode):
    c = cases("cube")
    g, f = c.gpu(), path_frame(mode, True)
    w = c.want(mode, True, 7)
    cuts = [0, 301, 302 + c.n // 3, c.n]
    first, parts = 7, []
    g.debug_set(L.DBG_BAND_SAMPLES, 200)
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts.append(g.path_points(f, c.pos[a:b], c.nrm[a:b], c.color[a:b], first_sample=first))
            first += b - a
    finally:
        g.debug_set(L.DBG_BAND_SAMPLES, -1)
    for k in range(3):
        assert same(np.concatenate([p[k] for p in parts]), w[k]), k


@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_host_table_hook_gives_identical_outputs(cases, mode):
    c = cases("cube")
    g, f = c.gpu(), path_frame(mode, True)
    w = c.want(mode, True, 63)
    g.debug_set(L.DBG_KERNEL_SWITCH, 45)
    g.debug_set(L.DBG_BAND_SAMPLES, 257)
    try:
        d = run_device(g, f, c.pos, c.nrm, c.color, first=63)
    finally:
        g.debug_set(L.DBG_KERNEL_SWITCH, -1)
        g.debug_set(L.DBG_BAND_SAMPLES, -1)
    assert same3(d, w)
    dev = run_device(g, f, c.pos, c.nrm, c.color, first=63)
    assert same3(dev, w) and np.array_equal(dev["stats"], d["stats"])


def test_host_table_refuses_a_distant_first_sample(cases):
    """The host draws its way to first_sample, so that path ends at first_sample + n = 2^30; the device's table has no such limit."""
    c = cases("obj")
    g, f = c.gpu(), path_frame("tree")
    pos, nrm = c.pos[:8], c.nrm[:8]
    far = run_device(g, f, pos, nrm, first=2 ** 30, out=False, incoming=False)
    assert same(far["dirs"], ppm.directions(sa.net_random_jump(SEED, 3 * 2 ** 30)[:24], nrm))
    g.debug_set(L.DBG_KERNEL_SWITCH, 45)
    try:
        with pytest.raises(sa.SoftrayError) as e:
            g.path_points(f, pos, nrm, first_sample=2 ** 30 - 7)
        assert e.value.code == L.SR_ERR_UNSUPPORTED and "2^30" in str(e.value)
        near = g.path_points(f, pos, nrm, first_sample=1000, want_out=False, want_incoming=False)[2]
    finally:
        g.debug_set(L.DBG_KERNEL_SWITCH, -1)
    assert same(near, model_dirs(SEED, 1000, nrm))


# ---- 6. points that are not finite ----
@pytest.mark.parametrize("name", ["cube", "obj"], ids=["with_a_plane", "without_extra_geometry"])
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_points_that_are_not_finite(cases, name, mode):
    c = cases(name)
    g = c.gpu()
    bpos, bnrm, has_nan = spm.bad_points()                                             # NaN and +-inf in pos, in normal, in both
    idx = np.arange(c.n)[:: max(1, c.n // 300)]
    rng = np.random.default_rng(11)
    pos, nrm, col = c.pos[idx].copy(), c.nrm[idx].copy(), c.color[idx]
    where = np.sort(rng.choice(idx.size, bpos.shape[0], replace=False))                # the bad points take these places of the batch
    pos[where], nrm[where] = bpos, bnrm
    for shading in (False, True):
        info = {}
        w = c.model(mode, shading, pos, nrm, col, first=3, info=info)
        d = run_device(g, path_frame(mode, shading), pos, nrm, col, first=3)
        assert same3(d, w), (shading, np.flatnonzero(d["out"] != w[0])[:8], where)
        assert stats_shape(d["stats"], mode, idx.size)
        assert not info["hit"][where][has_nan].any() and np.isfinite(w[2]).all()
    # a NaN normal on a miss: NaN channels, bytes 0
    k = int(np.flatnonzero(np.isnan(bnrm).any(axis=1) & ~np.isnan(bpos).any(axis=1))[0])
    assert w[0][where[k]] == 0xFF000000 and w[1][where[k]] == 0
    all_bad = run_device(g, path_frame(mode, True), bpos, bnrm, col[where], first=3)   # a batch in which no ray walks
    wb = c.model(mode, True, bpos, bnrm, col[where], first=3)
    assert same3(all_bad, wb)


# ---- 7. the chain on the device is the rendered frame ----
def gpu_scene(tris, prims=()):
    g = sa.GpuScene(0)
    g.set_triangles(*tris)
    if prims:
        g.set_extra(list(prims))
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH))
    return g


def device_chain(g, plain, shading, then=None):
    """render_hits -> ShadingMethod -> PathTracingMethod (-> then) over the compacted hit points on the null stream, resolved in torch:
    (pixels uint32 [rows * width], the call's d_stats, the number of hit points)."""
    n = sa.GpuScene.sample_count(plain)
    d_hit = torch.empty(n, dtype=torch.uint8, device=DEV)
    d_pos = torch.empty((n, 3), dtype=torch.float64, device=DEV)
    d_nrm = torch.empty((n, 3), dtype=torch.float64, device=DEV)
    d_col = torch.empty(n, dtype=torch.int32, device=DEV)
    g.render_hits_device(plain, d_hit=d_hit.data_ptr(), d_pos=d_pos.data_ptr(), d_normal=d_nrm.data_ptr(), d_color=d_col.data_ptr())
    idx = torch.nonzero(d_hit, as_tuple=False).reshape(-1)
    k = int(idx.numel())
    hp, hn, hc = d_pos[idx].contiguous(), d_nrm[idx].contiguous(), d_col[idx].contiguous()
    d_stats = torch.zeros(24, dtype=torch.int64, device=DEV)
    if shading:
        g.shade_points_device(plain, k, hp.data_ptr(), hn.data_ptr(), hc.data_ptr(), hc.data_ptr())
    g.path_points_device(plain, k, hp.data_ptr(), hn.data_ptr(), hc.data_ptr(), hc.data_ptr(), first_sample=0, d_stats_ptr=d_stats.data_ptr())
    if then is not None:
        then(k, hp, hn, hc)
    bg = (plain.background_argb | 0xFF000000) & 0xFFFFFFFF
    samples = torch.full((n,), bg - (1 << 32), dtype=torch.int32, device=DEV)
    samples[idx] = hc
    n2 = plain.sub_pixel_res ** 2
    if n2 > 1:
        s = samples.to(torch.int64).reshape(-1, n2)
        ch = [torch.div(((s >> sh) & 255).sum(1), n2, rounding_mode="floor") for sh in (16, 8, 0)]
        samples = (0xFF000000 | (ch[0] << 16) | (ch[1] << 8) | ch[2]).to(torch.int64)
    torch.cuda.synchronize(DEV)
    return (samples.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).astype(np.uint32), d_stats.cpu().numpy().view(np.uint64), k, (hp, hn, hc)


@pytest.mark.parametrize("sub", [1, 2])
@pytest.mark.parametrize("mode", ["tree", "bvh"])
@pytest.mark.parametrize("name", ["cube", "obj"])
def test_chain_on_the_device_is_the_rendered_frame(cases, name, mode, sub):
    c = cases(name)
    g = c.gpu()
    base = edge_light_frame(tsp.EDGE, 60, 44) if name == "cube" else make_frame(60, 44)
    base.flags &= ~orc.F_SHADOWS
    base.sub_pixel_res = sub
    base.concurrency = 1
    plain = sa.Frame.from_buffer_copy(bytes(base))
    plain.trace_mode = MODES[mode]
    full = sa.Frame.from_buffer_copy(bytes(plain))
    full.flags |= L.F_PATH_TRACING
    d_px = torch.zeros(full.width * full.height, dtype=torch.int32, device=DEV)
    d_fs = torch.zeros(24, dtype=torch.int64, device=DEV)
    g.render_device(full, d_px.data_ptr(), d_stats_ptr=d_fs.data_ptr())
    torch.cuda.synchronize(DEV)
    want = d_px.cpu().numpy().view(np.uint32)
    got, stats, k, _ = device_chain(g, plain, True)
    assert k > 500 * sub * sub and same(got, want)
    if mode == "tree":
        assert np.array_equal(stats[4:8], d_fs.cpu().numpy().view(np.uint64)[4:8]) and stats[4] == k


GOLDENS = [("pathTracing_noShading", "obj2.3DS", (), {}),
           ("pathTracing_noShading_focalBlurx2", "obj2.3DS", (), dict(focal_blur=True, sub_pixel_res=2, focal_depth=1.0)),
           ("pathTracing_noShading_6_geometry", "obj.3ds", ptm.PRIMITIVES, dict(depth=3.0))]


# (a golden with extra geometry holds the reference tree's hits: in SR_MODE_BVH it is no yardstick, as in tests/test_gpu_pathtrace.py)
GOLDEN_CASES = [g + (m,) for g in GOLDENS for m in ("tree", "bvh") if m == "tree" or not g[2]]


@pytest.mark.parametrize("name,model,prims,kw,mode", GOLDEN_CASES, ids=["%s-%s" % (x[0], x[4]) for x in GOLDEN_CASES])
def test_chain_on_the_device_is_the_golden(name, model, prims, kw, mode):
    """The one-block frame (concurrency = 1) pixel for pixel; the committed .bmp was rendered with the reference's four row blocks, whose
    first is the one-block frame's first 25 rows, and whose every block is the chain over that block's rows from sample 0."""
    g = gpu_scene(load_obj3ds(model), prims)
    gold = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))
    plain = sa.Frame.from_buffer_copy(bytes(make_frame(100, shading=False, concurrency=1, **kw)))
    plain.trace_mode = MODES[mode]
    full = sa.Frame.from_buffer_copy(bytes(plain))
    full.flags |= L.F_PATH_TRACING
    d_px = torch.zeros(100 * 100, dtype=torch.int32, device=DEV)
    g.render_device(full, d_px.data_ptr())
    torch.cuda.synchronize(DEV)
    got, _, _, _ = device_chain(g, plain, False)
    assert same(got, d_px.cpu().numpy().view(np.uint32))
    assert np.array_equal((got & 0xFFFFFF).reshape(100, 100)[:25], gold[:25])
    blocks = []
    for b in range(4):
        part = sa.Frame.from_buffer_copy(bytes(plain))
        part.start_row, part.end_row = 25 * b, 25 * b + 24
        blocks.append(device_chain(g, part, False)[0].reshape(25, 100))
    assert np.array_equal(np.concatenate(blocks) & 0xFFFFFF, gold)


# ---- 8. the combination a frame refuses: path tracing with shadows ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_path_tracing_then_shadows_on_the_device(cases, mode):
    c = cases("cube")
    g = c.gpu()
    base = edge_light_frame(tsp.EDGE, 48, 36)
    base.concurrency = 1
    shadowed = sa.Frame.from_buffer_copy(bytes(base))
    shadowed.trace_mode = MODES[mode]
    refused = sa.Frame.from_buffer_copy(bytes(shadowed))
    refused.flags |= L.F_PATH_TRACING
    with pytest.raises(sa.SoftrayError) as e:
        g.render(refused)
    assert e.value.code == L.SR_ERR_UNSUPPORTED
    plain = sa.Frame.from_buffer_copy(bytes(shadowed))
    plain.flags &= ~L.F_SHADOWS
    then = lambda k, hp, hn, hc: g.shadow_points_device(shadowed, k, hp.data_ptr(), hn.data_ptr(), hc.data_ptr(), hc.data_ptr())
    got, _, k, (hp, hn, _) = device_chain(g, plain, True, then)
    # the CPU composition on the same points
    pos, nrm = hp.cpu().numpy(), hn.cpu().numpy()
    hits = g.render_hits(plain)
    hit = hits["hit"].astype(bool)
    assert k == int(hit.sum()) > 300 and np.array_equal(hits["pos"][hit], pos)
    own = orc.shade_points(base, pos, nrm, hits["color"][hit])
    scene, target = c.geometry(mode)
    bounced = ppm.path_points(scene, target, plain, pos, nrm, own, inf_scene=c.o)[0]
    final = spm.shadowed(c.o, base, pos, nrm, bounced, tsp.TARGET)
    want = np.full(hit.size, (plain.background_argb | 0xFF000000) & 0xFFFFFFFF, dtype=np.uint32)
    want[hit] = final
    assert same(got, want) and not same(final, bounced) and not same(bounced, own)


# ---- 9. a two-part scene ----
def test_two_part_scene_on_one_ordinal(cases):
    c = cases("cube")
    gm = c.gpu(devices=[0, 0])
    w = c.want("bvh", True)
    out, incoming, dirs = gm.path_points(path_frame("bvh", True), c.pos, c.nrm, c.color)
    assert same(out, w[0]) and same(incoming, w[1]) and same(dirs, w[2])
    assert stats_shape(gm.ray_stats(), "bvh", c.n)
    d = run_device(gm, path_frame("tree", True), c.pos, c.nrm, c.color)
    assert same3(d, c.want("tree", True))


# ---- 10. stream ordering ----
def test_call_is_ordered_with_frames_on_other_streams(cases):
    """A frame on one stream, the call on another at once, a frame behind it: the scene's scratch belongs to one of them at a time."""
    c = cases("obj")
    g = c.gpu()
    fr = sa.Frame.from_buffer_copy(bytes(make_frame(256, 192, concurrency=1)))
    fr.trace_mode = sa.MODE_BVH
    fr.flags |= L.F_PATH_TRACING
    want_frame = g.render(fr)[0].copy()
    f = path_frame("bvh", True)
    w = c.want("bvh", True)
    n = c.n
    d_pos, d_nrm = torch.from_numpy(c.pos).to(DEV), torch.from_numpy(c.nrm).to(DEV)
    d_col = torch.from_numpy(c.color.view(np.int32).copy()).to(DEV)
    d_out, d_inc = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    d_dir = torch.zeros((n, 3), dtype=torch.float64, device=DEV)
    px1, px2 = torch.zeros(256 * 192, dtype=torch.int32, device=DEV), torch.zeros(256 * 192, dtype=torch.int32, device=DEV)
    s1, s2, s3 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)
    g.render_device(fr, px1.data_ptr(), s1.cuda_stream)
    g.path_points_device(f, n, d_pos.data_ptr(), d_nrm.data_ptr(), d_col.data_ptr(), d_out.data_ptr(), d_inc.data_ptr(), d_dir.data_ptr(), stream=s2)
    g.render_device(fr, px2.data_ptr(), s3.cuda_stream)
    torch.cuda.synchronize(DEV)
    assert same(d_out.cpu().numpy().view(np.uint32), w[0]) and same(d_inc.cpu().numpy().view(np.uint32), w[1]) and same(d_dir.cpu().numpy(), w[2])
    assert same(px1.cpu().numpy().view(np.uint32).reshape(want_frame.shape), want_frame)
    assert same(px2.cpu().numpy().view(np.uint32).reshape(want_frame.shape), want_frame)
