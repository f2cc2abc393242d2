"""sr_ao_points on the GPU against the CPU model (tests/ao_points_model.py, which tests/test_ao_points_model.py pins to the frame model
of the AO frames): every comparison is an exact equality over every point and every cache byte.  The point sets are those of
tests/test_gpu_shadow_points.py -- camera hit points in scan order, points on the extra geometry outside the cube (clamped origin), free
points inside and outside, zero / non-unit / reversed normals and 40 copies of one point (equal cells inside one wave)."""
import numpy as np
import pytest
import torch

import ao_model as aom
import ao_points_model as apm
import softray_amd as sa
import test_gpu_shadow_points as tsp
from helpers import edge_light_frame, load_obj3ds, make_frame, orc, unit_cube_scene

pytestmark = pytest.mark.gpu
L = sa._lib
DEV = torch.device("cuda", 0)
MODES = {"tree": sa.MODE_REF_TREE, "brute": sa.MODE_BRUTE, "bvh": sa.MODE_BVH}
GUARD32, GUARD8 = 0x01020304, 0xA5
SEED = 1234567890
CELLS = aom.RES ** 3


def ao_frame(mode="tree", uncached=False, extra_flags=0, seed=SEED):
    f = sa.Frame.from_buffer_copy(bytes(make_frame(16, shading=False)))
    f.trace_mode = MODES[mode]
    f.random_seed = seed
    f.flags |= (L.F_AO_UNCACHED if uncached else 0) | extra_flags
    return f


class Case:
    """One scene on the device and in the oracle, its point set and the model's answers, each computed once."""

    def __init__(self, name):
        self.name = name
        self.o, self.brute = orc.Scene(), orc.Scene()                    # (no tree: the root geometry of a SR_MODE_BRUTE frame)
        if name == "obj":
            self.tris, self.prims = load_obj3ds(), ()
            cam = make_frame(48, 40, shadows=True)
            light = tsp.spm.lsm.light_model(cam)[0]
        else:
            self.tris, self.prims = unit_cube_scene(2000), tsp.EDGE["prims"]
            cam = edge_light_frame(tsp.EDGE, 48, 40)
            light = tsp.EDGE["light"]
        for s in (self.o, self.brute):
            s.set_triangles(*self.tris)
            if self.prims:
                s.set_extra(list(self.prims))
        assert self.o.build_tree() == 0
        # the extra primitives alone: a model no probe can meet (a 1e-7 triangle in a corner of the box)
        self.extras_only = orc.Scene()
        c = 0.4999
        self.extras_only.set_triangles(np.array([[(c, c, c), (c + 1e-7, c, c), (c, c + 1e-7, c)]]), np.array([0xFFFFFFFF], dtype=np.uint32), *tsp.BOX)
        if self.prims:
            self.extras_only.set_extra(list(self.prims))
        pos, nrm, color, hits = tsp.point_set(self.o, cam, np.asarray(light, dtype=np.float64), tsp.spm.lsm.light_model(cam)[1], 4711 + len(name))
        keep = np.concatenate([np.arange(min(hits, 330)), np.arange(hits, pos.shape[0])])      # about 900 points: the camera's first hits, all the others
        self.pos, self.nrm, self.color = np.ascontiguousarray(pos[keep]), np.ascontiguousarray(nrm[keep]), np.ascontiguousarray(color[keep])
        self.camera_hits = min(hits, 330)
        self.n = self.pos.shape[0]
        self.scenes, self.wants = {}, {}

    def gpu(self, devices=None):
        key = None if devices is None else tuple(devices)
        if key not in self.scenes:
            g = sa.GpuScene(devices=devices) if devices else sa.GpuScene(0)
            g.set_triangles(*self.tris)
            if self.prims:
                g.set_extra(list(self.prims))
            g.build((sa.MODE_REF_TREE, sa.MODE_BVH))
            self.scenes[key] = g
        g = self.scenes[key]
        g.reset_ao_cache()
        return g

    def geometry(self, mode):
        """(scene, target) whose trace answers a probe as the frame's root geometry in `mode` does."""
        if mode == "brute":
            return self.brute, apm.TRACE_ROOT_TREE
        if mode == "tree":
            return self.o, apm.TRACE_ROOT_TREE
        if self.prims:
            return apm.NearestWithExtras(self.o, self.extras_only), apm.TRACE_NEAREST
        return self.o, apm.TRACE_NEAREST

    def model(self, mode, cache, sel=slice(None), uncached=False, first=0, color=True, seed=SEED):
        scene, target = self.geometry(mode)
        return apm.ao_points(scene, target, self.pos[sel], self.nrm[sel], seed, cache, uncached=uncached, first_generator=first,
                             color=self.color[sel] if color else None, inf_scene=self.o)

    def want(self, mode, uncached, first=0):
        """The model's (amount, out, generators, cache) for the whole set on an empty cache, read-only."""
        k = ("bvh" if mode == "bvh" else mode, uncached, first)
        if k not in self.wants:
            cache = np.zeros(CELLS, dtype=np.uint8)
            a, o, g = self.model(mode, cache, uncached=uncached, first=first)
            for x in (a, o, cache):
                x.setflags(write=False)
            self.wants[k] = (a, o, g, cache)
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


def run_device(g, f, pos, nrm, color=None, first=0, out=True, amount=True, alias=False, stats=True, stream=None, pad=64):
    """The device variant on torch tensors: dict(out, amount, generators, stats) with the guard words checked."""
    n = pos.shape[0]
    d_pos = torch.from_numpy(np.ascontiguousarray(pos)).to(DEV)
    d_nrm = torch.from_numpy(np.ascontiguousarray(nrm)).to(DEV)
    d_out = torch.full((n + pad,), GUARD32, dtype=torch.int32, device=DEV) if out else None
    d_amt = torch.full((n + pad,), GUARD8, dtype=torch.uint8, device=DEV) if amount else None
    d_col = None
    if color is not None:
        if alias:
            d_out[:n] = torch.from_numpy(color.view(np.int32)).to(DEV)
            d_col = d_out
        else:
            d_col = torch.from_numpy(color.view(np.int32).copy()).to(DEV)
    d_gen = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    d_stats = torch.full((25,), -1, dtype=torch.int64, device=DEV) if stats else None
    torch.cuda.synchronize(DEV)
    ptr = lambda t: t.data_ptr() if t is not None else 0
    g.ao_points_device(f, n, d_pos.data_ptr(), d_nrm.data_ptr(), ptr(d_col), ptr(d_out), ptr(d_amt), first_generator=first,
                       stream=stream if stream is not None else 0, d_generators_ptr=d_gen.data_ptr(), d_stats_ptr=ptr(d_stats) or None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize(DEV)
    res = dict(out=None, amount=None, stats=None)
    if out:
        o = d_out.cpu().numpy().view(np.uint32)
        assert np.all(o[n:] == GUARD32)
        res["out"] = o[:n]
    if amount:
        a = d_amt.cpu().numpy()
        assert np.all(a[n:] == GUARD8)
        res["amount"] = a[:n]
    gen = d_gen.cpu().numpy()
    assert gen[1] == -7
    res["generators"] = int(gen[0])
    if stats:
        s = d_stats.cpu().numpy()
        assert s[24] == -1
        res["stats"] = s[:24].view(np.uint64)
    return res


def same(got, want):
    return got.shape == want.shape and int(np.count_nonzero(got != want)) == 0


def cache_of(g):
    return g.get_ao_cache().reshape(-1)


# ---- 1. every trace mode, cached cold and uncached, host and device variant ----
@pytest.mark.parametrize("uncached", [False, True], ids=["cached", "uncached"])
@pytest.mark.parametrize("mode", ["tree", "brute", "bvh"])
@pytest.mark.parametrize("name", ["cube", "obj"])
def test_modes(cases, name, mode, uncached):
    c = cases(name)
    w_amount, w_out, w_gen, w_cache = c.want(mode, uncached)
    assert (w_gen == c.n) if uncached else (200 <= w_gen < c.n)                         # >= 3 chunk boundaries; equal cells are in the set
    assert len(np.unique(w_amount)) > 5
    g, f = c.gpu(), ao_frame(mode, uncached)
    out, amount, gens = g.ao_points(f, c.pos, c.nrm, c.color)
    assert gens == w_gen and same(amount, w_amount) and same(out, w_out) and same(cache_of(g), w_cache)
    host_stats = g.ray_stats().copy()
    g.reset_ao_cache()
    d = run_device(g, f, c.pos, c.nrm, c.color)
    assert d["generators"] == w_gen and same(d["amount"], w_amount) and same(d["out"], w_out) and same(cache_of(g), w_cache)
    for st in (host_stats, d["stats"]):
        assert not st[:4].any() and int(st[4]) == 100 * w_gen and not st[8:].any()
    if mode == "tree":
        assert np.array_equal(host_stats, d["stats"]) and host_stats[5] > 0 and host_stats[6] > 0 and host_stats[7] > 0
    g.reset_ao_cache()
    fp = ao_frame(mode, uncached, extra_flags=L.F_PRIMARY_STATS_ONLY)
    d = run_device(g, fp, c.pos, c.nrm, c.color)
    assert same(d["amount"], w_amount) and not d["stats"].any()


def test_tree_statistics_are_the_ao_frames(cases):
    """The probes of an uncached call over a frame's hit points are the probes of the uncached AO frame with one row block: [4..7] agree."""
    c = cases("obj")
    g = c.gpu()
    fr = sa.Frame.from_buffer_copy(bytes(aom.ao_frame(make_frame(40, 32, shading=False, concurrency=1), uncached=True)))
    hits = g.render_hits(fr)
    hit = hits["hit"].astype(bool)
    g.render(fr, stats=True)
    want = g.ray_stats().copy()
    _, _, gens = g.ao_points(ao_frame("tree", True), hits["pos"][hit], hits["normal"][hit])
    got = g.ray_stats()
    assert gens == int(hit.sum()) > 300 and np.array_equal(got[4:8], want[4:8]) and got[5] > 0 and not got[:4].any()


# ---- 2. cache states ----
def test_warm_call_and_half_preset_cache(cases):
    c = cases("cube")
    g, f = c.gpu(), ao_frame("tree")
    w_amount, w_out, w_gen, w_cache = c.want("tree", False)
    a1 = run_device(g, f, c.pos, c.nrm, c.color)
    a2 = run_device(g, f, c.pos, c.nrm, c.color)                                      # warm: nothing to generate, the same bytes
    assert a1["generators"] == w_gen and a2["generators"] == 0 and int(a2["stats"][4]) == 0
    assert same(a2["amount"], w_amount) and same(a2["out"], w_out) and same(cache_of(g), w_cache)
    # every second filled cell, and some cells the set never asks for, pre-set to 77
    preset = np.zeros(CELLS, dtype=np.uint8)
    filled = np.flatnonzero(w_cache)
    preset[filled[::2]] = 77
    preset[:4096:3] = 77
    g.set_ao_cache(preset.reshape(128, 128, 128))
    model_cache = preset.copy()
    m_amount, m_out, m_gen = c.model("tree", model_cache)
    d = run_device(g, f, c.pos, c.nrm, c.color)
    assert 0 < m_gen < w_gen and d["generators"] == m_gen
    assert same(d["amount"], m_amount) and same(d["out"], m_out) and same(cache_of(g), model_cache) and (m_amount == 77).any()


@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_calls_and_frames_share_the_cells(cases, mode):
    c = cases("obj")
    g = c.gpu()
    target = aom.TRACE_NEAREST if mode == "bvh" else aom.TRACE_ROOT_TREE
    fr = aom.ao_frame(make_frame(40, 32, shading=True, concurrency=1))
    sf = sa.Frame.from_buffer_copy(bytes(fr))
    sf.trace_mode = MODES[mode]
    # a frame, then a call
    fm = aom.AoModel()
    want_px = fm.render(c.o, fr, target)
    got_px, _ = g.render(sf)
    assert same(got_px.reshape(want_px.shape), want_px)
    m_amount, m_out, m_gen = c.model(mode, fm.cache)
    out, amount, gens = g.ao_points(ao_frame(mode), c.pos, c.nrm, c.color)
    assert 0 < m_gen == gens < c.want(mode, False)[2]                                  # the frame's cells were taken
    assert same(amount, m_amount) and same(out, m_out) and same(cache_of(g), fm.cache)
    # a call, then a frame
    g.reset_ao_cache()
    fm = aom.AoModel()
    c.model(mode, fm.cache)
    g.ao_points(ao_frame(mode), c.pos, c.nrm, c.color)
    want_px = fm.render(c.o, fr, target)
    got_px, _ = g.render(sf)
    assert same(got_px.reshape(want_px.shape), want_px) and same(cache_of(g), fm.cache)


# ---- 3. pass and chunk boundaries ----
@pytest.mark.parametrize("uncached", [False, True], ids=["cached", "uncached"])
@pytest.mark.parametrize("band", [64, 100, 257])
def test_passes(cases, band, uncached):
    """Duplicate cells straddle passes (the 40 copies and the camera's neighbours), pass ends fall inside a chunk of 64 generators."""
    c = cases("cube")
    g, f = c.gpu(), ao_frame("bvh", uncached)
    w_amount, w_out, w_gen, w_cache = c.want("bvh", uncached)
    g.debug_set(L.DBG_BAND_SAMPLES, band)
    try:
        d = run_device(g, f, c.pos, c.nrm, c.color)
        g.reset_ao_cache()
        out, amount, gens = g.ao_points(f, c.pos, c.nrm, c.color)
    finally:
        g.debug_set(L.DBG_BAND_SAMPLES, -1)
    assert d["generators"] == w_gen == gens and int(d["stats"][4]) == 100 * w_gen
    assert same(d["amount"], w_amount) and same(d["out"], w_out) and same(amount, w_amount) and same(out, w_out) and same(cache_of(g), w_cache)


@pytest.mark.parametrize("first", [0, 1, 63, 64, 12345])
def test_first_generator(cases, first):
    c = cases("obj")
    g = c.gpu()
    for uncached in (False, True):
        w_amount, w_out, w_gen, w_cache = c.want("tree", uncached, first)
        g.reset_ao_cache()
        d = run_device(g, ao_frame("tree", uncached), c.pos, c.nrm, c.color, first=first)
        assert d["generators"] == w_gen and same(d["amount"], w_amount) and same(d["out"], w_out) and same(cache_of(g), w_cache)
    assert first == 0 or not same(c.want("tree", True, first)[0], c.want("tree", True, 0)[0])          # the sequence really moved


@pytest.mark.parametrize("uncached", [False, True], ids=["cached", "uncached"])
def test_one_call_equals_three_chained_calls(cases, uncached):
    c = cases("cube")
    g, f = c.gpu(), ao_frame("tree", uncached)
    w_amount, w_out, w_gen, w_cache = c.want("tree", uncached, 7)
    cuts = [0, 301, 302 + c.n // 3, c.n]
    first, amounts, outs = 7, [], []
    g.debug_set(L.DBG_BAND_SAMPLES, 200)
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            out, amount, gens = g.ao_points(f, c.pos[a:b], c.nrm[a:b], c.color[a:b], first_generator=first)
            first += gens
            amounts.append(amount); outs.append(out)
    finally:
        g.debug_set(L.DBG_BAND_SAMPLES, -1)
    assert first == 7 + w_gen and same(np.concatenate(amounts), w_amount) and same(np.concatenate(outs), w_out) and same(cache_of(g), w_cache)


@pytest.mark.parametrize("uncached", [False, True], ids=["cached", "uncached"])
def test_host_table_hook_gives_identical_outputs(cases, uncached):
    c = cases("cube")
    g, f = c.gpu(), ao_frame("bvh", uncached)
    w_amount, w_out, w_gen, w_cache = c.want("bvh", uncached, 63)
    g.debug_set(L.DBG_KERNEL_SWITCH, 44)
    g.debug_set(L.DBG_BAND_SAMPLES, 257)
    try:
        d = run_device(g, f, c.pos, c.nrm, c.color, first=63)
    finally:
        g.debug_set(L.DBG_KERNEL_SWITCH, -1)
        g.debug_set(L.DBG_BAND_SAMPLES, -1)
    assert d["generators"] == w_gen and same(d["amount"], w_amount) and same(d["out"], w_out) and same(cache_of(g), w_cache)


def test_more_chunks_than_one_workgroup_of_states(cases):
    """9 300 generators in one pass: 146 chunks, so the start states of chunks 64.. come through the stride of 64 chunks.  The reference is
    the host's table (hook 44): System.Random itself, one draw after the other."""
    c = cases("obj")
    g, f = c.gpu(), ao_frame("bvh", True)
    reps = 9300 // c.n + 1
    pos, nrm = np.tile(c.pos, (reps, 1))[:9300], np.tile(c.nrm, (reps, 1))[:9300]
    dev = run_device(g, f, pos, nrm, first=5)
    g.debug_set(L.DBG_KERNEL_SWITCH, 44)
    try:
        host = run_device(g, f, pos, nrm, first=5)
    finally:
        g.debug_set(L.DBG_KERNEL_SWITCH, -1)
    assert dev["generators"] == host["generators"] == 9300 and same(dev["amount"], host["amount"]) and np.array_equal(dev["stats"], host["stats"])
    assert same(dev["amount"][:c.n], c.want("bvh", True, 5)[0])
    assert not same(dev["amount"][:c.n], dev["amount"][c.n:2 * c.n])                   # the copies drew other numbers


# ---- 4. the outputs ----
def test_outputs_are_optional_and_out_may_alias_color(cases):
    c = cases("obj")
    g, f = c.gpu(), ao_frame("bvh", True)
    w_amount, w_out, w_gen, _ = c.want("bvh", True)
    d = run_device(g, f, c.pos, c.nrm, c.color, alias=True)
    assert same(d["out"], w_out) and same(d["amount"], w_amount)
    d = run_device(g, f, c.pos, c.nrm, c.color, amount=False)
    assert same(d["out"], w_out) and d["amount"] is None
    d = run_device(g, f, c.pos, c.nrm, c.color, out=False)
    assert same(d["amount"], w_amount) and d["generators"] == w_gen
    d = run_device(g, f, c.pos, c.nrm, None)                                           # no colours: every point is white
    assert same(d["out"], aom.modulate(np.full(c.n, 0xFFFFFFFF, dtype=np.uint32), w_amount))
    out, amount, _ = g.ao_points(f, c.pos, c.nrm, c.color, want_out=False)
    assert out is None and same(amount, w_amount)
    out, amount, _ = g.ao_points(f, c.pos, c.nrm, None, want_amount=False)
    assert amount is None and same(out, aom.modulate(np.full(c.n, 0xFFFFFFFF, dtype=np.uint32), w_amount))
    side = torch.cuda.Stream(device=DEV)                                               # another stream than the null stream
    d = run_device(g, f, c.pos, c.nrm, c.color, stream=side)
    assert same(d["out"], w_out)


# ---- 5. probe origins that are not finite ----
@pytest.mark.parametrize("name", ["cube", "obj"], ids=["with_a_plane", "without_extra_geometry"])
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_normals_that_are_not_finite(cases, name, mode):
    c = cases(name)
    g = c.gpu()
    base = c.pos[:c.camera_hits:9][:24].copy()
    nrm = c.nrm[:c.camera_hits:9][:24].copy()
    kinds = [(np.nan, 0), (np.inf, 0), (-np.inf, 0), (np.inf, 1), (-np.inf, 1), (np.inf, 2), (-np.inf, 2), (np.nan, 2)]
    for i in range(16):
        v, axis = kinds[i % len(kinds)]
        nrm[i, axis] = v
    nrm[16] = (np.inf, -np.inf, np.inf)
    nrm[17] = (np.inf, np.nan, 0.0)
    nrm[18] = (1e6, -1e6, 0.0)                                                         # finite: the origin lies 1000 off the surface
    pos = np.concatenate([base, np.array([[np.nan, 0.1, 0.2], [0.3, np.nan, np.nan]])])   # NaN positions clamp to 0.5
    nrm = np.concatenate([nrm, np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])])
    scene, target = c.geometry(mode)
    for uncached in (False, True):
        cache = np.zeros(CELLS, dtype=np.uint8)
        m_amount, m_out, m_gen = apm.ao_points(scene, target, pos, nrm, SEED, cache, uncached=uncached, first_generator=3, inf_scene=c.o)
        g.reset_ao_cache()
        d = run_device(g, ao_frame(mode, uncached), pos, nrm, first=3)
        assert d["generators"] == m_gen and int(d["stats"][4]) == 100 * m_gen
        assert same(d["amount"], m_amount) and same(d["out"], m_out) and same(cache_of(g), cache)
    assert m_amount[0] == 255 and m_amount[7] == 255                                   # a NaN component: all 100 probes escape


# ---- 6. the chain on the device ----
@pytest.mark.parametrize("uncached", [False, True], ids=["cached", "uncached"])
@pytest.mark.parametrize("mode", ["tree", "bvh"])
@pytest.mark.parametrize("name", ["cube", "obj"])
def test_chain_on_the_device_is_the_rendered_frame(cases, name, mode, uncached):
    """render_hits -> ShadingMethod -> ShadowMethod -> AmbientOcclusionMethod, stage by stage on the null stream, against sr_render_device of
    the AO frame with one row block (concurrency = 1: the frame's generators are then numbered in scan order, as a batch's are)."""
    c = cases(name)
    g = c.gpu()
    base = edge_light_frame(tsp.EDGE, 60, 44) if name == "cube" else make_frame(60, 44, shadows=True)
    base.concurrency = 1
    plain = sa.Frame.from_buffer_copy(bytes(base))
    plain.trace_mode = MODES[mode]
    full = sa.Frame.from_buffer_copy(bytes(plain))
    full.flags |= L.F_AMBIENT_OCCLUSION | (L.F_AO_UNCACHED if uncached else 0)
    d_px = torch.zeros(full.width * full.height, dtype=torch.int32, device=DEV)
    g.render_device(full, d_px.data_ptr())
    torch.cuda.synchronize(DEV)
    want = d_px.cpu().numpy().view(np.uint32)
    want_cache = cache_of(g).copy()
    g.reset_ao_cache()
    n = sa.GpuScene.sample_count(plain)
    d_hit = torch.empty(n, dtype=torch.uint8, device=DEV)
    d_pos = torch.empty((n, 3), dtype=torch.float64, device=DEV)
    d_nrm = torch.empty((n, 3), dtype=torch.float64, device=DEV)
    d_col = torch.empty(n, dtype=torch.int32, device=DEV)
    g.render_hits_device(plain, d_hit=d_hit.data_ptr(), d_pos=d_pos.data_ptr(), d_normal=d_nrm.data_ptr(), d_color=d_col.data_ptr())
    idx = torch.nonzero(d_hit, as_tuple=False).reshape(-1)
    k = int(idx.numel())
    assert k > 500
    hp, hn, hc = d_pos[idx].contiguous(), d_nrm[idx].contiguous(), d_col[idx].contiguous()
    bg = (plain.background_argb | 0xFF000000) & 0xFFFFFFFF
    samples = torch.full((n,), bg - (1 << 32), dtype=torch.int32, device=DEV)
    g.shade_points_device(plain, k, hp.data_ptr(), hn.data_ptr(), hc.data_ptr(), hc.data_ptr())
    g.shadow_points_device(plain, k, hp.data_ptr(), hn.data_ptr(), hc.data_ptr(), hc.data_ptr())
    g.ao_points_device(full, k, hp.data_ptr(), hn.data_ptr(), hc.data_ptr(), hc.data_ptr(), 0)
    samples[idx] = hc
    torch.cuda.synchronize(DEV)
    got = samples.cpu().numpy().view(np.uint32)
    assert same(got, want) and same(cache_of(g), want_cache) and (want_cache.any() != uncached)


# ---- 7. a two-part scene ----
def test_two_part_scene_on_one_ordinal(cases):
    c = cases("cube")
    gm = c.gpu(devices=[0, 0])
    w_amount, w_out, w_gen, w_cache = c.want("bvh", False)
    out, amount, gens = gm.ao_points(ao_frame("bvh"), c.pos, c.nrm, c.color)
    assert gens == w_gen and same(amount, w_amount) and same(out, w_out) and same(cache_of(gm), w_cache)
    assert int(gm.ray_stats()[4]) == 100 * w_gen
    d = run_device(gm, ao_frame("bvh", True), c.pos, c.nrm, c.color)
    assert same(d["amount"], c.want("bvh", True)[0])


# ---- 8. ordered with the frames it shares the cache with ----
def test_call_is_ordered_with_frames_on_other_streams(cases):
    """An AO frame on one stream, the call on another at once, the frame again behind it, nothing waited for in between: the scene's scratch
    and its cache belong to one of the three at a time, so they leave what they leave one after the other with a device synchronise in
    between -- both images, the call's outputs and generator count and every cache byte.  (The serial sequence is bit-stable: it runs twice.)"""
    c = cases("obj")
    g = c.gpu()
    fr = sa.Frame.from_buffer_copy(bytes(aom.ao_frame(make_frame(256, 192, shading=True, concurrency=1))))
    fr.trace_mode = MODES["bvh"]
    f = ao_frame("bvh")
    n, npx = c.n, 256 * 192
    d_pos, d_nrm = torch.from_numpy(c.pos).to(DEV), torch.from_numpy(c.nrm).to(DEV)
    d_col = torch.from_numpy(c.color.view(np.int32).copy()).to(DEV)
    streams = [torch.cuda.Stream(DEV) for _ in range(3)]

    def sequence(serial):
        g.reset_ao_cache()
        px = [torch.zeros(npx, dtype=torch.int32, device=DEV) for _ in range(2)]
        d_out, d_amt = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
        d_gen = torch.full((1,), -7, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize(DEV)
        g.render_device(fr, px[0].data_ptr(), streams[0].cuda_stream)
        if serial:
            torch.cuda.synchronize(DEV)
        g.ao_points_device(f, n, d_pos.data_ptr(), d_nrm.data_ptr(), d_col.data_ptr(), d_out.data_ptr(), d_amt.data_ptr(), stream=streams[1],
                           d_generators_ptr=d_gen.data_ptr())
        if serial:
            torch.cuda.synchronize(DEV)
        g.render_device(fr, px[1].data_ptr(), streams[2].cuda_stream)
        torch.cuda.synchronize(DEV)
        return [px[0].cpu().numpy(), px[1].cpu().numpy(), d_out.cpu().numpy(), d_amt.cpu().numpy(), d_gen.cpu().numpy(), cache_of(g).copy()]
    want, again = sequence(True), sequence(True)
    assert all(same(a, b) for a, b in zip(want, again))
    gens, filled = int(want[4][0]), int(np.count_nonzero(want[5]))
    print("frame, call, frame: the call made %d generators of %d points, %d cells are filled" % (gens, n, filled))
    assert 0 < gens < n and filled > gens and len(np.unique(want[3])) > 5          # the frame took cells, the call made others
    got = sequence(False)
    for name, a, b in zip(("first image", "second image", "out", "amount", "generators", "cache"), got, want):
        assert same(a, b), name
