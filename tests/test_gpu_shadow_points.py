"""sr_shadow_points on the GPU against the CPU model (tests/shadow_points_model.py, which tests/test_shadow_points_model.py pins to the
reference's golden): every comparison is an exact equality over every point.  The point sets are small -- the oracle traces n x S rays for
them -- and built from what a batch of surface points can be: hit points of a camera frame in scan order, points on the extra geometry
outside the root box, points floating in free space inside and outside the box and behind the light, normals that are zero, not unit or
turned away from the light, and 40 copies of one point (equal sort keys)."""
import ctypes as C

import numpy as np
import pytest
import torch

import lightfield_model as lfm
import shadow_points_model as spm
import softray_amd as sa
from helpers import camera_rays, edge_light_case, edge_light_frame, load_obj3ds, make_frame, orc, unit_cube_scene

pytestmark = pytest.mark.gpu
L = sa._lib
DEV = torch.device("cuda", 0)
MODES = {"tree": sa.MODE_REF_TREE, "brute": sa.MODE_BRUTE, "bvh": sa.MODE_BVH}
TARGET = lfm.TRACE_ROOT_TREE                       # extra geometry + the model: a sample is blocked iff something is hit with rayFrac <= 1
GUARD = 0x01020304
EDGE = edge_light_case((1, 0, -1), 0.1, 0.6)       # the cube scene's light, its extra geometry (a plane, a sphere, a box) and offset table
BOX = (np.array([-0.5] * 3), np.array([0.5] * 3))


def as_sr(frame, mode="bvh", extra_flags=0):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = MODES[mode]
    f.flags |= extra_flags
    return f


def point_set(o, f, light, ldir, seed):
    """(pos, nrm, color) for one scene: see the module's docstring.  `f`: a camera frame that sees the scene (and its extra geometry)."""
    rng = np.random.default_rng(seed)
    origin, dirs = camera_rays(f)
    res = o.trace(TARGET, np.broadcast_to(origin, dirs.shape).copy(), dirs)
    hit = res["hit"].astype(bool)
    pos, nrm = [res["pos"][hit]], [res["normal"][hit]]                       # scan order; extra geometry outside the box is among them
    k = 160
    free_in = rng.uniform(-0.5, 0.5, (k, 3))
    free_out = rng.uniform(-1.5, 1.5, (k, 3))
    free_out[np.abs(free_out).max(axis=1) < 0.5] *= 4.0
    behind = light[None, :] + (light / np.linalg.norm(light))[None, :] * rng.uniform(0.05, 2.0, (k // 4, 1)) + rng.uniform(-0.2, 0.2, (k // 4, 3))
    # 1000.5 light directions up the directional light: such a point's sample rays start inside the model's box and run through it
    far = rng.uniform(-0.1, 0.1, (16, 3)) - ldir[None, :] * 1000.5
    for p in (free_in, free_out, behind, far):
        n = rng.normal(size=p.shape)
        pos.append(p); nrm.append(n / np.linalg.norm(n, axis=1)[:, None])
    base_p, base_n = res["pos"][hit][::7][:k], res["normal"][hit][::7][:k]
    pos.append(base_p[0::3]); nrm.append(np.zeros_like(base_p[0::3]))        # zero normals
    pos.append(base_p[1::3]); nrm.append(base_n[1::3] * 37.5)                # not unit: the probe end moves 0.0375 off the surface
    pos.append(base_p[2::3]); nrm.append(-base_n[2::3])                      # turned away: the probe end is inside the surface
    pos.append(np.repeat(base_p[:1], 40, axis=0)); nrm.append(np.repeat(base_n[:1], 40, axis=0))
    pos, nrm = np.ascontiguousarray(np.concatenate(pos)), np.ascontiguousarray(np.concatenate(nrm))
    color = (rng.integers(0, 1 << 24, pos.shape[0]).astype(np.uint32) | np.uint32(0xFF000000))
    order = np.arange(pos.shape[0])
    order[hit.sum():] = rng.permutation(order[hit.sum():])                   # the camera's hit points stay in scan order, the rest is mixed
    return pos[order], nrm[order], color[order], int(hit.sum())


class Case:
    """One scene on the device and in the oracle, its point set and the model's answers, each computed once per (frame, subset)."""

    def __init__(self, name):
        self.name = name
        self.o = orc.Scene()
        if name == "obj":
            self.tris = load_obj3ds()
            self.prims = ()
            self.frame = make_frame(48, 40, shadows=True)
            light = spm.lsm.light_model(self.frame)[0]
        else:
            self.tris = unit_cube_scene(2000)
            self.prims = EDGE["prims"]
            self.frame = edge_light_frame(EDGE, 48, 40)
            light = EDGE["light"]
        self.o.set_triangles(*self.tris)
        if self.prims:
            self.o.set_extra(list(self.prims))
        assert self.o.build_tree() == 0
        self.brute = orc.Scene()                     # no tree: the oracle's root geometry is the extra geometry + the brute-force model (SR_MODE_BRUTE)
        self.brute.set_triangles(*self.tris)
        if self.prims:
            self.brute.set_extra(list(self.prims))
        self.pos, self.nrm, self.color, self.camera_hits = point_set(self.o, self.frame, np.asarray(light, dtype=np.float64), spm.lsm.light_model(self.frame)[1], 20240 + len(name))
        self.n = self.pos.shape[0]
        self.scenes, self.wants = {}, {}

    def gpu(self, on_device=None, devices=None):
        key = (on_device, None if devices is None else tuple(devices))
        if key not in self.scenes:
            g = sa.GpuScene(devices=devices) if devices else sa.GpuScene(0)
            g.set_triangles(*self.tris)
            if self.prims:
                g.set_extra(list(self.prims))
            g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=on_device)
            self.scenes[key] = g
        return self.scenes[key]

    def want(self, f, idx=None, key=None, brute=False):
        """The model's colours for the points idx (default: all) under frame f, read-only.  brute: the root geometry of a SR_MODE_BRUTE frame -- it
        answers as the tree's (and the own BVH's) except where a probe end lies exactly on a triangle (the zero normals): rayFrac is 1 within an ulp."""
        k = (key if key is not None else bytes(f), None if idx is None else idx.tobytes(), brute)
        if k not in self.wants:
            sel = slice(None) if idx is None else idx
            w = spm.shadowed(self.brute if brute else self.o, f, self.pos[sel], self.nrm[sel], self.color[sel], TARGET)
            w.setflags(write=False)
            self.wants[k] = w
        return self.wants[k]


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name)
            c = made[name]
            print("%s: %d points, %d of them camera hits" % (name, c.n, c.camera_hits))
            assert 700 <= c.n <= 3000 and c.camera_hits >= 300
        return made[name]
    return get


def subset(c, n=600):
    """Every kind of point, few of them: what the frames with other lights, sample counts and hooks are checked on."""
    return np.ascontiguousarray(np.arange(c.n)[:: max(1, c.n // n)])


def run(g, f, c, idx=None, color=True, **kw):
    sel = slice(None) if idx is None else idx
    return g.shadow_points(f, c.pos[sel], c.nrm[sel], c.color[sel] if color else None, **kw)


def run_device(g, f, pos, nrm, color, coherent=False, stream=None, alias=False, stats=False, pad=64):
    """The device variant on torch tensors: (out [n], the guard words behind it, d_stats or None)."""
    n = pos.shape[0]
    d_pos = torch.from_numpy(np.ascontiguousarray(pos)).to(DEV)
    d_nrm = torch.from_numpy(np.ascontiguousarray(nrm)).to(DEV)
    d_out = torch.full((n + pad,), GUARD, dtype=torch.int32, device=DEV)
    d_col = None
    if color is not None:
        if alias:
            d_out[:n] = torch.from_numpy(color.view(np.int32)).to(DEV)
            d_col = d_out
        else:
            d_col = torch.from_numpy(color.view(np.int32).copy()).to(DEV)
    d_stats = torch.full((24,), -1, dtype=torch.int64, device=DEV) if stats else None
    torch.cuda.synchronize(DEV)
    g.shadow_points_device(f, n, d_pos.data_ptr(), d_nrm.data_ptr(), d_col.data_ptr() if d_col is not None else 0, d_out.data_ptr(), coherent=coherent,
                           stream=stream if stream is not None else 0, d_stats_ptr=d_stats.data_ptr() if stats else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize(DEV)
    out = d_out.cpu().numpy().view(np.uint32)
    return out[:n], out[n:], (d_stats.cpu().numpy().view(np.uint64) if stats else None)


def same(got, want):
    return got.shape == want.shape and int(np.count_nonzero(got != want)) == 0


# ---- 1. sizes and boundaries ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, None])
def test_sizes(cases, n):
    c = cases("obj")
    g, f = c.gpu(), as_sr(c.frame)
    n = c.n if n is None else n
    want = c.want(c.frame)[:n]
    got, guard, _ = run_device(g, f, c.pos[:n], c.nrm[:n], c.color[:n])
    assert same(got, want) and np.all(guard == GUARD)
    assert same(g.shadow_points(f, c.pos[:n], c.nrm[:n], c.color[:n]), want)
    if n == c.n:
        lit = want != spm.ao_model.modulate(c.color, np.zeros(c.n, dtype=np.int64))
        full = want == spm.ao_model.modulate(c.color, np.full(c.n, 255))
        assert lit.sum() > 100 and (~lit).sum() > 100 and (lit & ~full).sum() > 100           # light, umbra and penumbra are in the set


@pytest.mark.parametrize("coherent", [False, True])
def test_three_passes_with_a_partial_last_one(cases, coherent):
    c = cases("cube")
    g, f = c.gpu(), as_sr(c.frame)
    idx = np.arange(300)
    g.debug_set(L.DBG_BAND_SAMPLES, 128)
    try:
        got, guard, _ = run_device(g, f, c.pos[idx], c.nrm[idx], c.color[idx], coherent=coherent)
    finally:
        g.debug_set(L.DBG_BAND_SAMPLES, -1)
    assert same(got, c.want(c.frame)[:300]) and np.all(guard == GUARD)


# ---- 2. modes and paths ----
@pytest.mark.parametrize("mode", ["tree", "brute", "bvh"])
@pytest.mark.parametrize("name", ["obj", "cube"])
def test_modes(cases, name, mode):
    c = cases(name)
    assert same(run(c.gpu(), as_sr(c.frame, mode), c), c.want(c.frame, brute=mode == "brute"))


@pytest.mark.parametrize("name", ["obj", "cube"])
def test_host_built_bvh(cases, name):
    c = cases(name)
    g = c.gpu(on_device=False)
    assert g.bvh_stats()[3] == 0 and cases(name).gpu().bvh_stats()[3] == 1
    for mode in ("tree", "bvh"):
        assert same(run(g, as_sr(c.frame, mode), c), c.want(c.frame))


def directional(c, samples=17):
    f = orc.Frame.from_buffer_copy(bytes(c.frame))
    f.flags &= ~orc.F_POINT_LIGHT
    f.area_light_offsets = None
    f.shadow_samples = samples
    return f


@pytest.mark.parametrize("mode", ["tree", "bvh"])
@pytest.mark.parametrize("name", ["obj", "cube"])
def test_directional_light(cases, name, mode):
    """obj: no extra geometry, the samples of a point inside the model's box provably escape (the frame's shortcut) -- the points outside it
    take the literal rays.  cube: extra geometry, literal rays throughout.  SR_DBG_LITERAL_SHADOWS: literal rays for every point."""
    c = cases(name)
    f = directional(c)
    want = c.want(f)
    g = c.gpu()
    assert same(run(g, as_sr(f, mode), c), want)
    g.debug_set(L.DBG_LITERAL_SHADOWS, 1)
    try:
        assert same(run(g, as_sr(f, mode), c), want)
    finally:
        g.debug_set(L.DBG_LITERAL_SHADOWS, -1)
    if name == "obj":
        assert np.count_nonzero(want != spm.ao_model.modulate(c.color, np.full(c.n, 255))) > 0        # a point outside the box whose samples the model blocks


HOOKS = {"per_lane_shadows": dict(flags=L.F_PER_LANE_SHADOWS), "literal_secondary": dict(flags=L.F_LITERAL_SECONDARY, mode="tree"),
         "exact_shadow_tests": dict(dbg={L.DBG_EXACT_SHADOW_TESTS: 1}), "round_caps": dict(dbg={L.DBG_ROUND_CAP0: 2, L.DBG_ROUND_CAP1: 4}),
         "switch_37_no_sort": dict(dbg={L.DBG_KERNEL_SWITCH: 37}), "switch_38_per_lane_walks": dict(dbg={L.DBG_KERNEL_SWITCH: 38}),
         "per_lane_shaft_both": dict(dbg={L.DBG_PER_LANE_SHAFT: 3})}


@pytest.mark.parametrize("hook", sorted(HOOKS))
@pytest.mark.parametrize("name", ["obj", "cube"])
def test_paths_give_the_models_colours(cases, name, hook):
    c = cases(name)
    h = HOOKS[hook]
    g = c.gpu()
    f = as_sr(c.frame, h.get("mode", "bvh"), h.get("flags", 0))
    for key, value in h.get("dbg", {}).items():
        g.debug_set(key, value)
    try:
        got = run(g, f, c)
        second_round = g.debug_counters()[2]
    finally:
        for key in h.get("dbg", {}):
            g.debug_set(key, -1)
    assert same(got, c.want(c.frame))
    if hook == "round_caps":
        assert second_round > 0                                               # hit points went on to the second round


# ---- 3. samples and offsets ----
@pytest.mark.parametrize("samples", [1, 17, 100, 130])
@pytest.mark.parametrize("name", ["obj", "cube"])
def test_sample_counts(cases, name, samples):
    c = cases(name)
    f = orc.Frame.from_buffer_copy(bytes(make_frame(48, 40, shadows=True, shadow_samples=samples)))
    if name == "cube":                                                       # the seed's table (radius 0.2) around the cube scene's light
        t = [f.transform[i] for i in range(12)]
        m = EDGE["light"]
        for r in range(3):
            f.light_pos_view[r] = t[4 * r] * m[0] + t[4 * r + 1] * m[1] + t[4 * r + 2] * m[2] + t[4 * r + 3]
    idx = subset(c)
    want = c.want(f, idx)
    for mode in ("bvh", "tree"):
        assert same(run(c.gpu(), as_sr(f, mode), c, idx), want)


def test_caller_given_offset_table(cases):
    c = cases("obj")
    table = np.ascontiguousarray(orc.area_light_offsets(987654321, 23) * np.array([2.5, 0.5, 1.0]))
    f = orc.Frame.from_buffer_copy(bytes(make_frame(48, 40, shadows=True, shadow_samples=23)))
    f.area_light_offsets = table.ctypes.data
    idx = subset(c)
    want = c.want(f, idx, key=b"table23")
    assert same(run(c.gpu(), as_sr(f), c, idx), want)
    plain = orc.Frame.from_buffer_copy(bytes(f))
    plain.area_light_offsets = None
    assert not same(want, c.want(plain, idx))


@pytest.mark.parametrize("signs", [(0, -1, 0), (-1, -1, -1)])
def test_edge_light_with_radius_0_6(cases, signs):
    """Another light of helpers.edge_light_case, just outside the box with the wide table, on the cube scene's geometry and points."""
    c = cases("cube")
    e = edge_light_case(signs, 0.02, 0.6)
    f = edge_light_frame(e, 48, 40)
    idx = subset(c)
    want = c.want(f, idx, key=repr(signs).encode())
    for mode in ("bvh", "tree"):
        assert same(run(c.gpu(), as_sr(f, mode), c, idx), want)


# ---- 4. order ----
@pytest.mark.parametrize("coherent", [False, True])
@pytest.mark.parametrize("name", ["obj", "cube"])
def test_permuted_input_gives_permuted_output(cases, name, coherent):
    c = cases(name)
    perm = np.random.default_rng(5).permutation(c.n)
    got = run(c.gpu(), as_sr(c.frame), c, perm, coherent=coherent)
    assert same(got, c.want(c.frame)[perm])
    assert same(run(c.gpu(), as_sr(c.frame), c, coherent=coherent), c.want(c.frame))


def test_no_colours_is_white_and_out_may_alias_color(cases):
    c = cases("cube")
    g, f = c.gpu(), as_sr(c.frame)
    white = np.full(c.n, 0xFFFFFFFF, dtype=np.uint32)
    want = spm.ao_model.modulate(white, spm.light_bytes(spm.escapes(c.o, c.frame, c.pos, c.nrm, TARGET), EDGE["samples"]))
    assert same(run(g, f, c, color=False), want)
    assert same(g.shadow_points(f, c.pos, c.nrm, white), want)
    got, guard, _ = run_device(g, f, c.pos, c.nrm, None)
    assert same(got, want) and np.all(guard == GUARD)
    got, guard, _ = run_device(g, f, c.pos, c.nrm, c.color, alias=True)
    assert same(got, c.want(c.frame)) and np.all(guard == GUARD)


# ---- 5. against the frame path, device against device ----
def test_frame_pixels_are_the_calls_output_on_the_frames_hit_points():
    g = sa.GpuScene(0)
    g.set_triangles(*unit_cube_scene(2000))
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH))
    for mode in ("bvh", "tree"):
        f = as_sr(make_frame(200, 160, shadows=True, depth=1.6), mode)
        before = g.render(f)[0].copy()
        origin, dirs = camera_rays(f)
        res = g.trace(MODES[mode], np.broadcast_to(origin, dirs.shape).copy(), dirs)
        hit = res["hit"].astype(bool)
        assert 5000 < hit.sum() < hit.size
        shaded = g.shade_points(f, res["pos"][hit], res["normal"][hit], res["color"][hit])
        want = np.full(hit.size, 0xFFFF00FF, dtype=np.uint32)                 # the background where the camera ray misses
        for coherent in (True, False):
            want[hit] = g.shadow_points(f, res["pos"][hit], res["normal"][hit], shaded, coherent=coherent)
            assert same(before, want)
        assert same(g.render(f)[0], before)                                   # the call leaves the scene's per-frame state as a frame does
        plain = as_sr(make_frame(200, 160, depth=1.6), mode)
        assert not same(g.render(plain)[0], before) and same(g.render(f)[0], before)


# ---- 6. points that are not finite ----
@pytest.mark.parametrize("point_light", [True, False], ids=["point", "directional"])
@pytest.mark.parametrize("name", ["obj", "cube"])
def test_non_finite_points_in_a_batch(cases, name, point_light):
    c = cases(name)
    f = c.frame if point_light else directional(c)
    bpos, bnrm, has_nan = spm.bad_points()
    idx = subset(c, 300)
    rng = np.random.default_rng(11)
    pos, nrm, col = c.pos[idx], c.nrm[idx], c.color[idx]
    where = np.sort(rng.choice(idx.size, bpos.shape[0], replace=False))       # the bad points take these places of the batch
    mixed_pos, mixed_nrm = pos.copy(), nrm.copy()
    mixed_pos[where], mixed_nrm[where] = bpos, bnrm
    want_bad = spm.shadowed(c.o, f, bpos, bnrm, col[where], TARGET)
    assert np.array_equal(want_bad, spm.shadowed(c.brute, f, bpos, bnrm, col[where], TARGET))
    assert np.array_equal(want_bad[has_nan], spm.ao_model.modulate(col[where][has_nan], np.full(int(has_nan.sum()), 255)))
    if name == "cube" and point_light:
        assert np.count_nonzero(want_bad != spm.ao_model.modulate(col[where], np.full(where.size, 255))) > 0     # the plane blocks an infinite direction
    for mode in ("bvh", "tree", "brute"):
        want = c.want(f, idx, brute=mode == "brute").copy()
        want[where] = want_bad
        for coherent in (False, True):
            got = c.gpu().shadow_points(as_sr(f, mode), mixed_pos, mixed_nrm, col, coherent=coherent)
            assert same(got, want), (mode, coherent, np.flatnonzero(got != want)[:8])
    all_bad = c.gpu().shadow_points(as_sr(f), bpos, bnrm, col[where])        # a batch that queues nothing
    assert same(all_bad, want_bad)


# ---- 7. the device variant: a stream of the caller's, statistics ----
def test_device_variant_on_a_stream_with_statistics(cases):
    c = cases("obj")
    g, f = c.gpu(), as_sr(c.frame)
    want = c.want(c.frame)
    host = run(g, f, c)
    host_stats = g.ray_stats().copy()
    assert same(host, want)
    assert not host_stats[:4].any() and int(host_stats[4]) > 0 and int(host_stats[11]) > 0       # no primary rays; shadow rays, and hit points the shaft walk took
    st = torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)
    big = torch.ones((4096, 4096), dtype=torch.float64, device=DEV)
    with torch.cuda.stream(st):
        busy = big @ big                                                      # the call is enqueued behind work that is still running
        got, guard, stats = run_device(g, f, c.pos, c.nrm, c.color, stream=st, stats=True)
    assert same(got, want) and np.all(guard == GUARD)
    assert np.array_equal(stats, host_stats)
    assert float(busy[0, 0]) == 4096.0
    quiet = as_sr(c.frame, extra_flags=L.F_PRIMARY_STATS_ONLY)
    got, _, stats = run_device(g, quiet, c.pos, c.nrm, c.color, stream=st, stats=True)
    assert same(got, want) and not stats.any()
    assert same(run(g, quiet, c), want) and not g.ray_stats().any()


def test_call_is_ordered_with_frames_on_other_streams(cases):
    """A frame on one stream, the call on another at once, a frame behind it: the scene's scratch belongs to one of them at a time."""
    c = cases("obj")
    g = c.gpu()
    fr = as_sr(make_frame(256, 192, shadows=True))
    want_frame = g.render(fr)[0].copy()
    f = as_sr(c.frame)
    n = c.n
    d_pos, d_nrm = torch.from_numpy(c.pos).to(DEV), torch.from_numpy(c.nrm).to(DEV)
    d_col = torch.from_numpy(c.color.view(np.int32).copy()).to(DEV)
    d_out = torch.zeros(n, dtype=torch.int32, device=DEV)
    px1, px2 = torch.zeros(256 * 192, dtype=torch.int32, device=DEV), torch.zeros(256 * 192, dtype=torch.int32, device=DEV)
    s1, s2, s3 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)
    g.render_device(fr, px1.data_ptr(), s1.cuda_stream)
    g.shadow_points_device(f, n, d_pos.data_ptr(), d_nrm.data_ptr(), d_col.data_ptr(), d_out.data_ptr(), stream=s2)
    g.render_device(fr, px2.data_ptr(), s3.cuda_stream)
    torch.cuda.synchronize(DEV)
    assert same(d_out.cpu().numpy().view(np.uint32), c.want(c.frame))
    assert same(px1.cpu().numpy().view(np.uint32), want_frame) and same(px2.cpu().numpy().view(np.uint32), want_frame)


# ---- 8. a multi-device scene runs the call on its first device ----
def test_multi_device_scene(cases):
    c = cases("cube")
    g = c.gpu(devices=[0, 0])
    assert g.device_count() == 2
    f = as_sr(c.frame)
    assert same(run(g, f, c), c.want(c.frame))
    stats = g.ray_stats()                                                     # the first part's, reported by the multi-device scene
    assert int(stats[4]) > 0 and int(stats[11]) > 0 and not stats[:4].any()
    got, guard, _ = run_device(g, f, c.pos, c.nrm, c.color)
    assert same(got, c.want(c.frame)) and np.all(guard == GUARD)


# ---- 9. after a refit ----
def test_after_refit_equals_a_scene_built_on_the_moved_vertices(cases):
    c = cases("cube")
    v9, argb = unit_cube_scene(2000)[:2]
    grid = 2.0 ** 20
    v9 = np.round(np.asarray(v9) * grid) / grid
    rng = np.random.default_rng(3)
    moved = np.clip(v9 + np.round(rng.uniform(-0.02, 0.02, (v9.shape[0], 1, 3)) * grid) / grid, -0.5, 0.5)
    g = sa.GpuScene(0)
    g.set_triangles(v9, argb, *BOX)
    g.set_extra(list(c.prims))
    g.build((sa.MODE_BVH,), on_device=True)
    f = as_sr(c.frame)
    idx = subset(c)
    first = run(g, f, c, idx)                                                 # (a call before the refit: the per-light records are re-made after it)
    g.refit_triangles_device(torch.from_numpy(np.ascontiguousarray(moved)).to(DEV), None, *BOX)
    fresh = sa.GpuScene(0)
    fresh.set_triangles(moved, argb, *BOX)
    fresh.set_extra(list(c.prims))
    fresh.build((sa.MODE_BVH,), on_device=True)
    got, want = run(g, f, c, idx), run(fresh, f, c, idx)
    assert same(got, want) and not same(got, first)
    o = orc.Scene()
    o.set_triangles(moved, argb, *BOX)
    o.set_extra(list(c.prims))
    assert o.build_tree() == 0
    assert same(want, spm.shadowed(o, c.frame, c.pos[idx], c.nrm[idx], c.color[idx], TARGET))
