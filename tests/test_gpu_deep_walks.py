"""Every walk of the library on trees as deep as sr_build accepts: the host builder's chains under one triangle per leaf, the device
build's tree at the depth limit, the cluster staircases whose four-wide trees are the deepest the private walks and the packet walks
take, and the one whose four-wide tree no walk takes (tests/bvh_shape_cases.py).  A traversal stack undersized by one level gives a
plausible wrong answer here and nowhere else.  Every comparison is exact, against the oracle and the CPU models; the inputs are tests/deep_walk_cases.py's,
whose outcome classes tests/test_deep_walk_cases.py checks on the CPU."""
import numpy as np
import pytest
import torch

import all_hits_model as ahm
import ao_model as aom
import ao_points_model as apm
import bvh_shape_cases as bsc
import closest_points_cases as cpc
import closest_points_model as cpm
import deep_walk_cases as dw
import gbuffer_model as gbm
import lightfield_bake as lfb
import lightfield_model as lfm
import lightfield_rays_model as lrm
import lightfield_shadow_model as lsm
import occluded_rays_cases as occ
import path_points_model as ppm
import pathtrace_model as ptm
import shadow_points_model as spm
import softray_amd as sa
import static_shadow_points_model as sspm
from nearest_rays_model import KEYS, same_bits, same_values

pytestmark = pytest.mark.gpu
L = sa._lib
DEV = torch.device("cuda", 0)
SCENES = list(dw.SCENES)
NEAREST = dw.TRACE_NEAREST
TARGETS = (sa.MODE_BVH, sa.MODE_BVH | L.TARGET_ROOT)
TORCH_TYPES = dict(hit=torch.uint8, ray_frac=torch.float64, pos=torch.float64, normal=torch.float64, color=torch.int32, tri_index=torch.int32)
NP_TYPES = dict(hit=np.uint8, ray_frac=np.float64, pos=np.float64, normal=np.float64, color=np.uint32, tri_index=np.int32)


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(name):
        if name not in made:
            leaf, on_device = dw.SCENES[name]
            g = sa.GpuScene(0)
            g.set_triangles(*bsc.scene(name))
            if leaf is not None:
                g.debug_set(L.DBG_BVH_LEAF, leaf)
            g.build((sa.MODE_BVH,), on_device=on_device)
            depth, _, _, built_on_device = g.bvh_stats()
            wide = g.wide_tree_stats()[0]
            print("%s: depth %d, wide depth %d" % (name, depth, wide))
            assert built_on_device == (1 if on_device else 0) and depth <= 62
            assert {"chain": depth >= 50 and wide >= 21, "deep": wide >= 21, "limit": depth == 62, "private_edge": wide == 20, "wide_edge": wide == 40,
                    "wide_deep": wide >= 41}[name]
            made[name] = g
        return made[name]
    return get


def with_hook(g, hook, fn):
    g.debug_set(L.DBG_KERNEL_SWITCH, hook)
    try:
        return fn()
    finally:
        g.debug_set(L.DBG_KERNEL_SWITCH, -1)


def banded(g, fn, samples=1024):
    """fn() in passes of `samples` rays, points or camera samples (16 rows of these frames): two passes or more for every input here."""
    g.debug_set(L.DBG_BAND_SAMPLES, samples)
    try:
        return fn()
    finally:
        g.debug_set(L.DBG_BAND_SAMPLES, -1)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                        # (a copy: the inputs are read-only)


def sr_frame(f, flags=0):
    s = sa.Frame.from_buffer_copy(bytes(f))
    s.trace_mode = sa.MODE_BVH
    s.flags |= flags
    return s


def hit_tensors(n):
    return {k: torch.zeros((n, 3) if k in ("pos", "normal") else (n,), dtype=TORCH_TYPES[k], device=DEV) for k in KEYS}


def hits_back(out):
    return {k: out[k].cpu().numpy().view(NP_TYPES[k]) for k in KEYS}


# ---- ray batches ----
@pytest.mark.parametrize("scene", SCENES)
def test_origin_rays(scenes, scene):
    g = scenes(scene)
    for name, origin in dw.ORIGINS.items():
        dirs = dw.origin_dirs(scene, name)
        n = dirs.shape[0]
        starts = np.ascontiguousarray(np.tile(np.array(origin), (n, 1)))
        want = dw.oracle_origin(scene, name)
        for target in TARGETS:
            traced = g.trace(target, starts, dirs)
            assert same_values(traced, want), (name, target)
            for coherent in (False, True):
                assert same_bits(g.trace_origin(target, origin, dirs, coherent=coherent), traced), (name, target, coherent)
        assert n > 1024 and same_bits(banded(g, lambda: g.trace_origin(sa.MODE_BVH, origin, dirs)), traced), (name, "passes")
        st = torch.cuda.Stream(DEV)
        d_dirs, out = dev(dirs), hit_tensors(n)
        torch.cuda.synchronize(DEV)
        g.trace_origin_device(sa.MODE_BVH, origin, n, d_dirs.data_ptr(), *[out[k].data_ptr() for k in KEYS], stream=st)
        st.synchronize()
        assert same_bits(hits_back(out), traced), (name, "device")


@pytest.mark.parametrize("scene", SCENES)
def test_occluded_rays(scenes, scene):
    g = scenes(scene)
    s, d = dw.ray_batch(scene)
    lim = dw.batch_limits(scene)
    want = occ.model(dw.oracle_batch(scene), lim)
    for target in TARGETS:
        assert np.array_equal(occ.model(g.trace(target, s, d), lim), want), target
        for hook in (-1, 46, 47, 100, 124):
            for coherent in (False, True):
                got = with_hook(g, hook, lambda: g.occluded(target, s, d, limits=lim, coherent=coherent))
                assert np.array_equal(got, want), (target, hook, coherent)
    assert s.shape[0] > 1024 and np.array_equal(banded(g, lambda: g.occluded(sa.MODE_BVH, s, d, limits=lim)), want)
    st = torch.cuda.Stream(DEV)
    d_s, d_d, d_lim = dev(s), dev(d), dev(lim)
    d_out = torch.full((s.shape[0],), 7, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize(DEV)
    g.occluded_device(sa.MODE_BVH, s.shape[0], d_s.data_ptr(), d_d.data_ptr(), d_lim.data_ptr(), d_out.data_ptr(), stream=st)
    st.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)


@pytest.mark.parametrize("scene", SCENES)
def test_all_hits_rays(scenes, scene):
    g = scenes(scene)
    s, d = dw.ray_batch(scene)
    n, K = s.shape[0], 8
    cand = ahm.Candidates(bsc.scene(scene), (), s, d, False)
    for lim in (None, dw.batch_limits(scene)):
        want = ahm.rows(cand.lists(lim), K)
        for target in TARGETS:
            for hook in (-1, 50, 51):
                got = with_hook(g, hook, lambda: g.all_hits(target, s, d, limits=lim, max_hits=K))
                assert ahm.same_rows(got, want), (lim is None, target, hook)
        assert n > 1024 and ahm.same_rows(banded(g, lambda: g.all_hits(sa.MODE_BVH, s, d, limits=lim, max_hits=K)), want), (lim is None, "passes")
    st = torch.cuda.Stream(DEV)
    d_s, d_d, d_lim = dev(s), dev(d), dev(dw.batch_limits(scene))
    d_count = torch.zeros(n, dtype=torch.int32, device=DEV)
    d_index = torch.zeros((n, K), dtype=torch.int32, device=DEV)
    d_frac = torch.zeros((n, K), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize(DEV)
    g.all_hits_device(sa.MODE_BVH, n, d_s.data_ptr(), d_d.data_ptr(), d_lim.data_ptr(), K, d_count.data_ptr(), d_index.data_ptr(), d_frac.data_ptr(), stream=st)
    st.synchronize()
    got = dict(count=d_count.cpu().numpy().view(np.uint32), index=d_index.cpu().numpy(), ray_frac=d_frac.cpu().numpy())
    assert ahm.same_rows(got, want)


@pytest.mark.parametrize("scene", SCENES)
def test_closest_points(scenes, scene):
    g = scenes(scene)
    points = dw.closest_points(scene)
    n = points.shape[0]
    answers = cpm.Answers(points, bsc.scene(scene)[0])
    limits = cpc.limit_kinds(answers.dist)[0]
    for max_dist in (None, limits):
        want = answers.outputs(max_dist)
        for hook in (-1, 52, 53):
            for coherent in (False, True):
                got = with_hook(g, hook, lambda: g.closest_points(sa.MODE_BVH, points, max_dist=max_dist, coherent=coherent))
                for key in ("tri_index", "dist", "pos", "uv"):
                    assert cpm.same_bits(got[key], want[key]), (max_dist is None, hook, coherent, key)
        got = banded(g, lambda: g.closest_points(sa.MODE_BVH, points, max_dist=max_dist), 200)
        assert all(cpm.same_bits(got[key], want[key]) for key in want), (max_dist is None, "passes")
    st = torch.cuda.Stream(DEV)
    d_p, d_lim = dev(points), dev(limits)
    out = dict(tri_index=torch.zeros(n, dtype=torch.int32, device=DEV), dist=torch.zeros(n, dtype=torch.float64, device=DEV),
               pos=torch.zeros((n, 3), dtype=torch.float64, device=DEV), uv=torch.zeros((n, 2), dtype=torch.float64, device=DEV))
    torch.cuda.synchronize(DEV)
    g.closest_points_device(sa.MODE_BVH, n, d_p.data_ptr(), d_lim.data_ptr(), out["tri_index"].data_ptr(), out["dist"].data_ptr(), out["pos"].data_ptr(),
                            out["uv"].data_ptr(), stream=st)
    st.synchronize()
    for key in out:
        assert cpm.same_bits(out[key].cpu().numpy(), want[key]), ("device", key)


# ---- the frame G-buffer ----
@pytest.mark.parametrize("scene", SCENES)
def test_render_hits(scenes, scene):
    g = scenes(scene)
    o = bsc.oracle_scene(scene)
    for kw in (dict(), dict(sub_pixel_res=2), dict(sub_pixel_res=2, focal_blur=True)):
        f = dw.frame(scene, **kw)
        want = gbm.hits(o, f, NEAREST)[2]
        got = g.render_hits(sr_frame(f))
        assert same_values(got, want), kw
        assert same_bits(banded(g, lambda: g.render_hits(sr_frame(f)), 1024 * f.sub_pixel_res ** 2), got), (kw, "passes")
        assert 0 < int(got["hit"].sum()) < got["hit"].size
    f = sr_frame(dw.frame(scene))
    n = g.sample_count(f)
    st = torch.cuda.Stream(DEV)
    out = hit_tensors(n)
    torch.cuda.synchronize(DEV)
    g.render_hits_device(f, 0, 0, *[out[k].data_ptr() for k in KEYS], stream=st)
    st.synchronize()
    assert same_bits(hits_back(out), g.render_hits(f))


# ---- the point calls ----
def point_tensors(scene):
    pos, nrm, col = dw.surface_points(scene)
    return dev(pos), dev(nrm), dev(col.view(np.int32)), torch.zeros(pos.shape[0], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("scene", SCENES)
def test_shadow_points(scenes, scene):
    g = scenes(scene)
    pos, nrm, col = dw.surface_points(scene)
    f = dw.frame(scene, shadows=True, shadow_samples=dw.SHADOW_SAMPLES)
    want = spm.shadowed(bsc.oracle_scene(scene), f, pos, nrm, col, NEAREST)
    for hook in (-1, 37, 38):
        for coherent in (False, True):
            got = with_hook(g, hook, lambda: g.shadow_points(sr_frame(f), pos, nrm, col, coherent=coherent))
            assert np.array_equal(got, want), (hook, coherent)
    assert np.array_equal(banded(g, lambda: g.shadow_points(sr_frame(f), pos, nrm, col), 128), want)
    st = torch.cuda.Stream(DEV)
    d_pos, d_nrm, d_col, d_out = point_tensors(scene)
    torch.cuda.synchronize(DEV)
    g.shadow_points_device(sr_frame(f), pos.shape[0], d_pos.data_ptr(), d_nrm.data_ptr(), d_col.data_ptr(), d_out.data_ptr(), stream=st)
    st.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize("scene", SCENES)
def test_static_shadow_points(scenes, scene):
    g = scenes(scene)
    pos, nrm, col = dw.surface_points(scene)
    f = dw.frame(scene, shadows=True, shadow_samples=dw.SHADOW_SAMPLES)
    amount, out, generators = sspm.static_shadow_points(bsc.oracle_scene(scene), f, pos, nrm, NEAREST, np.zeros(sspm.CELLS, dtype=np.uint8), col)
    for coherent in (False, True):
        g.reset_shadow_cache()
        got = g.static_shadow_points(sr_frame(f), pos, nrm, col, coherent=coherent)
        assert np.array_equal(got[0], out) and np.array_equal(got[1], amount) and got[2] == generators, coherent
    g.reset_shadow_cache()
    got = banded(g, lambda: g.static_shadow_points(sr_frame(f), pos, nrm, col), 128)
    assert np.array_equal(got[0], out) and np.array_equal(got[1], amount) and got[2] == generators
    g.reset_shadow_cache()
    st = torch.cuda.Stream(DEV)
    d_pos, d_nrm, d_col, d_out = point_tensors(scene)
    d_amount = torch.zeros(pos.shape[0], dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize(DEV)
    g.static_shadow_points_device(sr_frame(f), pos.shape[0], d_pos.data_ptr(), d_nrm.data_ptr(), d_col.data_ptr(), d_out.data_ptr(), d_amount.data_ptr(), stream=st)
    st.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), out) and np.array_equal(d_amount.cpu().numpy(), amount)
    g.reset_shadow_cache()


def seeded(scene, **kw):
    f = dw.frame(scene, **kw)
    f.random_seed = 20261021
    return f


@pytest.mark.parametrize("scene", SCENES)
def test_ao_points(scenes, scene):
    g = scenes(scene)
    o = bsc.oracle_scene(scene)
    pos, nrm, col = dw.surface_points(scene)
    f = seeded(scene, shading=False)
    for uncached in (False, True):
        flags = L.F_AO_UNCACHED if uncached else 0
        amount, out, generators = apm.ao_points(o, NEAREST, pos, nrm, f.random_seed, np.zeros(aom.RES ** 3, dtype=np.uint8), uncached=uncached, color=col)
        for hook in (-1, 44):
            g.reset_ao_cache()
            got = with_hook(g, hook, lambda: g.ao_points(sr_frame(f, flags), pos, nrm, col))
            assert np.array_equal(got[0], out) and np.array_equal(got[1], amount) and got[2] == generators, (uncached, hook)
        g.reset_ao_cache()
        got = banded(g, lambda: g.ao_points(sr_frame(f, flags), pos, nrm, col), 128)
        assert np.array_equal(got[0], out) and np.array_equal(got[1], amount) and got[2] == generators, (uncached, "passes")
        assert scene == "chain" or 0 < int((amount < 255).sum())          # (nothing faces the chain's one plane: tests/test_deep_walk_cases.py)
    g.reset_ao_cache()
    st = torch.cuda.Stream(DEV)
    d_pos, d_nrm, d_col, d_out = point_tensors(scene)
    d_amount = torch.zeros(pos.shape[0], dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize(DEV)
    g.ao_points_device(sr_frame(f, L.F_AO_UNCACHED), pos.shape[0], d_pos.data_ptr(), d_nrm.data_ptr(), d_col.data_ptr(), d_out.data_ptr(), d_amount.data_ptr(), stream=st)
    st.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), out) and np.array_equal(d_amount.cpu().numpy(), amount)
    g.reset_ao_cache()


@pytest.mark.parametrize("scene", SCENES)
def test_path_points(scenes, scene):
    g = scenes(scene)
    o = bsc.oracle_scene(scene)
    pos, nrm, col = dw.surface_points(scene)
    for shading in (False, True):
        f = seeded(scene, shading=shading)
        want = ppm.path_points(o, NEAREST, f, pos, nrm, col)
        for hook in (-1, 45):
            got = with_hook(g, hook, lambda: g.path_points(sr_frame(f), pos, nrm, col))
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (shading, hook)
        got = banded(g, lambda: g.path_points(sr_frame(f), pos, nrm, col), 128)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), (shading, "passes")
    assert scene == "chain" or len(set(want[1].tolist())) > 3            # some second rays hit, on triangles of more than one colour
    st = torch.cuda.Stream(DEV)
    d_pos, d_nrm, d_col, d_out = point_tensors(scene)
    d_in = torch.zeros(pos.shape[0], dtype=torch.int32, device=DEV)
    d_dirs = torch.zeros((pos.shape[0], 3), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize(DEV)
    g.path_points_device(sr_frame(f), pos.shape[0], d_pos.data_ptr(), d_nrm.data_ptr(), d_col.data_ptr(), d_out.data_ptr(), d_in.data_ptr(), d_dirs.data_ptr(), stream=st)
    st.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(d_in.cpu().numpy().view(np.uint32), want[1])
    assert np.array_equal(d_dirs.cpu().numpy(), want[2])


# ---- frames whose second rays are probes ----
def render_rows(g, f):
    got, _ = g.render(f)
    a, b = f.start_row, f.end_row
    return np.asarray(got).view(np.uint32).reshape(f.height, f.width)[a:b + 1]


@pytest.mark.parametrize("scene", SCENES)
def test_path_traced_and_ambient_occlusion_frames(scenes, scene):
    """The second rays on the walk route and (hooks 33, 34) one per lane; the path-traced frame in three row bands too (an
    ambient-occlusion frame takes one band only)."""
    g = scenes(scene)
    o = bsc.oracle_scene(scene)
    f = seeded(scene, concurrency=1)
    want = ptm.render(o, f, NEAREST)
    for hook in (-1, 33):
        got = with_hook(g, hook, lambda: render_rows(g, sr_frame(f, L.F_PATH_TRACING)))
        assert np.array_equal(got, want), ("path tracing", hook)
    assert np.array_equal(banded(g, lambda: render_rows(g, sr_frame(f, L.F_PATH_TRACING))), want), ("path tracing", "passes")
    f = aom.ao_frame(seeded(scene, concurrency=1))
    try:
        for hook in (-1, 34):
            g.reset_ao_cache()
            want = aom.AoModel().render(o, f, NEAREST)
            got = with_hook(g, hook, lambda: render_rows(g, sr_frame(f)))
            assert np.array_equal(got, want), ("ambient occlusion", hook)
    finally:
        g.reset_ao_cache()


@pytest.mark.parametrize("scene", SCENES)
def test_light_field_at_resolution_8(scenes, scene):
    """A frame that fills its cells, the same with shadowed cells, the bake of the whole table (hook 35: one lane per cell) and the
    lookup of caller-given rays."""
    g = scenes(scene)
    o = bsc.oracle_scene(scene)
    n = 8
    try:
        g.light_field_res = n
        for shadows in (False, True):
            g.light_field_shadows = shadows
            g.reset_light_field()
            model = lsm.LightFieldShadowModel(n) if shadows else lfm.LightFieldModel(n)
            f = lfm.lf_frame(dw.frame(scene, shadows=shadows, shadow_samples=dw.SHADOW_SAMPLES if shadows else 0))
            want = model.render(o, f, NEAREST)
            assert model.coord_margin > lfm.MARGIN and model.term_margin > lfm.MARGIN       # (the frame's input conditions)
            assert np.array_equal(render_rows(g, sr_frame(f)), want), shadows
            g.reset_light_field()
            assert np.array_equal(banded(g, lambda: render_rows(g, sr_frame(f))), want), (shadows, "passes")
            filled = np.flatnonzero(g.get_light_field())
            assert np.array_equal(filled, np.array(sorted(model.cache), dtype=np.int64)) and np.array_equal(g.get_light_field()[filled], model.entries(filled))
        g.light_field_shadows = False
        f = lfb.bake_frame(True, **(bsc.DEEP_POSE if scene == "deep" else {}))
        table = lfb.model_table(o, f, n, NEAREST)
        assert len(set(table.tolist())) > 10                             # the canonical rays of the cells meet many triangles
        for hook in (-1, 35):
            g.reset_light_field()
            assert with_hook(g, hook, lambda: g.bake_light_field(sr_frame(f))) == table.size
            assert np.array_equal(g.get_light_field(), table), hook
        s, d, _ = lrm.usable(*dw.ray_batch(scene), (n,))                 # (the call's input condition: no ray on a cell boundary)
        assert s.shape[0] > 200
        g.reset_light_field()
        rays = lrm.LightFieldRaysModel(lfm.LightFieldModel(n))
        want = rays.rays(o, f, s, d, NEAREST)
        got = g.light_field_rays(sr_frame(f), s, d)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        g.reset_light_field()
        got = banded(g, lambda: g.light_field_rays(sr_frame(f), s, d), 100)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        g.reset_light_field()
        st = torch.cuda.Stream(DEV)
        d_s, d_d = dev(s), dev(d)
        d_out = torch.zeros(s.shape[0], dtype=torch.int32, device=DEV)
        d_inside = torch.zeros(s.shape[0], dtype=torch.uint8, device=DEV)
        d_filled = torch.zeros(1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize(DEV)
        g.light_field_rays_device(sr_frame(f), s.shape[0], d_s.data_ptr(), d_d.data_ptr(), d_out.data_ptr(), d_inside.data_ptr(), stream=st,
                                  d_filled_ptr=d_filled.data_ptr())
        st.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(d_inside.cpu().numpy(), want[1])
        assert int(d_filled.cpu()[0]) == want[2]
        assert 0 < int(want[1].sum())
    finally:
        g.light_field_shadows = False
        g.light_field_res = 64
        g.reset_light_field()
