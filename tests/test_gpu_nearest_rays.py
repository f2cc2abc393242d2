"""Nearest-hit ray batches with a distance limit (sr_nearest_rays) on the GPU.  Every comparison is an exact equality over every ray and every
output: the call against sr_trace_rays of the same rays with the answers cut by their limit blanked (tests/nearest_rays_model.py), for regular
rays against the oracle's model, the schedules against each other, passes against one pass, the device variant against the host variant, the
decorators' second rays (sr_path_points' incoming, a mirror level of sr_render) against chains built on the call, and frames around the call
against themselves.  Scenes, ray sets and limits: tests/occluded_rays_cases.py (their shares of kept, cut and missing rays are checked on the
CPU in tests/test_nearest_rays_model.py); deep trees and ties: tests/bvh_shape_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import bvh_shape_cases as shapes
import bvh_shapes as bs
import gbuffer_cases as gbc
import occluded_rays_cases as occ
import softray_amd as sa
from helpers import make_frame, unit_cube_scene
from nearest_rays_model import KEYS, nearest_model, same_bits, same_values, take

pytestmark = pytest.mark.gpu
L = sa._lib
DEV = torch.device("cuda", 0)
MODES = {"tree": sa.MODE_REF_TREE, "brute": sa.MODE_BRUTE, "bvh": sa.MODE_BVH}
GUARD = 0x5A
VARIANTS = ("rot", None)                                   # the limits of a set: its rotation of every kind, and none
NP_TYPES = dict(hit=np.uint8, ray_frac=np.float64, pos=np.float64, normal=np.float64, color=np.uint32, tri_index=np.int32)
SIZE = {k: np.dtype(t).itemsize for k, t in NP_TYPES.items()}
WIDTH = dict(hit=1, ray_frac=1, pos=3, normal=3, color=1, tri_index=1)


class Scene:
    """One scene on the device (host-built and device-built own BVH) and in the oracle."""

    def __init__(self, name):
        self.name = name
        self.tris, self.prims = gbc.scene_data(name)
        self.tree, self.brute = gbc.oracle_scenes(name)
        self.gpus = {}
        self.traces = {}

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

    def trace(self, on_device, target, rs):
        """sr_trace_rays of a ray set, computed once and left unchanged."""
        key = (on_device, target, rs.name)
        if key not in self.traces:
            res = self.gpu(on_device).trace(target, rs.starts, rs.D)
            for a in res.values():
                a.setflags(write=False)
            self.traces[key] = res
        return self.traces[key]


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Scene(name)
        return made[name]
    return get


def limits_of(rs, variant):
    return None if variant is None else rs.limits[variant]


def call(g, target, rs, variant, **kw):
    return g.nearest(target, rs.starts, rs.dirs, limits=limits_of(rs, variant), endpoints=rs.endpoints, **kw)


def with_hook(g, hook, fn):
    g.debug_set(L.DBG_KERNEL_SWITCH, hook)
    try:
        return fn()
    finally:
        g.debug_set(L.DBG_KERNEL_SWITCH, -1)


# ---- 1. equals sr_trace_rays with the cut answers blanked, and for regular rays the oracle's model ----
@pytest.mark.parametrize("scene", occ.SCENES)
def test_equals_trace_rays_and_the_oracle(scenes, scene):
    sc = scenes(scene)
    kept = cut = 0
    for name in occ.SETS:
        rs = occ.ray_set(scene, name)
        for variant in VARIANTS:
            lim = limits_of(rs, variant)
            reg = rs.regular(variant) if variant is not None else occ.regular(rs.starts, rs.dirs, rs.endpoints, None)
            for mode in MODES:
                for root in (False, True):
                    target = MODES[mode] | (L.TARGET_ROOT if root else 0)
                    res = occ.oracle_trace(sc.tree, sc.brute, mode, root, sc.prims, np.ascontiguousarray(rs.starts[reg]), np.ascontiguousarray(rs.D[reg]))
                    model = None if res is None else nearest_model(res, None if lim is None else lim[reg])
                    for on_device in sc.builds():
                        g = sc.gpu(on_device)
                        traced = sc.trace(on_device, target, rs)
                        got = call(g, target, rs, variant)
                        label = (name, variant, mode, root, on_device)
                        assert set(np.unique(got["hit"])) <= {0, 1}, label
                        assert same_bits(got, nearest_model(traced, lim)), label
                        if lim is None:
                            assert same_bits(got, traced), label
                        if model is not None:
                            assert same_values(take(got, reg), model), label
                        kept += int(got["hit"].sum())
                        cut += int(traced["hit"].sum()) - int(got["hit"].sum())
    assert kept > 2000 and cut > 1000


def raw_call(h, target, n, starts, dirs, limits, outs, options, stats=None):
    """sr_nearest_rays with the outputs of `outs` (a dict keyed like KEYS; a missing key is NULL)."""
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)          # noqa: E731
    rc = L.lib().sr_nearest_rays(h, target, n, p(starts), p(dirs), p(limits), *[p(outs.get(k)) for k in KEYS], options, p(stats))
    return rc, (L.lib().sr_last_error().decode() if rc else "")


def test_any_subset_of_the_outputs_may_be_asked_for(scenes):
    sc = scenes("cube")
    g = sc.gpu(True)
    for name in ("irregular", "far", "n65"):
        rs = occ.ray_set("cube", name)
        lim = rs.limits["rot"]
        options = L.RAYS_ENDPOINTS if rs.endpoints else 0
        for mode in MODES.values():
            target = mode | L.TARGET_ROOT
            full = call(g, target, rs, "rot")
            two = dict(hit=np.full(rs.n, GUARD, dtype=np.uint8), ray_frac=np.full(rs.n, -7.0))
            assert raw_call(g._h, target, rs.n, rs.starts, rs.dirs, lim, two, options) == (0, "")
            assert same_bits(two, full, ("hit", "ray_frac"))
            rest = dict(pos=np.full((rs.n, 3), -7.0), normal=np.full((rs.n, 3), -7.0), color=np.full(rs.n, 7, dtype=np.uint32),
                        tri_index=np.full(rs.n, 7, dtype=np.int32))
            assert raw_call(g._h, target, rs.n, rs.starts, rs.dirs, lim, rest, options) == (0, "")
            assert same_bits(rest, full, ("pos", "normal", "color", "tri_index"))
            stats = np.full(4, 77, dtype=np.uint64)
            assert raw_call(g._h, target, rs.n, rs.starts, rs.dirs, lim, {}, options, stats) == (0, "")      # all NULL: runs for the statistics
            assert stats[0] == rs.n


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
                assert same_bits(base, nearest_model(sc.trace(on_device, target, rs), rs.limits["rot"]))
                assert same_bits(call(g, target, rs, "rot", coherent=True), base), (name, "coherent")
                # input order, every ray per lane, persistent lanes refilled at 0 / 24 / 63 busy ones, two stack levels in LDS
                for hook in (48, 49, 100, 124, 163, 202):
                    for coherent in (False, True):
                        assert same_bits(with_hook(g, hook, lambda: call(g, target, rs, "rot", coherent=coherent)), base), (name, hook, coherent)
                g.debug_set(L.DBG_BVH2_PACKETS, 1)                                # the walk on the binary tree
                try:
                    assert same_bits(call(g, target, rs, "rot"), base), (name, "binary")
                    assert same_bits(with_hook(g, 202, lambda: call(g, target, rs, "rot")), base), (name, "binary", 202)
                finally:
                    g.debug_set(L.DBG_BVH2_PACKETS, -1)
                assert same_bits(call(g, target, rs, "rot"), base)


# ---- 3. deep trees and ties ----
# (the staircase at the depth limit is the device build's)
SHAPES = [("chain", "at_triangles", False), ("chain", "at_triangles", True), ("chain", "through_point", False), ("chain", "through_point", True),
          ("chain", "near_miss", False), ("chain", "near_miss", True), ("duplicates", "at_triangles", False), ("duplicates", "at_triangles", True),
          ("limit", "at_triangles", True)]


@pytest.mark.parametrize("scene_name,family,on_device", SHAPES, ids=["%s-%s-%s" % (a, b, "device_built" if c else "host_built") for a, b, c in SHAPES])
def test_deep_trees_and_ties(scene_name, family, on_device):
    g = sa.GpuScene(0)
    g.set_triangles(*shapes.scene(scene_name))
    g.build((sa.MODE_BVH,), on_device=on_device)
    depth = g.bvh_stats()[0]
    if scene_name == "chain" and not on_device:
        assert depth >= 50                                                    # past the 24 stack levels of LDS
    s, d = shapes.ray_batch(scene_name, family)
    traced = g.trace(sa.MODE_BVH, s, d)
    want = shapes.oracle_trace(scene_name, family, "nearest")
    assert same_values(traced, want, shapes.TRACE_KEYS)
    f = np.where(traced["hit"].astype(bool), traced["ray_frac"], 1.0)
    for hook in (-1, 202, 49):
        free = with_hook(g, hook, lambda: g.nearest(sa.MODE_BVH, s, d))
        assert same_bits(free, traced), (hook, "no limits")
        assert same_values(free, want, shapes.TRACE_KEYS), (hook, "oracle")
        for coherent in (False, True):
            lim = occ.rotated_limits(f)
            got = with_hook(g, hook, lambda: g.nearest(sa.MODE_BVH, s, d, limits=lim, coherent=coherent))
            assert same_bits(got, nearest_model(traced, lim)), (hook, coherent)
    if family == "at_triangles":
        hit = traced["hit"].astype(bool)
        assert hit.any()
        if scene_name == "duplicates":                                        # four exact copies of every triangle: the lowest index wins
            lowest = bs.duplicate_groups(shapes.scene("duplicates")[0])
            got = g.nearest(sa.MODE_BVH, s, d)["tri_index"][hit]
            assert np.array_equal(lowest[got], got) and len(set(got.tolist())) > 50
    else:
        assert not traced["hit"].any()


# ---- 4. passes ----
@pytest.mark.parametrize("mode", ["bvh", "tree", "brute"])
def test_four_passes_equal_one_pass(scenes, mode):
    sc = scenes("cube")
    g = sc.gpu(True)
    rs = occ.ray_set("cube", "n449")
    target = MODES[mode] | L.TARGET_ROOT
    whole = call(g, target, rs, "rot", stats=True)
    assert same_bits(whole, nearest_model(sc.trace(True, target, rs), rs.limits["rot"]))
    assert whole["stats"][0] == 449
    for coherent in (False, True):
        g.debug_set(L.DBG_BAND_SAMPLES, 128)
        g.reset_kernel_times()
        g.debug_set(L.DBG_KERNEL_TIMING, 1)
        try:
            banded = call(g, target, rs, "rot", coherent=coherent, stats=True)
            times = g.kernel_times()
        finally:
            g.debug_set(L.DBG_BAND_SAMPLES, -1)
            g.debug_set(L.DBG_KERNEL_TIMING, -1)
        assert times["k_nearest"][1] == 4                                     # 3 x 128 + 65
        assert ("k_nearest_sort" in times) == (mode == "bvh") and (mode != "bvh" or times["k_nearest_sort"][1] == 4)
        assert same_bits(banded, whole), coherent
        assert banded["stats"][0] == 449
        if mode != "bvh":
            assert np.array_equal(banded["stats"], whole["stats"])
    if mode == "bvh":                                                         # ... and four passes with two stack levels in LDS
        g.debug_set(L.DBG_BAND_SAMPLES, 128)
        try:
            deep = with_hook(g, 202, lambda: call(g, target, rs, "rot", stats=True))
        finally:
            g.debug_set(L.DBG_BAND_SAMPLES, -1)
        assert same_bits(deep, whole) and deep["stats"][0] == 449


# ---- 5. the device variant on a stream of the caller's: guards, inputs, statistics ----
def run_device(g, target, rs, variant, stream=None, stats=False, coherent=False, keys=KEYS):
    n = rs.n
    lim = limits_of(rs, variant)
    d_starts, d_dirs = torch.from_numpy(rs.starts).to(DEV), torch.from_numpy(rs.dirs).to(DEV)
    d_lim = torch.from_numpy(lim).to(DEV) if lim is not None else None
    # 64 bytes of guard before and behind every output
    d_out = {k: torch.full((64 + n * WIDTH[k] * SIZE[k] + 64,), GUARD, dtype=torch.uint8, device=DEV) for k in keys}
    d_stats = torch.full((24,), -1, dtype=torch.int64, device=DEV) if stats else None
    torch.cuda.synchronize(DEV)
    ptr = {k: (d_out[k].data_ptr() + 64 if k in keys else 0) for k in KEYS}
    g.nearest_device(target, n, d_starts.data_ptr(), d_dirs.data_ptr(), d_lim.data_ptr() if d_lim is not None else 0, ptr["hit"], ptr["ray_frac"], ptr["pos"],
                     ptr["normal"], ptr["color"], ptr["tri_index"], endpoints=rs.endpoints, coherent=coherent, stream=stream if stream is not None else 0,
                     d_stats_ptr=d_stats.data_ptr() if stats else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize(DEV)
    guards_ok = True
    res = {}
    for k in keys:
        raw = d_out[k].cpu().numpy()
        guards_ok = guards_ok and bool(np.all(raw[:64] == GUARD) and np.all(raw[-64:] == GUARD))
        a = raw[64:-64].copy().view(NP_TYPES[k])
        res[k] = a.reshape(n, 3) if WIDTH[k] == 3 else a
    inputs_ok = (np.array_equal(d_starts.cpu().numpy().view(np.uint64), rs.starts.view(np.uint64)) and
                 np.array_equal(d_dirs.cpu().numpy().view(np.uint64), rs.dirs.view(np.uint64)) and
                 (d_lim is None or np.array_equal(d_lim.cpu().numpy().view(np.uint64), lim.view(np.uint64))))
    return res, guards_ok, inputs_ok, (d_stats.cpu().numpy().view(np.uint64) if stats else None)


@pytest.mark.parametrize("mode", ["tree", "brute", "bvh"])
@pytest.mark.parametrize("name", ["irregular", "irregular_ends", "n65"])
def test_device_variant_on_a_stream_guards_and_statistics(scenes, mode, name):
    sc = scenes("cube")
    g = sc.gpu(True)
    rs = occ.ray_set("cube", name)
    target = MODES[mode] | L.TARGET_ROOT
    st = torch.cuda.Stream(DEV)
    for variant in VARIANTS:
        host = call(g, target, rs, variant, stats=True)
        last = g.ray_stats()
        assert np.array_equal(last[:4], host["stats"]) and not last[4:].any() and host["stats"][0] == rs.n
        got, guards_ok, inputs_ok, stats = run_device(g, target, rs, variant, stream=st, stats=True)
        assert guards_ok and inputs_ok
        assert same_bits(got, host)
        assert stats[0] == rs.n and not stats[4:].any()
        assert np.array_equal(stats, last)                                    # (the own BVH's counters are what the walks fetched, the same walks in both variants)
        if mode != "bvh":
            cnt = g.trace(target, rs.starts, rs.D, counters=True)["counters"].astype(np.uint64)
            assert np.array_equal(stats[1:4], cnt.sum(axis=0))
        got2, guards_ok, inputs_ok, none = run_device(g, target, rs, variant, coherent=True)
        assert guards_ok and inputs_ok and none is None and same_bits(got2, host)
        two, guards_ok, inputs_ok, _ = run_device(g, target, rs, variant, stream=st, keys=("hit", "ray_frac"))
        assert guards_ok and inputs_ok and same_bits(two, host, ("hit", "ray_frac"))


# ---- 6. refusals ----
def raw_call_device(h, target, n, starts, dirs, limits, outs, options):
    v = lambda t: None if t is None else C.c_void_p(t.data_ptr())              # noqa: E731
    rc = L.lib().sr_nearest_rays_device(h, target, n, v(starts), v(dirs), v(limits), *[v(outs.get(k)) for k in KEYS], options, None, None)
    return rc, (L.lib().sr_last_error().decode() if rc else "")


def test_refusals_in_the_headers_order(scenes):
    sc = scenes("cube")
    g = sc.gpu(True)
    s = np.zeros((4, 3)); d = np.ones((4, 3))
    outs = dict(hit=np.full(4, GUARD, dtype=np.uint8), ray_frac=np.full(4, 7.0), pos=np.full((4, 3), 7.0), normal=np.full((4, 3), 7.0),
                color=np.full(4, 7, dtype=np.uint32), tri_index=np.full(4, 7, dtype=np.int32))
    untouched = lambda: np.all(outs["hit"] == GUARD) and all(np.all(outs[k] == 7) for k in KEYS[1:])        # noqa: E731
    bare = sa.GpuScene(0)                                                    # no model
    unbuilt = sa.GpuScene(0)                                                 # a model, no tree
    unbuilt.set_triangles(*sc.tris)
    host = sa.GpuScene(-1)                                                   # a model and its reference tree, no device
    host.set_triangles(*sc.tris)
    host.build((sa.MODE_REF_TREE,))
    bvh, vox = sa.MODE_BVH, L.TARGET_VOXELS
    options_text = "sr_nearest_rays: unknown option bits (SR_RAYS_COHERENT and SR_RAYS_ENDPOINTS are the options)"
    no_device = "sr_nearest_rays: a host-only scene has no HIP device to walk on (compute is never emulated on the CPU)"
    # every row breaks the rule it names and every later one it can: the earliest refusal is the one reported
    table = [
        ((None, vox, -1, None, None, None, outs, 4), L.SR_ERR_INVALID_ARG, "sr_nearest_rays: the scene is NULL"),
        ((bare._h, vox, -1, None, None, None, outs, 4), L.SR_ERR_INVALID_ARG, "sr_nearest_rays: n is negative"),
        ((bare._h, vox, 4, None, d, None, outs, 4), L.SR_ERR_INVALID_ARG, "sr_nearest_rays: starts and dirs must not be NULL when n > 0"),
        ((bare._h, vox, 4, s, None, None, outs, 4), L.SR_ERR_INVALID_ARG, "sr_nearest_rays: starts and dirs must not be NULL when n > 0"),
        ((bare._h, vox, 4, s, d, None, outs, 4), L.SR_ERR_INVALID_ARG, options_text),
        ((bare._h, vox, 0, None, None, None, {}, 1 << 31), L.SR_ERR_INVALID_ARG, options_text),
        ((bare._h, vox | bvh, 4, s, d, None, outs, 3), L.SR_ERR_UNSUPPORTED,
         "sr_nearest_rays: the voxel grid (SR_TARGET_VOXELS) has no tree to walk and its hits have rayFrac 0; use sr_trace_rays"),
        ((bare._h, bvh, 4, s, d, None, outs, 0), L.SR_ERR_NO_MODEL, "sr_nearest_rays: the scene has no model (sr_set_triangles, sr_load_3ds)"),
        ((unbuilt._h, bvh, 4, s, d, None, outs, 0), L.SR_ERR_NOT_BUILT, "SR_MODE_BVH needs sr_build(1 << SR_MODE_BVH)"),
        ((unbuilt._h, sa.MODE_REF_TREE | L.TARGET_ROOT, 4, s, d, None, outs, 0), L.SR_ERR_NOT_BUILT, "SR_MODE_REF_TREE needs sr_build(1 << SR_MODE_REF_TREE)"),
        ((host._h, bvh, 4, s, d, None, outs, 0), L.SR_ERR_NOT_BUILT, "SR_MODE_BVH needs sr_build(1 << SR_MODE_BVH)"),
        ((host._h, sa.MODE_REF_TREE, 4, s, d, None, outs, 0), L.SR_ERR_NO_DEVICE, no_device),
        ((host._h, sa.MODE_REF_TREE, 0, None, None, None, {}, 0), L.SR_ERR_NO_DEVICE, no_device),
    ]
    for args, code, message in table:
        assert raw_call(*args) == (code, message), message
        assert untouched()
    # the device variant refuses the same way, with the same messages
    d_s, d_d = torch.zeros((4, 3), dtype=torch.float64, device=DEV), torch.ones((4, 3), dtype=torch.float64, device=DEV)
    d_outs = dict(hit=torch.full((4,), GUARD, dtype=torch.uint8, device=DEV), ray_frac=torch.full((4,), 7.0, dtype=torch.float64, device=DEV))
    for (h, target, n, a, b, options), code, message in (
            ((None, bvh, 4, d_s, d_d, 0), L.SR_ERR_INVALID_ARG, "sr_nearest_rays: the scene is NULL"),
            ((g._h, bvh, -1, d_s, d_d, 0), L.SR_ERR_INVALID_ARG, "sr_nearest_rays: n is negative"),
            ((g._h, bvh, 4, d_s, None, 0), L.SR_ERR_INVALID_ARG, "sr_nearest_rays: starts and dirs must not be NULL when n > 0"),
            ((g._h, bvh, 4, d_s, d_d, 8), L.SR_ERR_INVALID_ARG, options_text),
            ((g._h, vox, 4, d_s, d_d, 0), L.SR_ERR_UNSUPPORTED,
             "sr_nearest_rays: the voxel grid (SR_TARGET_VOXELS) has no tree to walk and its hits have rayFrac 0; use sr_trace_rays"),
            ((bare._h, bvh, 4, d_s, d_d, 0), L.SR_ERR_NO_MODEL, "sr_nearest_rays: the scene has no model (sr_set_triangles, sr_load_3ds)"),
            ((unbuilt._h, bvh, 4, d_s, d_d, 0), L.SR_ERR_NOT_BUILT, "SR_MODE_BVH needs sr_build(1 << SR_MODE_BVH)"),
            ((host._h, sa.MODE_REF_TREE, 4, d_s, d_d, 0), L.SR_ERR_NO_DEVICE, no_device)):
        assert raw_call_device(h, target, n, a, b, None, d_outs, options) == (code, message), message
    torch.cuda.synchronize(DEV)
    assert bool((d_outs["hit"] == GUARD).all()) and bool((d_outs["ray_frac"] == 7.0).all())
    # n == 0 that passes every check: SR_OK, nothing is touched -- with arrays and without
    stats = np.full(4, 77, dtype=np.uint64)
    before = g.ray_stats().copy()
    for target in (bvh, sa.MODE_REF_TREE | L.TARGET_ROOT, sa.MODE_BRUTE):
        assert raw_call(g._h, target, 0, s, d, None, outs, 3, stats) == (0, "")
        assert raw_call(g._h, target, 0, None, None, None, {}, 0) == (0, "")
        assert raw_call_device(g._h, target, 0, None, None, None, {}, 0) == (0, "")
    assert untouched() and np.all(stats == 77) and np.array_equal(g.ray_stats(), before)
    with pytest.raises(sa.SoftrayError):
        g.nearest(bvh | vox, s, d)


# ---- 7. state ----
def as_sr(frame, mode="bvh", extra_flags=0):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = MODES[mode]
    f.flags |= extra_flags
    return f


def test_a_shadowed_frame_before_and_after_the_call_is_the_same_frame(scenes):
    sc = scenes("cube")
    g = sa.GpuScene(0)                                                       # a scene of its own: the frames' hints stay here
    g.set_triangles(*sc.tris)
    g.set_extra(list(sc.prims))
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=True)
    f = as_sr(gbc.frame_of(("cube", "out", 200, 160, None, 1, False), shadows=True))
    rs = occ.ray_set("cube", "irregular")
    target = sa.MODE_BVH | L.TARGET_ROOT
    want = nearest_model(g.trace(target, rs.starts, rs.D), rs.limits["rot"])
    first = np.asarray(g.render(f)[0]).view(np.uint32).ravel().copy()
    assert same_bits(call(g, target, rs, "rot"), want)
    for _ in range(2):
        assert np.array_equal(np.asarray(g.render(f)[0]).view(np.uint32).ravel(), first)
        assert same_bits(call(g, target, rs, "rot", coherent=True), want)
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
        d_out = {k: torch.full((rs.n * WIDTH[k] * SIZE[k],), GUARD, dtype=torch.uint8, device=DEV) for k in KEYS}
        px = [torch.zeros(200 * 160, dtype=torch.int32, device=DEV) for _ in range(2)]
        torch.cuda.synchronize(DEV)
        g.render_device(f, px[0].data_ptr(), s1.cuda_stream)
        g.nearest_device(target, rs.n, d_starts.data_ptr(), d_dirs.data_ptr(), d_lim.data_ptr(), *[d_out[k].data_ptr() for k in KEYS], endpoints=rs.endpoints,
                         stream=s2)
        g.render_device(f2, px[1].data_ptr(), s3.cuda_stream)
        torch.cuda.synchronize(DEV)
        got = {k: d_out[k].cpu().numpy().view(NP_TYPES[k]) for k in KEYS}
        got["pos"], got["normal"] = got["pos"].reshape(-1, 3), got["normal"].reshape(-1, 3)
        assert same_bits(got, want)
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
            got = call(g, target, rs, "rot", stats=True)
            assert same_bits(got, call(g1, target, rs, "rot"))
            assert got["stats"][0] == rs.n and np.array_equal(g.ray_stats()[:4], got["stats"])      # the first part's, reported by the multi-device scene
            dev, guards_ok, inputs_ok, _ = run_device(g, target, rs, "rot")
            assert guards_ok and inputs_ok and same_bits(dev, got)


def test_after_a_refit_the_call_equals_trace_rays_on_the_refit_scene():
    v9, argb, lo, hi = unit_cube_scene(1500, seed=4242)
    g = sa.GpuScene(0)
    g.set_triangles(v9, argb, lo, hi)
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=True)
    rs = occ.ray_set("cube", "segments")                                      # (the same box)
    before = call(g, sa.MODE_BVH, rs, "rot")
    assert same_bits(before, nearest_model(g.trace(sa.MODE_BVH, rs.starts, rs.D), rs.limits["rot"]))
    moved = np.ascontiguousarray(v9.reshape(-1, 3, 3) * np.array([0.9, 0.8, 0.95]) + np.array([0.02, -0.03, 0.01])).reshape(v9.shape)
    g.refit_triangles_device(torch.from_numpy(moved.reshape(-1, 3, 3)).to(DEV), None, lo, hi)
    torch.cuda.synchronize(DEV)
    traced = g.trace(sa.MODE_BVH, rs.starts, rs.D)
    for variant in VARIANTS:
        after = call(g, sa.MODE_BVH, rs, variant)
        assert same_bits(after, nearest_model(traced, limits_of(rs, variant)))
        assert 0 < after["hit"].sum() < rs.n
    assert not same_bits(call(g, sa.MODE_BVH, rs, "rot"), before)
    fresh = sa.GpuScene(0)
    fresh.set_triangles(moved, argb, lo, hi)
    fresh.build((sa.MODE_BVH,), on_device=True)
    for variant in VARIANTS:
        assert same_bits(call(g, sa.MODE_BVH, rs, variant), call(fresh, sa.MODE_BVH, rs, variant))


# ---- 8. the decorator chain: second rays ----
@pytest.mark.parametrize("shading", [False, True], ids=["plain", "shaded"])
@pytest.mark.parametrize("mode", ["tree", "brute", "bvh"])
def test_path_points_incoming_is_the_call_plus_shade_points(scenes, mode, shading):
    sc = scenes("cube")
    g = sc.gpu(True)
    hits = g.render_hits(as_sr(gbc.frame_of(("cube", "out", 64, 48, None, 1, False)), mode))
    idx = np.flatnonzero(hits["hit"])
    pos, nrm = np.ascontiguousarray(hits["pos"][idx]), np.ascontiguousarray(hits["normal"][idx])
    assert pos.shape[0] > 300
    f = sa.Frame.from_buffer_copy(bytes(make_frame(16, shading=shading)))
    f.trace_mode = MODES[mode]
    f.random_seed = 1234567890
    _, incoming, dirs = g.path_points(f, pos, nrm, None, want_out=False)
    origin = pos + nrm * 0.001                                                # one multiply and one add, as PathTracingMethod.cs
    second = g.nearest(L.TARGET_ROOT | MODES[mode], origin, dirs)
    col = second["color"]
    if shading:
        col = g.shade_points(f, second["pos"], second["normal"], col)
    got = np.where(second["hit"].astype(bool), col, 0).astype(np.uint32)
    assert np.array_equal(got, incoming)
    assert 0 < int(second["hit"].sum()) and len(set(incoming.tolist())) > 20
    # with a limit the chain sees what lies within it and nothing else
    lim = np.full(pos.shape[0], float(np.median(second["ray_frac"][second["hit"].astype(bool)])))
    near = g.nearest(L.TARGET_ROOT | MODES[mode], origin, dirs, limits=lim)
    assert same_bits(near, nearest_model(second, lim)) and 0 < near["hit"].sum() < second["hit"].sum()


def blend(surface, reflected, k):
    """The header's per-channel fold: ((s * (255 - k)) >> 8) + ((r * k) >> 8), alpha 0xFF."""
    out = np.full(surface.shape, 0xFF000000, dtype=np.uint32)
    for shift in (16, 8, 0):
        s = (surface >> shift) & 0xFF
        r = (reflected >> shift) & 0xFF
        out |= ((((s * (255 - k)) >> 8) + ((r * k) >> 8)) & 0xFF) << shift
    return out.astype(np.uint32)


def test_a_mirror_level_of_a_frame_is_the_callers_loop(scenes):
    sc = scenes("cube")
    g = sc.gpu(True)
    W, H = 64, 48
    f = as_sr(gbc.frame_of(("cube", "out", W, H, None, 1, False)))           # shading on, no shadows, one sample per pixel, the extra geometry
    f.max_bounces, f.reflectivity = 1, 0.5
    assert f.flags & L.F_SHADING
    want = np.asarray(g.render(f)[0]).view(np.uint32).ravel()
    plain = sa.Frame.from_buffer_copy(bytes(f))                              # the same frame without the mirror level: the G-buffer and the shading
    plain.max_bounces = 0
    hits = g.render_hits(plain, rays=True)
    first = hits["hit"].astype(bool)
    d, n, p = hits["dirs"][first], hits["normal"][first], hits["pos"][first]
    dn = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]          # Dot(dir, n)
    r = d - n * (2.0 * dn)[:, None]                                           # dir - n * (2.0 * Dot(dir, n))
    start = p + n * 0.001
    second = g.nearest(L.TARGET_ROOT | sa.MODE_BVH, start, r)
    again = second["hit"].astype(bool)
    background = np.uint32(0xFF000000 | (f.background_argb & 0xFFFFFF))
    level0 = g.shade_points(plain, p, n, hits["color"][first])
    level1 = np.full(level0.shape, background, dtype=np.uint32)
    level1[again] = g.shade_points(plain, second["pos"][again], second["normal"][again], second["color"][again])
    k = int(f.reflectivity * 255.0) & 0xFF
    got = np.full(W * H, background, dtype=np.uint32)
    got[first] = blend(level0, level1, k)
    assert np.array_equal(got, want)
    assert first.sum() > 500 and 50 < again.sum() < first.sum() and len(set(want.tolist())) > 100
