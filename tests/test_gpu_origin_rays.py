"""Ray batches from one origin (sr_trace_origin_rays) on the GPU.  Every comparison is an exact equality over every ray and every output
array: the call against sr_trace_rays of the same rays with the origin tiled, for regular rays against the oracle, the schedules against each
other, passes against one pass, the device variant against the host variant, and frames around the call against themselves and the oracle.
Scenes, origins and direction sets: tests/origin_rays_cases.py (their hit counts are checked on the CPU in tests/test_origin_rays_model.py)."""
import os

import numpy as np
import pytest
import torch

import gbuffer_cases as gbc
import origin_rays_cases as oc
import softray_amd as sa
from helpers import make_frame, orc, unit_cube_scene

pytestmark = pytest.mark.gpu
L = sa._lib
DEV = torch.device("cuda", 0)
MODES = {"tree": sa.MODE_REF_TREE, "brute": sa.MODE_BRUTE, "bvh": sa.MODE_BVH}
KEYS = ("hit", "ray_frac", "pos", "normal", "color", "tri_index")
ITEM = dict(hit=(np.uint8, 1), ray_frac=(np.float64, 1), pos=(np.float64, 3), normal=(np.float64, 3), color=(np.uint32, 1), tri_index=(np.int32, 1))
GUARD = 0x5A
NCPU = os.cpu_count() or 1


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, want):
    want = np.asarray(want).reshape(got.shape)
    return np.array_equal(bits(got), bits(want))


def same_hits(got, want, rows=None):
    if rows is None:
        return all(same(got[k], want[k]) for k in KEYS)
    return all(same(np.ascontiguousarray(got[k][rows]), np.ascontiguousarray(np.asarray(want[k]).reshape(got[k].shape)[rows])) for k in KEYS)


def tiled(origin, n):
    return np.ascontiguousarray(np.tile(np.asarray(origin, dtype=np.float64), (n, 1)))


class Scene:
    """One scene on the device (host-built and device-built own BVH) and in the oracle."""

    def __init__(self, name):
        self.name = name
        self.tris, self.prims = gbc.scene_data(name)
        self.tree, self.brute = gbc.oracle_scenes(name)
        self.gpus = {}

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
        return (None,) if self.name == "small" else (False, True)       # (at most 64 triangles: the library builds on the host by itself)


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Scene(name)
        return made[name]
    return get


def known_axes(g):
    return (g.debug_counters()[5] >> 4) & 7


# ---- 1. equals sr_trace_rays, and for regular rays the oracle ----
@pytest.mark.parametrize("origin", oc.ORIGINS)
@pytest.mark.parametrize("scene", oc.SCENES)
def test_equals_trace_rays_and_the_oracle(scenes, scene, origin):
    sc = scenes(scene)
    o = oc.origin_of(scene, origin)
    some_hit = False
    for name in oc.SETS:
        dirs = oc.dirs_of(scene, origin, name)
        reg = oc.regular(dirs)
        starts = tiled(o, dirs.shape[0])
        for mode in MODES:
            for root in (False, True):
                target = MODES[mode] | (L.TARGET_ROOT if root else 0)
                model = oc.oracle_trace(sc.tree, sc.brute, mode, root, sc.prims, o, np.ascontiguousarray(dirs[reg]))
                for on_device in sc.builds():
                    g = sc.gpu(on_device)
                    if scene == "small":
                        assert g.bvh_stats()[3] == 0
                    got = g.trace_origin(target, o, dirs, coherent=oc.coherent_ok(name))
                    want = g.trace(target, starts, dirs)
                    assert same_hits(got, want), (name, mode, root, on_device)
                    if model is not None:
                        assert all(same(np.ascontiguousarray(got[k][reg]), model[k]) for k in KEYS), (name, mode, root, on_device)
                    miss = got["hit"] == 0
                    assert np.all(got["tri_index"][miss] == -1) and not got["pos"][miss].any() and not got["color"][miss].any()
                    some_hit |= bool(got["hit"].any())
    assert some_hit


# ---- 2. the schedules agree ----
@pytest.mark.parametrize("origin", ["out", "one", "centre", "plane"])
@pytest.mark.parametrize("scene", oc.SCENES)
def test_schedules_agree(scenes, scene, origin):
    sc = scenes(scene)
    o = oc.origin_of(scene, origin)
    for on_device in sc.builds():
        g = sc.gpu(on_device)
        for name in ("tiles", "sphere", "irregular", "n65"):
            dirs = oc.dirs_of(scene, origin, name)
            for target in (sa.MODE_BVH, sa.MODE_BVH | L.TARGET_ROOT):
                base = g.trace_origin(target, o, dirs)
                known = known_axes(g)
                if scene != "small":                      # (whatever tree so few triangles get)
                    # (near, far) planes exactly when the origin is outside the root box's slab on all three axes
                    assert known == (7 if origin == "out" else 0), (origin, known)
                assert same_hits(g.trace_origin(target, o, dirs, coherent=True), base), (name, "coherent")
                for key, value in ((L.DBG_PER_LANE_PRIMARY, 1), (L.DBG_BVH2_PACKETS, 1), (L.DBG_KERNEL_SWITCH, 61), (L.DBG_KERNEL_SWITCH, 71),
                                   (L.DBG_KERNEL_SWITCH, 72)):
                    # (hook 61 speaks when the ordered copy is made: a call from elsewhere first, so that this origin's copy is made under it --
                    # and again afterwards, so that the next one is made without it)
                    rekey = (key, value) == (L.DBG_KERNEL_SWITCH, 61)
                    g.debug_set(key, value)
                    try:
                        if rekey:
                            g.trace_origin(target, o + 0.37, dirs[:1])
                        for coherent in (False, True):
                            assert same_hits(g.trace_origin(target, o, dirs, coherent=coherent), base), (name, key, value, coherent)
                        if rekey:
                            assert known_axes(g) == 0
                    finally:
                        g.debug_set(key, -1)
                    if rekey:
                        g.trace_origin(target, o + 0.37, dirs[:1])
                assert same_hits(g.trace_origin(target, o, dirs), base)


def test_origins_beyond_the_packet_rule_take_private_walks(scenes):
    """An origin further from the box than 2^20 diagonals (include/softray.h) runs per lane: no order is made, the answers are sr_trace_rays'."""
    sc = scenes("cube")
    g = sc.gpu(True)
    lo, hi = oc.box("cube")
    c, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    rows, cols = np.mgrid[0:16, 0:24]
    for away, packets in ((2.0 ** 19, True), (2.0 ** 21, False), (1e150, False)):
        o = c + away * diag * np.array([1.0, -0.5, 0.25])
        fwd = c - o
        dist = float(np.linalg.norm(fwd))
        right = np.cross(fwd / dist, [0.0, 1.0, 0.0])
        right /= np.linalg.norm(right)
        up = np.cross(right, fwd / dist)
        half = 0.45 * diag
        dirs = np.ascontiguousarray((fwd[None, :] + (((cols + 0.5) / 24 - 0.5) * 2 * half).reshape(-1, 1) * right[None, :] +
                                     (((rows + 0.5) / 16 - 0.5) * 2 * half).reshape(-1, 1) * up[None, :]) * (min(dist / 100.0, 2.0 ** 30) / dist))
        assert oc.regular(dirs).all()
        for target in (sa.MODE_BVH, sa.MODE_BVH | L.TARGET_ROOT):
            g.reset_kernel_times()
            g.debug_set(L.DBG_KERNEL_TIMING, 1)
            try:
                got = g.trace_origin(target, o, dirs)
                times = g.kernel_times()
            finally:
                g.debug_set(L.DBG_KERNEL_TIMING, -1)
            assert ("k_origin_sort" in times) == packets and times["k_origin_rays"][1] == 1, (away, times)
            assert same_hits(got, g.trace(target, tiled(o, dirs.shape[0]), dirs)), away
            if away < 1e100:
                assert 0.1 * dirs.shape[0] < got["hit"].sum() < 0.9 * dirs.shape[0], (away, int(got["hit"].sum()))


# ---- 3. passes ----
@pytest.mark.parametrize("mode", ["bvh", "tree"])
def test_passes_equal_one_pass(scenes, mode):
    sc = scenes("cube")
    g = sc.gpu(True)
    o = oc.origin_of("cube", "out")
    dirs = np.ascontiguousarray(np.concatenate([oc.dirs_of("cube", "out", "irregular"), oc.dirs_of("cube", "out", "grid")])[:1000])
    assert (~oc.regular(dirs)).sum() > 50
    target = MODES[mode] | L.TARGET_ROOT
    whole = g.trace_origin(target, o, dirs, stats=True)
    assert same_hits(whole, g.trace(target, tiled(o, 1000), dirs))
    for coherent in (False, True):
        g.debug_set(L.DBG_BAND_SAMPLES, 128)
        g.reset_kernel_times()
        g.debug_set(L.DBG_KERNEL_TIMING, 1)
        try:
            banded = g.trace_origin(target, o, dirs, coherent=coherent, stats=True)
            times = g.kernel_times()
        finally:
            g.debug_set(L.DBG_BAND_SAMPLES, -1)
            g.debug_set(L.DBG_KERNEL_TIMING, -1)
        assert times["k_origin_rays"][1] == 8                                 # 7 x 128 + 104
        assert ("k_origin_sort" in times) == (mode == "bvh")
        assert same_hits(banded, whole), coherent
        assert banded["stats"][0] == 1000
        if mode == "tree":
            assert np.array_equal(banded["stats"], whole["stats"])


# ---- 4. the device variant: guards, subsets, statistics ----
def run_device(g, target, origin, dirs, wanted, coherent=False, stream=None, stats=False):
    """The device variant into guard-fenced torch buffers: ({name: array}, all guards intact, d_stats or None)."""
    n = dirs.shape[0]
    d_dirs = torch.from_numpy(dirs).to(DEV)
    bufs, ptrs = {}, {}
    for name in KEYS:
        dt, k = ITEM[name]
        nbytes = n * k * np.dtype(dt).itemsize
        if name in wanted:
            bufs[name] = torch.full((64 + nbytes + 64,), GUARD, dtype=torch.uint8, device=DEV)
            ptrs["d_" + name] = bufs[name].data_ptr() + 64
    d_stats = torch.full((24,), -1, dtype=torch.int64, device=DEV) if stats else None
    torch.cuda.synchronize(DEV)
    g.trace_origin_device(target, origin, n, d_dirs.data_ptr(), coherent=coherent, stream=stream if stream is not None else 0,
                          d_stats_ptr=d_stats.data_ptr() if stats else None, **ptrs)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize(DEV)
    out, guards_ok = {}, True
    for name, b in bufs.items():
        dt, k = ITEM[name]
        raw = b.cpu().numpy()
        guards_ok &= bool(np.all(raw[:64] == GUARD) and np.all(raw[-64:] == GUARD))
        a = raw[64:-64].copy().view(dt)
        out[name] = a.reshape(-1, 3) if k == 3 else a
    return out, guards_ok, (d_stats.cpu().numpy().view(np.uint64) if stats else None)


@pytest.mark.parametrize("mode", ["tree", "brute", "bvh"])
@pytest.mark.parametrize("origin", ["out", "centre"])
def test_device_variant_subsets_guards_and_statistics(scenes, mode, origin):
    sc = scenes("cube")
    g = sc.gpu(True)
    o = oc.origin_of("cube", origin)
    dirs = oc.dirs_of("cube", origin, "irregular")
    target = MODES[mode] | L.TARGET_ROOT
    host = g.trace_origin(target, o, dirs, stats=True)
    assert np.array_equal(g.ray_stats()[:4], host["stats"]) and not g.ray_stats()[4:].any()
    full, ok, st = run_device(g, target, o, dirs, KEYS, stats=True)
    assert ok and same_hits(full, host)
    assert np.array_equal(st[:4], host["stats"]) and not st[4:].any() and st[0] == dirs.shape[0]
    if mode != "bvh":
        cnt = g.trace(target, tiled(o, dirs.shape[0]), dirs, counters=True)["counters"].astype(np.uint64)
        assert np.array_equal(st[1:4], cnt.sum(axis=0))
    for name in KEYS:
        one, ok, _ = run_device(g, target, o, dirs, (name,), coherent=True)
        assert ok and list(one) == [name] and same(one[name], full[name]), name
    none, ok, st2 = run_device(g, target, o, dirs, (), stats=True)
    assert not none and ok and np.array_equal(st2, st)
    assert L.lib().sr_trace_origin_rays(g._h, target, o.ctypes.data, dirs.shape[0], dirs.ctypes.data, *([None] * 6), 0, None) == 0    # all NULL: legal
    assert np.array_equal(g.ray_stats()[:4], st[:4])


# ---- 5. the scene is left as a frame leaves it ----
def as_sr(frame, mode="bvh"):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = MODES[mode]
    return f


@pytest.mark.parametrize("size", [(200, 160), (512, 384)], ids=["direct", "persistent"])
def test_frames_around_the_call_are_unchanged(scenes, size):
    """A shaded frame with 100-sample point-light shadows at pose A, the call from an origin that is neither A's camera nor the light, frame A
    again: pixel-identical and the oracle's.  512 x 384 under hook 831 is the smallest frame tests/test_gpu_fuzz.py sends to the persistent
    grid of the shaft walk.  The same around sr_render_hits and sr_shadow_points."""
    sc = scenes("cube")
    g = sa.GpuScene(0)                                                   # a scene of its own: the hook and the frames' hints stay here
    g.set_triangles(*sc.tris)
    g.set_extra(list(sc.prims))
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=True)
    if size[0] >= 512:
        g.debug_set(L.DBG_KERNEL_SWITCH, 831)
    frame = gbc.frame_of(("cube", "out", size[0], size[1], None, 1, False), shadows=True)      # shadow_samples 0: the reference's 100
    f = as_sr(frame)
    want = np.zeros(size[0] * size[1], dtype=np.int32)
    sc.tree.render(frame, threads=NCPU, out=want)
    want = want.view(np.uint32)
    o = oc.origin_of("cube", "one")
    dirs = oc.dirs_of("cube", "one", "sphere")
    target = sa.MODE_BVH | L.TARGET_ROOT
    ref = g.trace(target, tiled(o, dirs.shape[0]), dirs)
    first, _ = g.render(f)
    first = np.asarray(first).view(np.uint32).ravel().copy()
    assert np.array_equal(first, want)
    assert same_hits(g.trace_origin(target, o, dirs), ref)
    for _ in range(2):
        again, _ = g.render(f)
        assert np.array_equal(np.asarray(again).view(np.uint32).ravel(), first)
    # sr_render_hits and sr_shadow_points of pose A, the call between them and after them
    hits = g.render_hits(f)
    assert same_hits(g.trace_origin(target, o, dirs, coherent=True), ref)
    assert same_hits(g.render_hits(f), hits)
    idx = np.flatnonzero(hits["hit"])[:4096]
    pos, nrm, col = hits["pos"][idx], hits["normal"][idx], hits["color"][idx]
    shadowed = g.shadow_points(f, pos, nrm, col)
    assert same_hits(g.trace_origin(target, o, dirs), ref)
    assert np.array_equal(g.shadow_points(f, pos, nrm, col), shadowed)
    again, _ = g.render(f)
    assert np.array_equal(np.asarray(again).view(np.uint32).ravel(), want)


def test_call_after_refit_and_after_a_new_build():
    v9, argb, lo, hi = unit_cube_scene(1500, seed=4242)
    g = sa.GpuScene(0)
    g.set_triangles(v9, argb, lo, hi)
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=True)
    o = oc.origin_of("cube", "one")                                       # (the same box: outside it on one axis)
    dirs = oc.sphere_dirs()
    starts = tiled(o, dirs.shape[0])
    before = g.trace_origin(sa.MODE_BVH, o, dirs)
    assert same_hits(before, g.trace(sa.MODE_BVH, starts, dirs)) and before["hit"].sum() > 20
    # moved vertices, the device-built tree refit (sr_refit_triangles_device)
    moved = np.ascontiguousarray(v9.reshape(-1, 3, 3) * np.array([0.9, 0.8, 0.95]) + np.array([0.02, -0.03, 0.01])).reshape(v9.shape)
    g.refit_triangles_device(torch.from_numpy(moved.reshape(-1, 3, 3)).to(DEV), None, lo, hi)
    torch.cuda.synchronize(DEV)
    after = g.trace_origin(sa.MODE_BVH, o, dirs)
    assert same_hits(after, g.trace(sa.MODE_BVH, starts, dirs)) and not same_hits(after, before)
    check = orc.Scene()
    check.set_triangles(moved, argb, lo, hi)
    assert check.build_tree() == 0
    model = oc.oracle_trace(check, None, "bvh", False, (), o, dirs)
    assert same_hits(after, model)
    # other geometry altogether: sr_set_triangles + sr_build
    v2, a2, lo2, hi2 = unit_cube_scene(700, seed=99)
    g.set_triangles(v2, a2, lo2, hi2)
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=True)
    for mode in MODES.values():
        assert same_hits(g.trace_origin(mode, o, dirs), g.trace(mode, starts, dirs)), mode


# ---- 6. stream ordering ----
def test_a_frame_and_the_call_on_two_streams_keep_their_order(scenes):
    sc = scenes("cube")
    g = sc.gpu(True)
    f = as_sr(gbc.frame_of(("cube", "out", 200, 160, None, 1, False), shadows=True))
    o = oc.origin_of("cube", "one")
    dirs = oc.dirs_of("cube", "one", "irregular")
    target = sa.MODE_BVH | L.TARGET_ROOT
    want_px, _ = g.render(f)
    want_px = np.asarray(want_px).view(np.uint32).ravel().copy()
    want = g.trace(target, tiled(o, dirs.shape[0]), dirs)
    A, B = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    n = dirs.shape[0]
    px = [torch.zeros(f.width * f.height, dtype=torch.int32, device=DEV) for _ in range(2)]
    d_dirs = torch.from_numpy(dirs).to(DEV)
    bufs = {k: torch.zeros(n * ITEM[k][1] * np.dtype(ITEM[k][0]).itemsize, dtype=torch.uint8, device=DEV) for k in KEYS}
    torch.cuda.synchronize(DEV)
    g.render_device(f, px[0].data_ptr(), stream=A.cuda_stream)
    g.trace_origin_device(target, o, n, d_dirs.data_ptr(), stream=B, **{"d_" + k: v.data_ptr() for k, v in bufs.items()})
    g.render_device(f, px[1].data_ptr(), stream=A.cuda_stream)
    A.synchronize(); B.synchronize()
    torch.cuda.synchronize(DEV)
    for p in px:
        assert np.array_equal(p.cpu().numpy().view(np.uint32), want_px)
    for k in KEYS:
        assert np.array_equal(bufs[k].cpu().numpy(), np.ascontiguousarray(want[k]).view(np.uint8).reshape(-1)), k
