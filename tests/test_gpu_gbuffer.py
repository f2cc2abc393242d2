"""The frame G-buffer (sr_render_hits) on the GPU.  Every comparison is an exact equality over every sample: the rays against the CPU model's
camera samples bit for bit, the hits against sr_trace_rays of those rays and against the oracle, the three walks against each other, the
device variant against the host variant, and the chain a caller composes on the device -- hits, ShadingMethod, ShadowMethod, resolve --
against sr_render_device of the same frame and against the reference's goldens.  Scenes, poses and shapes: tests/gbuffer_cases.py (their hit
counts are checked on the CPU in tests/test_gbuffer_model.py)."""
import os

import numpy as np
import pytest
import torch

import gbuffer_cases as gbc
import gbuffer_model as gbm
import pathtrace_model as ptm
import softray_amd as sa
from helpers import GOLDEN, read_bmp_rgb

pytestmark = pytest.mark.gpu
L = sa._lib
DEV = torch.device("cuda", 0)
MODES = {"tree": sa.MODE_REF_TREE, "brute": sa.MODE_BRUTE, "bvh": sa.MODE_BVH}
KEYS = gbm.KEYS
GUARD = 0x5A
DECORATORS = L.F_SHADING | L.F_SHADOWS | L.F_STATIC_SHADOWS | L.F_AMBIENT_OCCLUSION | L.F_AO_UNCACHED | L.F_PATH_TRACING


def as_sr(frame, mode="bvh", extra_flags=0):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = MODES[mode]
    f.flags |= extra_flags
    return f


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def same_hits(got, want, keys=KEYS):
    return all(same(got[k], np.asarray(want[k]).reshape(got[k].shape)) for k in keys)


class Scene:
    """One scene on the device (host-built and device-built own BVH) and in the oracle; the model's answers are computed once per frame."""

    def __init__(self, name):
        self.name = name
        self.tris, self.prims = gbc.scene_data(name)
        self.tree, self.brute = gbc.oracle_scenes(name)
        self.gpus, self.models = {}, {}

    def gpu(self, on_device=None):
        if on_device not in self.gpus:
            g = sa.GpuScene(0)
            g.set_triangles(*self.tris)
            if self.prims:
                g.set_extra(list(self.prims))
            g.build((sa.MODE_REF_TREE, sa.MODE_BVH), on_device=on_device)
            self.gpus[on_device] = g
        return self.gpus[on_device]

    def model(self, f, mode):
        """(starts, dirs, the oracle's hits) for the frame's camera samples in `mode`, read-only."""
        key = (bytes(f), mode)
        if key not in self.models:
            starts, dirs = ptm.camera_samples(f)
            if mode == "tree":
                res = self.tree.trace(ptm.TRACE_ROOT_TREE, starts, dirs)
            elif mode == "brute":
                res = self.brute.trace(ptm.TRACE_ROOT_TREE, starts, dirs)              # no tree: extra geometry + the triangles by brute force
            elif not self.prims:
                res = self.tree.trace(ptm.TRACE_NEAREST, starts, dirs)
            else:
                # the oracle's nearest-hit target knows no extra geometry.  Where its answer for the model alone is the tree's -- asserted for
                # these very rays -- the tree's root geometry is the own BVH's too
                alone, near = self.tree.trace(1, starts, dirs), self.tree.trace(ptm.TRACE_NEAREST, starts, dirs)
                assert same_hits({k: np.asarray(alone[k]) for k in KEYS}, near)
                res = self.tree.trace(ptm.TRACE_ROOT_TREE, starts, dirs)
            for a in (starts, dirs) + tuple(res.values()):
                a.setflags(write=False)
            self.models[key] = (starts, dirs, res)
        return self.models[key]


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Scene(name)
        return made[name]
    return get


def nondegenerate(case):
    return case[1] != "away" and case[2] * case[3] >= 256


# ---- 1. the rays are the model's, the hits are sr_trace_rays' of those rays ----
@pytest.mark.parametrize("case", gbc.CASES, ids=gbc.case_id)
def test_rays_are_the_models_and_hits_are_trace_rays(scenes, case):
    sc = scenes(case[0])
    f = gbc.frame_of(case)
    starts, dirs = ptm.camera_samples(f)
    builds = (False, True) if case[0] != "small" else (None,)              # (at most 64 triangles: the library builds on the host by itself)
    for on_device in builds:
        g = sc.gpu(on_device)
        if case[0] == "small":
            assert g.bvh_stats()[3] == 0
        for mode in MODES:
            got = g.render_hits(as_sr(f, mode), rays=True)
            assert got["hit"].shape == (sa.GpuScene.sample_count(as_sr(f)),) == (starts.shape[0],)
            assert same(got["starts"], starts) and same(got["dirs"], dirs), (mode, on_device)
            want = g.trace(L.TARGET_ROOT | MODES[mode], starts, dirs)
            assert same_hits(got, want), (mode, on_device)


# ---- 2. ... and the oracle's ----
@pytest.mark.parametrize("case", gbc.CASES, ids=gbc.case_id)
def test_hits_are_the_oracles(scenes, case):
    sc = scenes(case[0])
    f = gbc.frame_of(case)
    for mode in MODES:
        starts, dirs, want = sc.model(f, mode)
        hit = want["hit"].astype(bool)
        print("%s %s: %d of %d samples hit, %d of them extra geometry" % (gbc.case_id(case), mode, hit.sum(), hit.size, (want["tri_index"][hit] < 0).sum()))
        if nondegenerate(case):
            assert 0.1 * hit.size < int(hit.sum()) < 0.9 * hit.size
        if case[1] == "away":
            assert not hit.any()
        got = sc.gpu().render_hits(as_sr(f, mode))
        assert same_hits(got, want), mode
        miss = got["hit"] == 0
        assert np.all(got["tri_index"][miss] == -1) and not got["pos"][miss].any() and not got["normal"][miss].any()
        assert not got["ray_frac"][miss].any() and not got["color"][miss].any()
        on_extra = (got["hit"] == 1) & (got["tri_index"] < 0)
        if sc.prims:
            assert on_extra.sum() > 0                      # (their colours are the primitives' own: equal to the oracle's above)
        else:
            assert on_extra.sum() == 0


# ---- 3. the walks of the own BVH: packets on the four-wide tree, per-lane walks, packets on the binary tree ----
@pytest.mark.parametrize("case", [c for c in gbc.CASES if not c[6]], ids=gbc.case_id)
def test_schedules_agree_and_both_camera_positions_occur(scenes, case):
    sc = scenes(case[0])
    g = sc.gpu()
    f = as_sr(gbc.frame_of(case))
    base = g.render_hits(f, rays=True)
    known = (g.debug_counters()[5] >> 4) & 7
    if case[0] == "small":
        pass                                            # (whatever tree so few triangles get: both positions are shown on the larger scenes)
    elif case[1] == "out":
        assert known == 7                               # (near, far) planes on all axes
    elif case[1] == "in":
        assert known == 0                               # inside the slab on at least one axis: (lo, hi) planes everywhere
    for key in (L.DBG_PER_LANE_PRIMARY, L.DBG_BVH2_PACKETS):
        g.debug_set(key, 1)
        try:
            other = g.render_hits(f, rays=True)
        finally:
            g.debug_set(key, -1)
        assert same_hits(other, base, KEYS + ("starts", "dirs")), key


def test_three_row_bands(scenes):
    for case in [c for c in gbc.CASES if c[2:5] == (48, 40, None)]:
        sc = scenes(case[0])
        g = sc.gpu()
        for mode in MODES:
            f = as_sr(gbc.frame_of(case), mode)
            whole = g.render_hits(f, rays=True)
            g.debug_set(L.DBG_BAND_SAMPLES, 16 * 48 * case[5] * case[5])        # 16 rows per band: 16 + 16 + 8
            g.reset_kernel_times()
            g.debug_set(L.DBG_KERNEL_TIMING, 1)
            try:
                banded = g.render_hits(f, rays=True)
                launches = g.kernel_times()["k_hits"][1]
            finally:
                g.debug_set(L.DBG_BAND_SAMPLES, -1)
                g.debug_set(L.DBG_KERNEL_TIMING, -1)
            assert launches == 3
            assert same_hits(banded, whole, KEYS + ("starts", "dirs")), (gbc.case_id(case), mode)


# ---- 4. subsets of the outputs, guard words, device against host ----
NAMES = ("starts", "dirs") + KEYS
ITEM = dict(starts=(np.float64, 3), dirs=(np.float64, 3), hit=(np.uint8, 1), ray_frac=(np.float64, 1), pos=(np.float64, 3), normal=(np.float64, 3),
            color=(np.uint32, 1), tri_index=(np.int32, 1))


def run_device(g, f, wanted, stream=None, stats=False):
    """The device variant into guard-filled torch buffers: ({name: array}, all guards intact, d_stats or None)."""
    n = sa.GpuScene.sample_count(f)
    bufs, ptrs = {}, {}
    for name in NAMES:
        dt, k = ITEM[name]
        nbytes = n * k * np.dtype(dt).itemsize
        if name in wanted:
            bufs[name] = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device=DEV)
            ptrs["d_" + name] = bufs[name].data_ptr()
    d_stats = torch.full((24,), -1, dtype=torch.int64, device=DEV) if stats else None
    torch.cuda.synchronize(DEV)
    g.render_hits_device(f, stream=stream if stream is not None else 0, d_stats_ptr=d_stats.data_ptr() if stats else None, **ptrs)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize(DEV)
    out, guards_ok = {}, True
    for name, b in bufs.items():
        dt, k = ITEM[name]
        raw = b.cpu().numpy()
        guards_ok &= bool(np.all(raw[-64:] == GUARD))
        a = raw[:-64].view(dt)
        out[name] = a.reshape(-1, 3) if k == 3 else a
    return out, guards_ok, (d_stats.cpu().numpy().view(np.uint64) if stats else None)


@pytest.mark.parametrize("case", [gbc.CASES[1], gbc.CASES[3], gbc.CASES[13]], ids=gbc.case_id)
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_every_subset_of_the_outputs_and_the_guards(scenes, case, mode):
    g = scenes(case[0]).gpu()
    f = as_sr(gbc.frame_of(case), mode)
    host = g.render_hits(f, rays=True, stats=True)
    full, ok, st = run_device(g, f, NAMES, stats=True)
    assert ok and same_hits(full, host, NAMES)
    assert np.array_equal(st[:4], host["stats"]) and not st[4:].any() and st[0] == host["hit"].size
    for name in NAMES:
        one, ok, _ = run_device(g, f, (name,))
        assert ok and same(one[name], full[name]), name
    none, ok, st = run_device(g, f, (), stats=True)
    assert not none and ok and st[0] == host["hit"].size and not st[4:].any()
    L.lib().sr_render_hits(g._h, __import__("ctypes").byref(f), *([None] * 9))                # all NULL, no statistics: legal
    assert np.array_equal(g.ray_stats()[:4], st[:4]) and not g.ray_stats()[4:].any()


# ---- 5. statistics ----
@pytest.mark.parametrize("case", [gbc.CASES[0], gbc.CASES[3], gbc.CASES[13], gbc.CASES[16]], ids=gbc.case_id)
@pytest.mark.parametrize("mode", ["tree", "brute"])
def test_statistics_are_the_undecorated_frames(scenes, case, mode):
    g = scenes(case[0]).gpu()
    plain = as_sr(gbc.frame_of(case, shading=False), mode)
    plain.flags &= ~DECORATORS
    _, want = g.render(plain)
    decorated = as_sr(gbc.frame_of(case, shadows=True), mode, L.F_AMBIENT_OCCLUSION)
    got = g.render_hits(decorated, stats=True)["stats"]
    assert np.array_equal(got, want) and got[0] == sa.GpuScene.sample_count(plain) and got[1] > 0
    full = g.ray_stats()
    assert np.array_equal(full[:4], want) and not full[4:].any()


# ---- 6. the chain on the device ----
def device_chain(g, f):
    """hits -> ShadingMethod -> ShadowMethod -> resolve on the null stream, which is torch's too, with nothing read back in between (torch's
    nonzero waits for the hit count by itself): uint32 [rows, width]."""
    n = sa.GpuScene.sample_count(f)
    nn = f.sub_pixel_res * f.sub_pixel_res
    d_hit = torch.empty(n, dtype=torch.uint8, device=DEV)
    d_pos = torch.empty((n, 3), dtype=torch.float64, device=DEV)
    d_nrm = torch.empty((n, 3), dtype=torch.float64, device=DEV)
    d_col = torch.empty(n, dtype=torch.int32, device=DEV)
    g.render_hits_device(f, d_hit=d_hit.data_ptr(), d_pos=d_pos.data_ptr(), d_normal=d_nrm.data_ptr(), d_color=d_col.data_ptr())
    idx = torch.nonzero(d_hit, as_tuple=False).reshape(-1)
    k = int(idx.numel())
    hp, hn, hc = d_pos[idx].contiguous(), d_nrm[idx].contiguous(), d_col[idx].contiguous()
    bg = (f.background_argb | 0xFF000000) & 0xFFFFFFFF
    samples = torch.full((n,), bg - (1 << 32) if bg >= (1 << 31) else bg, dtype=torch.int32, device=DEV)
    if k:
        if f.flags & L.F_SHADING:
            g.shade_points_device(f, k, hp.data_ptr(), hn.data_ptr(), hc.data_ptr(), hc.data_ptr())
        if f.flags & L.F_SHADOWS:
            g.shadow_points_device(f, k, hp.data_ptr(), hn.data_ptr(), hc.data_ptr(), hc.data_ptr())
        samples[idx] = hc
    if nn == 1:
        out = samples
    else:
        c = samples.reshape(-1, nn).to(torch.int64) & 0xFFFFFFFF
        r, gr, b = ((c >> 16) & 255).sum(1) // nn, ((c >> 8) & 255).sum(1) // nn, (c & 255).sum(1) // nn
        out = (0xFF000000 | (r << 16) | (gr << 8) | b).to(torch.int32)
    torch.cuda.synchronize(DEV)
    return out.cpu().numpy().view(np.uint32).reshape(-1, f.width)


def render_device(g, f, stream=None):
    rows = sa.GpuScene.sample_count(f) // (f.width * f.sub_pixel_res ** 2)
    a = min(max(0, f.start_row), f.height - 1)
    d_px = torch.zeros(f.width * f.height, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize(DEV)
    g.render_device(f, d_px.data_ptr(), stream=getattr(stream, "cuda_stream", 0) if stream is not None else 0)
    torch.cuda.synchronize(DEV)
    return d_px.cpu().numpy().view(np.uint32).reshape(f.height, f.width)[a:a + rows]


CHAIN_CASES = [gbc.CASES[0], ("obj", "out", 100, 100, None, 2, True), gbc.CASES[1], gbc.CASES[3], gbc.CASES[12], ("cube", "out", 37, 21, None, 2, True)]


@pytest.mark.parametrize("case", CHAIN_CASES, ids=gbc.case_id)
@pytest.mark.parametrize("mode", ["bvh", "tree"])
@pytest.mark.parametrize("shadows", [False, True], ids=["shading", "shading+shadows"])
def test_chain_on_the_device_is_the_rendered_frame(scenes, case, mode, shadows):
    g = scenes(case[0]).gpu()
    f = as_sr(gbc.frame_of(case, shadows=shadows), mode)                  # shadow_samples 0: the reference's 100
    got = device_chain(g, f)
    want = render_device(g, f)
    assert got.shape == want.shape and int(np.count_nonzero(got != want)) == 0


GOLDENS = [("shading", dict()), ("shading_4xAA", dict(sub_pixel_res=4)), ("shading_focalBlurx2", dict(focal_blur=True, sub_pixel_res=2)),
           ("shading_shadows", dict(shadows=True))]


@pytest.mark.parametrize("name,kw", GOLDENS, ids=[n for n, _ in GOLDENS])
@pytest.mark.parametrize("mode", ["bvh", "tree"])
def test_chain_on_the_device_is_the_golden_frame(scenes, name, kw, mode):
    g = scenes("obj").gpu()
    f = as_sr(gbc.frame_of(("obj", "out", 100, 100, None, 1, False), **kw), mode)
    got = device_chain(g, f)
    want = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))
    assert got.shape == want.shape and int(np.count_nonzero((got & 0xFFFFFF) != want)) == 0
    assert int(np.count_nonzero(got != render_device(g, f))) == 0


# ---- 7. ordering, and the decorator switches that are not read ----
def test_frames_and_hits_on_two_streams_keep_their_order(scenes):
    g = scenes("obj").gpu()
    fa = as_sr(gbc.frame_of(gbc.CASES[0], shadows=True))
    fh = as_sr(gbc.frame_of(gbc.CASES[2]))                                  # another camera: the per-camera records are re-made in between
    fb = as_sr(gbc.frame_of(gbc.CASES[0], shadows=True, yaw_deg=100.0))
    one_by_one = (render_device(g, fa), run_device(g, fh, NAMES)[0], render_device(g, fb))
    A, B = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    n = sa.GpuScene.sample_count(fh)
    px = [torch.zeros(fa.width * fa.height, dtype=torch.int32, device=DEV) for _ in range(2)]
    bufs = {name: torch.zeros(n * ITEM[name][1] * np.dtype(ITEM[name][0]).itemsize, dtype=torch.uint8, device=DEV) for name in NAMES}
    torch.cuda.synchronize(DEV)
    g.render_device(fa, px[0].data_ptr(), stream=A.cuda_stream)
    g.render_hits_device(fh, stream=B, **{"d_" + k: v.data_ptr() for k, v in bufs.items()})
    g.render_device(fb, px[1].data_ptr(), stream=A.cuda_stream)
    A.synchronize(); B.synchronize()
    torch.cuda.synchronize(DEV)
    assert np.array_equal(px[0].cpu().numpy().view(np.uint32).reshape(100, 100), one_by_one[0])
    assert np.array_equal(px[1].cpu().numpy().view(np.uint32).reshape(100, 100), one_by_one[2])
    for name in NAMES:
        assert np.array_equal(bufs[name].cpu().numpy(), np.ascontiguousarray(one_by_one[1][name]).view(np.uint8).reshape(-1)), name


@pytest.mark.parametrize("mode", ["bvh", "tree"])
def test_decorator_switches_change_nothing(scenes, mode):
    g = scenes("cube").gpu()
    case = gbc.CASES[13]
    base = g.render_hits(as_sr(gbc.frame_of(case, shading=False), mode), rays=True)
    variants = [as_sr(gbc.frame_of(case, shadows=True), mode), as_sr(gbc.frame_of(case, shadows=True, static_shadows=True), mode),
                as_sr(gbc.frame_of(case), mode, L.F_AMBIENT_OCCLUSION | L.F_AO_UNCACHED), as_sr(gbc.frame_of(case), mode, L.F_PATH_TRACING),
                as_sr(gbc.frame_of(case, point_light=False, specular=False), mode, L.F_NO_SPLIT | L.F_PRIMARY_STATS_ONLY)]
    bounced = as_sr(gbc.frame_of(case, shadows=True), mode, L.F_AMBIENT_OCCLUSION)
    bounced.max_bounces = 2
    bounced.reflectivity = 0.5
    variants.append(bounced)
    for f in variants:
        assert same_hits(g.render_hits(f, rays=True), base, NAMES), hex(f.flags)
