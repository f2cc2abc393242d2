"""Path tracing on a multi-device scene (sr_create_multi): the frame is split into interleaved 16-row strips like any other, the parts
exchange the hit counts of their rows between the primary pass and the second rays, and the row blocks stay those of the whole row
range.  A multi-device scene over the same GPU several times runs the real strip bookkeeping and the real exchange on one card.
Every comparison is an exact equality over every pixel: against the reference's goldens, the CPU model (tests/pathtrace_model.py) and
the single-device scene."""
import json
import os
import zlib

import numpy as np
import pytest

import pathtrace_model as ptm
import softray_amd as sa
from helpers import GOLDEN, load_obj3ds, make_frame, orc, unit_cube_scene
from test_gpu_pathtrace import MODES, as_sr, golden_rgb, gpu_rows, path_frame

pytestmark = pytest.mark.gpu
NCPU = os.cpu_count() or 8
PARTS = (2, 3, 8)


class Trio:
    """The same scene three times: single-device, the oracle (for the CPU model), and multi-device scenes over device 0, made on demand."""

    def __init__(self, v9, argb, bmin, bmax, prims=(), modes=(sa.MODE_REF_TREE, sa.MODE_BVH)):
        self.args, self.prims, self.modes = (v9, argb, bmin, bmax), list(prims), tuple(modes)
        self.single = self._gpu(sa.GpuScene(0))
        self.oracle = orc.Scene()
        self.oracle.set_triangles(*self.args)
        if self.prims:
            self.oracle.set_extra(self.prims)
        assert self.oracle.build_tree() == 0
        self._multi = {}

    def _gpu(self, g):
        g.set_triangles(*self.args)
        if self.prims:
            g.set_extra(self.prims)
        g.build(self.modes)
        return g

    def multi(self, n):
        if n not in self._multi:
            m = sa.GpuScene(devices=[0] * n)
            assert m.device_count() == n
            self._multi[n] = self._gpu(m)
        return self._multi[n]

    def close(self):
        for m in self._multi.values():
            m.close()
        self.single.close()


@pytest.fixture(scope="module")
def obj2():
    t = Trio(*load_obj3ds("obj2.3DS"))
    yield t
    t.close()


@pytest.fixture(scope="module")
def obj():
    t = Trio(*load_obj3ds("obj.3ds"))
    yield t
    t.close()


@pytest.fixture(scope="module")
def primitives():
    t = Trio(*load_obj3ds("obj.3ds"), prims=ptm.PRIMITIVES)
    yield t
    t.close()


def strips_of(f):
    a = min(max(0, f.start_row), f.height - 1)
    b = min(max(0, f.end_row), f.height - 1)
    return b // 16 - a // 16 + 1


def check(t, f, parts=PARTS, modes=("tree", "bvh")):
    """The frame through multi-device scenes of `parts` parts: equal to the CPU model and to the single-device scene, really split."""
    want = {}
    for m in modes:
        key = "bvh" if m == "bvh" else "tree"
        if key not in want:
            want[key] = ptm.render(t.oracle, f, ptm.TRACE_NEAREST if key == "bvh" else ptm.TRACE_ROOT_TREE)
        one = gpu_rows(t.single, f, MODES[m])
        assert int(np.count_nonzero(one != want[key])) == 0, m
        for n in parts:
            g = t.multi(n)
            got = gpu_rows(g, f, MODES[m])
            assert got.shape == want[key].shape
            assert int(np.count_nonzero(got != want[key])) == 0, (m, n)
            assert g.last_frame_parts() == min(n, strips_of(f)), (m, n)
    return want


# ---- 1. the reference's goldens through a multi-device scene ----
@pytest.mark.parametrize("n", PARTS)
@pytest.mark.parametrize("name,kw", ptm.TRIANGLE_GOLDENS, ids=[x for x, _ in ptm.TRIANGLE_GOLDENS])
def test_triangle_goldens_through_a_multi_scene(obj2, name, kw, n):
    """100 rows are 7 strips, and blocks of 25 rows: every block boundary lies inside a strip."""
    g = obj2.multi(n)
    for mode in (sa.MODE_REF_TREE, sa.MODE_BVH):
        got = gpu_rows(g, path_frame(**kw), mode)
        assert g.last_frame_parts() == min(n, 7)
        assert np.all(got >> 24 == 0xFF)
        assert int(np.count_nonzero((got & 0xFFFFFF) != golden_rgb(name))) == 0, mode


@pytest.mark.parametrize("n", PARTS)
@pytest.mark.parametrize("name,kw", ptm.SPHERE_GOLDENS, ids=[x for x, _ in ptm.SPHERE_GOLDENS])
def test_sphere_goldens_through_a_multi_scene(primitives, name, kw, n):
    g = primitives.multi(n)
    got = gpu_rows(g, path_frame(**kw), sa.MODE_REF_TREE)
    assert g.last_frame_parts() == min(n, 7)
    assert np.all(got >> 24 == 0xFF)
    assert int(np.count_nonzero((got & 0xFFFFFF) != golden_rgb(name))) == 0


# ---- 2. against the CPU model and the single-device scene ----
@pytest.mark.parametrize("concurrency", [1, 3, 4, 7, 0, 500])
def test_concurrency_row_blocks(obj2, obj, concurrency):
    """67 rows are 5 strips; the blocks (67, 23, 17, 10, 17 and 1 rows) do not line up with them."""
    for t in (obj2, obj):
        for n in (1, 2):
            check(t, path_frame(90, 67, sub_pixel_res=n, concurrency=concurrency))


def test_row_windows(obj2, obj):
    for t in (obj2, obj):
        for a, b in ((10, 57), (0, 0), (33, 99), (-5, 20), (50, 1000)):
            for conc in (4, 3):
                check(t, path_frame(100, 100, start_row=a, end_row=b, concurrency=conc))


def test_most_parts_own_nothing(obj2, obj):
    """Rows 37..41 lie in one strip: one of the 8 parts renders, the others contribute no counts."""
    for t in (obj2, obj):
        check(t, path_frame(100, 100, start_row=37, end_row=41), parts=(8,))
        check(t, path_frame(100, 100, start_row=30, end_row=50, sub_pixel_res=2, concurrency=3), parts=(8,))
        assert t.multi(8).last_frame_parts() == 3


def test_shading_focal_blur_seeds_and_sub_samples(obj2, obj):
    for t in (obj2, obj):
        w = check(t, path_frame(96, 80, shading=True))
        assert np.array_equal(w["tree"], w["bvh"])
        check(t, path_frame(64, 48, shading=True, sub_pixel_res=3))
        check(t, path_frame(64, 48, shading=True, sub_pixel_res=2, focal_blur=True, point_light=False, specular=False))
    base = path_frame(80, 60)
    seeded = path_frame(80, 60)
    seeded.random_seed = 42
    a = check(obj, base)["tree"]
    b = check(obj, seeded)["tree"]
    assert not np.array_equal(a, b)
    check(obj, base)                                                            # back to the first seed: every part makes its table again


def test_non_square_frames(obj2, obj):
    for t in (obj2, obj):
        for w, h in ((160, 50), (37, 121), (1, 64), (200, 3)):
            check(t, path_frame(w, h))


def test_extra_geometry_in_tree_and_brute_mode(primitives):
    w = check(primitives, path_frame(72, 54, depth=3.0, shading=True), modes=("tree", "brute"))
    for n in PARTS:
        assert np.array_equal(gpu_rows(primitives.multi(n), path_frame(72, 54, depth=3.0, shading=True), sa.MODE_BVH), w["tree"])


def test_every_sample_misses(obj2, obj):
    for t in (obj2, obj):
        f = path_frame(64, 40, depth=-5.0)                                      # the model is behind the camera
        for n in (1, 2):
            f.sub_pixel_res = n
            for parts in PARTS:
                assert np.all(gpu_rows(t.multi(parts), f, sa.MODE_BVH) == 0xFFFF00FF)
            check(t, f)


# ---- 3. several row bands per part: the first phase only counts, the second repeats the primary pass ----
@pytest.mark.parametrize("n", (2, 3))
def test_several_bands_per_part(obj2, n):
    g, o = obj2.multi(n), obj2.oracle
    try:
        for band_samples, sub, conc in ((16 * 90, 1, 3), (16 * 90, 1, 1), (16 * 96 * 4, 2, 4), (16 * 96 * 4, 2, 7)):
            g.debug_set(sa._lib.DBG_BAND_SAMPLES, band_samples)
            for f in (path_frame(90, 67, sub_pixel_res=sub, concurrency=conc, shading=True),
                      path_frame(90, 67, sub_pixel_res=sub, concurrency=conc, start_row=9, end_row=60)):
                rows = min(f.end_row, 66) - max(f.start_row, 0) + 1
                for mode, target in ((sa.MODE_REF_TREE, ptm.TRACE_ROOT_TREE), (sa.MODE_BVH, ptm.TRACE_NEAREST)):
                    want = ptm.render(o, f, target)
                    got, st = gpu_rows(g, f, mode, stats=True)
                    assert int(np.count_nonzero(got != want)) == 0, (band_samples, sub, conc, mode)
                    # the counting pass is not counted: one camera ray per sample
                    assert st[0] == g.ray_stats()[0] == rows * 90 * sub * sub
                    assert g.last_frame_parts() == n
    finally:
        g.debug_set(sa._lib.DBG_BAND_SAMPLES, -1)


# ---- 4. a scene that runs several workgroups per kernel ----
@pytest.mark.parametrize("name", ["cube20k_640x480", "cube20k_640x480_2xAA"])
def test_cube20k_with_eight_parts(name):
    doc = json.load(open(os.path.join(GOLDEN, "pathtrace", name + ".json")))
    g = sa.GpuScene(devices=[0] * 8)
    g.set_triangles(*unit_cube_scene(doc["scene"]["triangles"]))
    g.build((sa.MODE_BVH,))
    f = path_frame(doc["width"], doc["height"], shading=True, depth=doc["frame"]["depth"], sub_pixel_res=doc["frame"].get("sub_pixel_res", 1))
    n2 = f.sub_pixel_res ** 2
    got, st = gpu_rows(g, f, sa.MODE_BVH, stats=True)
    assert g.last_frame_parts() == 8
    assert st[0] == 640 * 480 * n2
    assert len(doc["strips"]) == 30
    for s, crc in doc["strips"].items():
        s = int(s)
        assert zlib.crc32(np.ascontiguousarray(got[16 * s:16 * s + 16], dtype="<u4").tobytes()) & 0xFFFFFFFF == crc, (name, s)
    assert int(np.count_nonzero(got == 0xFFFF00FF)) == doc["background_pixels"]
    if n2 == 1:
        assert g.ray_stats()[4] == 640 * 480 - int(np.count_nonzero(got == 0xFFFF00FF))      # one second ray per camera sample that hit
    g.close()


# ---- 5. the device surface: nothing waits on the host between frames ----
@pytest.mark.parametrize("n", PARTS)
def test_device_surface_twice_in_a_row(obj2, n):
    import torch
    g = obj2.multi(n)
    f = as_sr(path_frame(150, 203, shading=True), sa.MODE_BVH)
    want, _ = obj2.single.render(f)
    dev = torch.device("cuda", 0)
    out = torch.zeros(150 * 203, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev)
    try:
        for no_peer in (-1, 1):
            g.debug_set(sa._lib.DBG_NO_PEER, no_peer)
            out.zero_()
            g.render_device(f, out.data_ptr(), st.cuda_stream)
            g.render_device(f, out.data_ptr(), st.cuda_stream)
            torch.cuda.synchronize(dev)
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want), no_peer
            assert g.last_frame_parts() == n
    finally:
        g.debug_set(sa._lib.DBG_NO_PEER, -1)


def test_two_different_frames_back_to_back_on_the_device(obj2):
    """The second frame's counts must not reach the pinned array before every part has taken the first frame's."""
    import torch
    g = obj2.multi(3)
    fa = as_sr(path_frame(150, 203, shading=True), sa.MODE_BVH)
    fb = as_sr(path_frame(150, 203, depth=1.6, yaw_deg=100.0, concurrency=7), sa.MODE_BVH)
    want_a, _ = obj2.single.render(fa)
    want_b, _ = obj2.single.render(fb)
    dev = torch.device("cuda", 0)
    outs = [torch.zeros(150 * 203, dtype=torch.int32, device=dev) for _ in range(4)]
    st = torch.cuda.current_stream(dev)
    for k, f in enumerate((fa, fb, fa, fb)):
        g.render_device(f, outs[k].data_ptr(), st.cuda_stream)
    torch.cuda.synchronize(dev)
    for k, want in enumerate((want_a, want_b, want_a, want_b)):
        assert np.array_equal(outs[k].cpu().numpy().view(np.uint32), want), k


def test_frame_kinds_alternate_on_one_multi_scene(obj):
    shadowed = make_frame(96, 72, shadows=True)
    bounce = make_frame(96, 72)
    bounce.max_bounces, bounce.reflectivity = 2, 0.5
    traced = path_frame(96, 72, shading=True)
    for n in PARTS:
        g = obj.multi(n)
        for mode in (sa.MODE_REF_TREE, sa.MODE_BVH):
            for _ in range(2):
                for f in (traced, shadowed, bounce):
                    want, _ = obj.single.render(as_sr(f, mode))
                    got, _ = g.render(as_sr(f, mode))
                    assert np.array_equal(got, want), (n, mode)
                    assert g.last_frame_parts() == min(n, 5)


def test_same_frame_three_times(obj2):
    f = path_frame(128, 96, shading=True, sub_pixel_res=2)
    for n in PARTS:
        g = obj2.multi(n)
        a = gpu_rows(g, f, sa.MODE_BVH)
        assert np.array_equal(a, gpu_rows(g, f, sa.MODE_BVH)) and np.array_equal(a, gpu_rows(g, f, sa.MODE_BVH))
        assert np.array_equal(a, gpu_rows(obj2.single, f, sa.MODE_BVH))


def test_statistics_are_the_sums_over_the_parts(obj2):
    f = path_frame(100, 100)
    one, st1 = gpu_rows(obj2.single, f, sa.MODE_REF_TREE, stats=True)
    hits = int(np.count_nonzero(one != 0xFFFF00FF))
    for n in PARTS:
        g = obj2.multi(n)
        got, st = gpu_rows(g, f, sa.MODE_REF_TREE, stats=True)
        rs = g.ray_stats()
        assert np.array_equal(got, one)
        assert np.array_equal(st, st1)                                          # the reference tree's counters do not depend on the split
        assert rs[0] == 10000 and rs[4] == hits


# ---- 6. sr_last_frame_parts ----
def test_last_frame_parts(obj):
    assert obj.single.last_frame_parts() == 1
    obj.single.render(as_sr(path_frame(64, 64), sa.MODE_BVH))
    assert obj.single.last_frame_parts() == 1
    for n in PARTS:
        g = obj.multi(n)
        g.render(as_sr(make_frame(150, 203), sa.MODE_BVH))                      # 13 strips
        assert g.last_frame_parts() == n
        g.reset_shadow_cache()
        g.render(as_sr(make_frame(96, 64, shadows=True, static_shadows=True), sa.MODE_BVH))
        assert g.last_frame_parts() == 1                                        # one global fill order: the first part renders it whole
        g.render(as_sr(make_frame(150, 203, start_row=37, end_row=41), sa.MODE_BVH))
        assert g.last_frame_parts() == 1
        g.render(as_sr(path_frame(150, 203), sa.MODE_BVH))
        assert g.last_frame_parts() == n


def test_caller_made_strips_stay_refused(obj):
    """One call on one scene cannot know the other ranks' counts -- also when the scene is a multi-device one (its first part takes the call)."""
    for g in (obj.single, obj.multi(2)):
        for mode in (sa.MODE_REF_TREE, sa.MODE_BVH):
            with pytest.raises(sa.SoftrayError) as e:
                g.render(as_sr(path_frame(32, 32, strips=(16, 2, 0)), mode))
            assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED


# ---- 7. distinct devices ----
@pytest.mark.skipif(__import__("torch").cuda.device_count() < 2, reason="needs two GPUs: the exchange of the row counts between distinct devices")
def test_path_tracing_over_distinct_gpus():
    import torch
    ndev = min(torch.cuda.device_count(), 8)
    v9, argb, bmin, bmax = unit_cube_scene(20000)
    single = sa.GpuScene(0)
    single.set_triangles(v9, argb, bmin, bmax)
    single.build((sa.MODE_BVH,))
    multi = sa.GpuScene(devices=list(range(ndev)))
    multi.set_triangles(v9, argb, bmin, bmax)
    multi.build((sa.MODE_BVH,))
    f = as_sr(path_frame(640, 515, depth=1.5, shading=True), sa.MODE_BVH)
    want, _ = single.render(f)
    assert np.array_equal(multi.render(f)[0], want)
    assert multi.last_frame_parts() == ndev
    dev = torch.device("cuda", 0)
    out = torch.zeros(640 * 515, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev)
    for no_peer in (-1, 1):
        multi.debug_set(sa._lib.DBG_NO_PEER, no_peer)
        out.zero_()
        multi.render_device(f, out.data_ptr(), st.cuda_stream)
        multi.render_device(f, out.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize(dev)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want), no_peer
    multi.close()
