"""sr_bake_light_field on the device against the CPU model's whole tables (tests/lightfield_bake.py) and the reference's goldens -- bit for bit:
every comparison is an exact equality.  The figures of the model's tables are pinned without a GPU by tests/test_lightfield_bake_model.py."""
import os
import subprocess

import numpy as np
import pytest

import lightfield_bake as lfb
import lightfield_model as lfm
import softray_amd as sa
from helpers import GOLDEN, ROOT, load_obj3ds, read_bmp_rgb, unit_cube_scene

pytestmark = pytest.mark.gpu
MODES = {"tree": sa.MODE_REF_TREE, "brute": sa.MODE_BRUTE, "bvh": sa.MODE_BVH}
UNTOUCHED = 0x01020304
PACKET = 35                                  # SR_DBG_KERNEL_SWITCH: the SR_MODE_BVH bake with one packet walk per wave instead of private per-lane walks


def target_of(mode):
    return lfm.TRACE_NEAREST if mode == "bvh" else lfm.TRACE_ROOT_TREE


def as_sr(frame, mode):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = MODES[mode]
    return f


def gpu_scene(model, prims=(), modes=(sa.MODE_REF_TREE, sa.MODE_BVH), on_device=None, devices=None):
    g = sa.GpuScene(devices=devices) if devices else sa.GpuScene(0)
    g.set_triangles(*(unit_cube_scene(2000) if model == "unit_cube_2000" else load_obj3ds(model)))
    if prims:
        g.set_extra(list(prims))
    g.build(tuple(modes), on_device=on_device)
    return g


@pytest.fixture(scope="module")
def obj_gpu():
    """obj.3ds with the reference tree and the device-built BVH."""
    g = gpu_scene("obj.3ds")
    assert g.bvh_stats()[3] == 1
    return g


@pytest.fixture(scope="module")
def obj_gpu_host_bvh():
    g = gpu_scene("obj.3ds", modes=(sa.MODE_BVH,), on_device=False)
    assert g.bvh_stats()[3] == 0
    return g


@pytest.fixture(scope="module")
def tables():
    """The model's whole tables, each computed once: (model, extra geometry?, N, shading, target) -> uint32 [4 N^4], read-only."""
    scenes, made = {}, {}

    def get(model, n, shading, target, prims=()):
        key = (model, bool(prims), n, shading, target)
        if key not in made:
            if key[:2] not in scenes:
                scenes[key[:2]] = lfb.oracle_scene(model, prims)
            t = lfb.model_table(scenes[key[:2]], lfb.bake_frame(shading), n, target)
            t.setflags(write=False)
            made[key] = t
        return made[key]
    get.scene = lambda model, prims=(): scenes.setdefault((model, bool(prims)), lfb.oracle_scene(model, prims))
    return get


def fresh(g, n):
    """The scene as a new Renderer with resolution n has it."""
    g.light_field_res = n
    g.reset_light_field()


def bake(g, frame, mode, first=0, count=None):
    """(entries written, the eight ray statistics) of one bake."""
    filled = g.bake_light_field(as_sr(frame, mode), first, count)
    return filled, [int(x) for x in g.ray_stats()[:8]]


# ---- 1. the whole table against the model: clipped tiles (N = 2, 4, 12), zero-length directions, both pole rows, the NaN rays of N = 1 ----
@pytest.mark.parametrize("shading", [False, True], ids=["noShading", "shading"])
@pytest.mark.parametrize("mode", ["tree", "brute", "bvh_host", "bvh_device"])
@pytest.mark.parametrize("n", [1, 2, 4, 8, 12])
def test_whole_table(obj_gpu, obj_gpu_host_bvh, tables, n, mode, shading):
    g = obj_gpu_host_bvh if mode == "bvh_host" else obj_gpu
    mode = "bvh" if mode.startswith("bvh") else mode
    fresh(g, n)
    total = lfm.cache_entries(n)
    filled, rs = bake(g, lfb.bake_frame(shading), mode)
    assert filled == total
    assert rs[:4] == [0, 0, 0, 0] and rs[4] == (0 if n == 1 else total)
    want = tables("obj.3ds", n, shading, target_of(mode))
    got = g.get_light_field()
    assert got.size == total and int(np.count_nonzero(got != want)) == 0
    if n == 1:
        assert got.tolist() == [lfb.BACKGROUND] * 4 and rs[5:8] == [0, 0, 0]
    else:
        assert int(np.count_nonzero(got != lfb.BACKGROUND)) == lfb.NON_BACKGROUND[("obj.3ds", n)][0]


# ---- 2. a scene whose walks are long: 2000 triangles, the device-built BVH; the per-lane walk (default) and the packet walk in its place ----
@pytest.mark.parametrize("n", [8, 16])
def test_per_lane_walk_and_packet_walk(tables, n):
    g = gpu_scene("unit_cube_2000", modes=(sa.MODE_BVH,), on_device=True)
    assert g.bvh_stats()[3] == 1
    total = lfm.cache_entries(n)
    want = tables("unit_cube_2000", n, True, lfm.TRACE_NEAREST)
    assert int(np.count_nonzero(want != lfb.BACKGROUND)) == lfb.NON_BACKGROUND[("unit_cube_2000", n)][0]
    fresh(g, n)
    filled, lanes = bake(g, lfb.bake_frame(True), "bvh")
    assert filled == total == lanes[4]
    got = g.get_light_field()
    assert int(np.count_nonzero(got != want)) == 0
    try:
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, PACKET)
        g.reset_light_field()
        filled, packet = bake(g, lfb.bake_frame(True), "bvh")
    finally:
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
    assert filled == total == packet[4]
    assert np.array_equal(g.get_light_field(), got)
    # the switch selects another walk: a wave fetches a node once for its 64 rays, private walks count it once per ray
    assert 0 < packet[6] < lanes[6]


@pytest.mark.parametrize("n", [1, 2, 4, 12])
def test_packet_walk_on_clipped_tiles(obj_gpu, tables, n):
    """The packet walk needs all 64 lanes of a wave, also where a tile hangs over the 2N x N targets, a range cuts it, or the rays are NaN."""
    g = obj_gpu
    total = lfm.cache_entries(n)
    first, last = (0, total) if n == 1 else (3, total - 2)
    fresh(g, n)
    try:
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, PACKET)
        filled, rs = bake(g, lfb.bake_frame(True), "bvh", first, last - first)
    finally:
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
    assert filled == last - first and rs[4] == (0 if n == 1 else filled)
    want = tables("obj.3ds", n, True, lfm.TRACE_NEAREST).copy()
    want[:first] = 0
    want[last:] = 0
    assert np.array_equal(g.get_light_field(), want)


# ---- 3. extra geometry: the canonical rays see it, first and with strict < ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_extra_geometry(tables, mode):
    """(the oracle's nearest-hit target has no extra geometry: both modes against TRACE_ROOT_TREE, as the frames of test_gpu_lightfield.py;
    tests/test_lightfield_bake_model.py checks that the two targets agree on every cell of this model at this resolution)"""
    n = 8
    g = gpu_scene("obj.3ds", prims=lfm.ptm.PRIMITIVES)
    fresh(g, n)
    filled, rs = bake(g, lfb.bake_frame(True), mode)
    assert filled == lfm.cache_entries(n) == rs[4]
    want = tables("obj.3ds", n, True, lfm.TRACE_ROOT_TREE, prims=lfm.ptm.PRIMITIVES)
    got = g.get_light_field()
    assert int(np.count_nonzero(got != want)) == 0
    assert int(np.count_nonzero(got != tables("obj.3ds", n, True, lfm.TRACE_ROOT_TREE))) > 1000       # the spheres and the plane are in it


# ---- 4. ranges whose borders are multiples neither of 64 nor of 2 N^2 ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_ranges(obj_gpu, tables, mode):
    g, n = obj_gpu, 8
    total = lfm.cache_entries(n)
    want = tables("obj.3ds", n, True, target_of(mode))
    fresh(g, n)
    borders = [0, 5001, 11000, total]
    assert all(b % 64 and b % (2 * n * n) for b in borders[1:-1])
    done = np.zeros(total, dtype=bool)
    written = 0
    for first, last in ((5001, 11000), (0, 5001), (11000, total)):                # (out of order: a chunk touches nothing before or behind it)
        filled, rs = bake(g, lfb.bake_frame(True), mode, first, last - first)
        assert filled == last - first == rs[4]
        written += filled
        done[first:last] = True
        got = g.get_light_field()
        assert not got[~done].any() and np.array_equal(got[done], want[done])
    assert written == total and np.array_equal(g.get_light_field(), want)
    assert bake(g, lfb.bake_frame(True), mode, 123, 0)[0] == 0                    # count == 0


# ---- 5. entries that are there already survive ----
@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_existing_entries_survive(obj_gpu, tables, mode):
    g, n = obj_gpu, 8
    total = lfm.cache_entries(n)
    want = tables("obj.3ds", n, True, target_of(mode)).copy()
    fresh(g, n)
    where = (np.arange(1000, dtype=np.int64) * 16381 + 7) % total                 # scattered; 16381 is prime, so no two coincide
    assert np.unique(where).size == 1000
    mine = (np.arange(1000, dtype=np.uint32) + np.uint32(0x00010001))            # alpha 0: nothing a traced or a background colour can be
    table = np.zeros(total, dtype=np.uint32)
    table[where] = mine
    g.set_light_field(table)
    filled, rs = bake(g, lfb.bake_frame(True), mode)
    assert filled == total - 1000 == rs[4]
    want[where] = mine
    assert np.array_equal(g.get_light_field(), want)
    filled, rs = bake(g, lfb.bake_frame(True), mode)                             # nothing left
    assert filled == 0 and rs == [0] * 8
    assert np.array_equal(g.get_light_field(), want)


# ---- 6. large offsets ----
def test_range_high_in_the_largest_table(obj_gpu, tables):
    """N = 128: 4 GiB, entries beyond 2^29 (byte offsets beyond 2^31)."""
    g, n = obj_gpu, 128
    first, count = 2 ** 29 + 12345, 50000
    f = lfb.bake_frame(True)
    try:
        fresh(g, n)
        filled, rs = bake(g, f, "bvh", first, count)
        assert filled == count == rs[4]
        want = lfb.model_entries(tables.scene("obj.3ds"), f, n, np.arange(first, first + count), lfm.TRACE_NEAREST)
        assert np.array_equal(g.get_light_field(first, count), want)
        assert int(np.count_nonzero(want != lfb.BACKGROUND)) > 100
        assert not g.get_light_field(first - 4096, 4096).any() and not g.get_light_field(first + count, 4096).any()
    finally:
        g.light_field_res = 64                                                   # (drops the 4 GiB)


def test_range_of_a_million_entries(obj_gpu, tables):
    g, n = obj_gpu, 64
    first, count = 2 ** 25 + 777, 2 ** 20
    f = lfb.bake_frame(True)
    fresh(g, n)
    filled, rs = bake(g, f, "tree", first, count)
    assert filled == count == rs[4]
    got = g.get_light_field(first - 64, count + 128)
    assert not got[:64].any() and not got[-64:].any() and np.all(got[64:-64] != 0)
    sample = first + np.arange(20000, dtype=np.int64) * 52 + 3
    assert int(sample.max()) < first + count
    want = lfb.model_entries(tables.scene("obj.3ds"), f, n, sample, lfm.TRACE_ROOT_TREE)
    assert np.array_equal(got[64:-64][sample - first], want)
    assert int(np.count_nonzero(want != lfb.BACKGROUND)) > 100
    g.reset_light_field()


# ---- 7. frames after a bake are pure look-ups ----
def gpu_rows(g, frame, mode):
    f = as_sr(frame, mode)
    out = np.full(f.width * f.height, UNTOUCHED, dtype=np.uint32)
    _, stats = g.render(f, out=out, stats=True)
    return out.reshape(f.height, f.width), stats


@pytest.mark.parametrize("mode", ["tree", "bvh"])
def test_frames_after_a_bake_trace_nothing(obj_gpu, tables, mode):
    g, n = obj_gpu, 8
    baking = lfb.bake_frame(True, yaw_deg=30.0, pitch_deg=10.0)                  # (a shaded cell carries the pose of the frame that filled it)
    o = tables.scene("obj.3ds")
    model = lfm.LightFieldModel(n)
    model.fill(o, baking, np.arange(lfm.cache_entries(n), dtype=np.int64), target_of(mode))
    fresh(g, n)
    assert bake(g, baking, mode)[0] == lfm.cache_entries(n)
    table = g.get_light_field()
    for name in ("view0_n8", "view1_n8", "view2_n8"):
        _, _, fn, f = lfm.gpu_frame(name)
        assert fn == n
        want = model.render(o, f, target_of(mode))
        assert model.filled.size == 0 and model.coord_margin > lfm.MARGIN and model.term_margin > lfm.MARGIN
        got, stats = gpu_rows(g, f, mode)
        assert got.shape == want.shape and int(np.count_nonzero(got != want)) == 0
        assert [int(x) for x in stats] == [want.size * f.sub_pixel_res ** 2, 0, 0, 0]
        assert not g.ray_stats()[4:8].any()
    assert np.array_equal(g.get_light_field(), table)


# ---- 8. the reference's goldens from a baked table: 4 x 64^4 canonical rays per bake ----
@pytest.mark.parametrize("shade", ["noShading", "shading"])
def test_goldens_from_a_baked_table(obj_gpu, shade):
    g, n = obj_gpu, 64
    names = [name for name, _ in lfm.GOLDENS if name.startswith(shade + "_")]
    assert len(names) == 4
    fresh(g, n)
    total = lfm.cache_entries(n)
    filled, rs = bake(g, lfm.gpu_frame(names[0])[3], "bvh")
    assert filled == total == rs[4]
    for name in names:
        _, _, fn, f = lfm.gpu_frame(name)
        assert fn == n
        got, _ = gpu_rows(g, f, "bvh")
        want = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))
        assert int(np.count_nonzero((got & 0xFFFFFF) != want)) == 0
        assert not g.ray_stats()[4:8].any()                                      # no cell was filled
    g.reset_light_field()


def test_cpp_mirror_bakes_and_reproduces_the_goldens(tmp_path):
    exe = str(tmp_path / "lightfield_bake_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "lightfield_bake_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL OK" in r.stdout
    for line in ("noShading_lightFieldColor", "shading_lightFieldColor_4xAA", "second bake fills 0 ok"):
        assert line in r.stdout


# ---- 9. a multi-device scene bakes on its first part ----
def test_multi_device_scene(obj_gpu, tables):
    n = 8
    gm = gpu_scene("obj.3ds", devices=[0, 0])
    gm.light_field_res = n
    filled = gm.bake_light_field(as_sr(lfb.bake_frame(True), "bvh"))
    assert filled == lfm.cache_entries(n) == int(gm.ray_stats()[4]) and not gm.ray_stats()[:4].any()
    fresh(obj_gpu, n)
    bake(obj_gpu, lfb.bake_frame(True), "bvh")
    got = gm.get_light_field()
    assert np.array_equal(got, obj_gpu.get_light_field()) and np.array_equal(got, tables("obj.3ds", n, True, lfm.TRACE_NEAREST))


# ---- 10. refusals leave the table untouched ----
def test_refusals_leave_the_table_untouched(obj_gpu, tables):
    g, n = obj_gpu, 8
    total = lfm.cache_entries(n)
    fresh(g, n)
    good = lfb.bake_frame(True)
    assert bake(g, good, "tree", 0, 6000)[0] == 6000
    before = g.get_light_field()
    assert not before[6000:].any()

    def refused(frame, code, text, first=0, count=None):
        with pytest.raises(sa.SoftrayError) as e:
            g.bake_light_field(frame, first, count)
        assert e.value.code == code and text in str(e.value)
        assert np.array_equal(g.get_light_field(), before)

    for change in lfm.REFUSED:
        refused(lfm.apply_change(as_sr(good, "tree"), change), sa._lib.SR_ERR_UNSUPPORTED, "light field")
    plain = as_sr(good, "tree")
    plain.flags &= ~lfm.F_LIGHT_FIELD
    refused(plain, sa._lib.SR_ERR_INVALID_ARG, "SR_F_LIGHT_FIELD")
    refused(as_sr(good, "tree"), sa._lib.SR_ERR_INVALID_ARG, "the range exceeds the 4 N^4 entries", 1, total)
    assert bake(g, good, "tree")[0] == total - 6000                              # and the scene still bakes
    assert np.array_equal(g.get_light_field(), tables("obj.3ds", n, True, lfm.TRACE_ROOT_TREE))


# ---- 11. statistics and the kernel-name list ----
def test_statistics_and_kernel_times(obj_gpu):
    g, n = obj_gpu, 8
    total = lfm.cache_entries(n)
    for mode in ("tree", "brute", "bvh"):
        fresh(g, n)
        filled, rs = bake(g, lfb.bake_frame(True), mode)
        assert filled == total and rs[:5] == [0, 0, 0, 0, total] and rs[5] > 0
        if mode != "brute":
            assert rs[6] > 0 and rs[7] > 0
        table = g.get_light_field()
        g.reset_light_field()
        quiet = as_sr(lfb.bake_frame(True), mode)
        quiet.flags |= sa._lib.F_PRIMARY_STATS_ONLY
        assert g.bake_light_field(quiet) == total
        assert [int(x) for x in g.ray_stats()[:8]] == [0, 0, 0, 0, total, 0, 0, 0]
        assert np.array_equal(g.get_light_field(), table)
    try:
        g.debug_set(sa._lib.DBG_KERNEL_TIMING, 1)
        g.reset_kernel_times()
        g.reset_light_field()
        bake(g, lfb.bake_frame(True), "bvh")
        times = g.kernel_times()
    finally:
        g.debug_set(sa._lib.DBG_KERNEL_TIMING, -1)
    assert times["k_lf_bake"][1] == 1 and times["k_lf_bake"][0] > 0.0
    assert not any(k in times for k in ("k_lf_lookup", "k_lf_fill", "k_lf_apply"))
