"""The own BVH on adversarial geometry, on the GPU: trees as deep as the LDS traversal stacks allow (where the four-wide private walks
are switched off and the packet walks stay on, and past that a four-wide tree too deep for the packet walks as well), equal Morton keys,
exact duplicates and ties, a flat root box, and builds the library refuses.  Everything is bit for bit against the oracle, whose side
tests/test_bvh_shapes_model.py settles on the CPU."""
import numpy as np
import pytest
import torch

import bvh_shape_cases as cases
import bvh_shapes as bs
import sequence_cases as seq
import softray_amd as sa
from helpers import orc

pytestmark = pytest.mark.gpu
L = sa._lib

# the walks a frame can take: the defaults (packet walks on the four-wide tree), private primary walks, private shaft walks in every
# round, the packet walks on the binary tree
SWITCHES = ((), ((L.DBG_PER_LANE_PRIMARY, 1),), ((L.DBG_PER_LANE_SHAFT, 3),), ((L.DBG_BVH2_PACKETS, 1),))
TINY_CAPS = ((L.DBG_ROUND_CAP0, 2), (L.DBG_ROUND_CAP1, 3))              # tiny candidate lists: round 2 and the exact fallback run
OMODE = {sa.MODE_BVH: orc.MODE_NEAREST, sa.MODE_REF_TREE: orc.MODE_REF_TREE, sa.MODE_BRUTE: orc.MODE_BRUTE}
OTARGET = {sa.MODE_BVH: "nearest", sa.MODE_REF_TREE: "tree", sa.MODE_BRUTE: "brute"}


def as_sr(frame, mode, per_lane=False, flags=0):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = mode
    f.flags |= flags
    if per_lane:
        f.flags |= L.F_PER_LANE_SHADOWS
    return f


def gpu_scene(name, modes, leaf=None, on_device=None, devices=None):
    g = sa.GpuScene(devices=devices) if devices else sa.GpuScene(0)
    g.set_triangles(*cases.scene(name))
    if leaf is not None:
        g.debug_set(L.DBG_BVH_LEAF, leaf)
    g.build(modes, on_device=on_device)
    return g


def render_with(g, frame, mode, switches=(), per_lane=False, flags=0):
    for key, value in switches:
        g.debug_set(key, value)
    try:
        got, _ = g.render(as_sr(frame, mode, per_lane, flags))
    finally:
        for key, _ in switches:
            g.debug_set(key, -1)
    return got


def assert_frames(g, scene_name, frame_names, mode, switch_sets=SWITCHES, caps_on=("shadows",), label=""):
    for frame_name in frame_names:
        want = cases.oracle_frame(scene_name, frame_name, OMODE[mode])
        f = cases.frame(scene_name, frame_name, OMODE[mode])
        for switches in switch_sets:
            assert np.array_equal(render_with(g, f, mode, switches), want), (label, scene_name, frame_name, mode, switches)
        if frame_name in caps_on:
            assert np.array_equal(render_with(g, f, mode, TINY_CAPS), want), (label, scene_name, frame_name, mode, "caps")


def assert_traces(g, scene_name, family, mode, label=""):
    s, d = cases.ray_batch(scene_name, family)
    got = g.trace(mode, s, d, counters=True)
    want = cases.oracle_trace(scene_name, family, OTARGET[mode])
    for key in cases.TRACE_KEYS:
        assert np.array_equal(got[key], want[key]), (label, scene_name, family, mode, key)
    return got


def assert_code(call, code):
    with pytest.raises(sa.SoftrayError) as e:
        call()
    assert e.value.code == code


def test_deep_host_tree_private_walks_leave_the_wide_tree():
    """The shrinking chain under one triangle per leaf: the wide tree is at least 21 levels deep, so the private walks of every
    kernel run on the binary tree while the packet walks stay on the wide one; with four per leaf every walk is on the wide tree."""
    seen = {}
    for leaf in (1, 4):
        g = gpu_scene("deep", (sa.MODE_BVH,), leaf, on_device=False)
        depth, _, tris, on_device = g.bvh_stats()
        wide_depth = g.wide_tree_stats()[0]
        seen[leaf] = (depth, wide_depth)
        print("deep scene, leaf %d: depth %d, wide depth %d" % (leaf, depth, wide_depth))
        assert tris == 300 and on_device == 0 and depth <= 62
        assert (wide_depth >= 21) if leaf == 1 else (wide_depth < 21)
        assert_frames(g, "deep", cases.DEEP_FRAMES, sa.MODE_BVH, label="leaf %d" % leaf)
        f = cases.frame("deep", "shadows")                                # one lane per hit point (k_shadow), a private walk again
        assert np.array_equal(render_with(g, f, sa.MODE_BVH, per_lane=True), cases.oracle_frame("deep", "shadows"))
    assert seen[1][0] > seen[4][0]


@pytest.mark.parametrize("on_device", [False, True], ids=["host_built", "device_built"])
@pytest.mark.parametrize("leaf", [1, 4])
def test_ray_batches_reach_every_level(leaf, on_device):
    """Rays at every triangle of the chain, through the point it converges to and past it by less than the boxes' pad.  The triangles
    the rays can hit are the first 29 (cases.chain_hittable); the chain of those 29 alone is covered completely, the chain of 200
    in exactly those, and its deeper levels by the rays through the point, which visit a node on every level of a host-built tree."""
    g = gpu_scene("chain", (sa.MODE_BVH,), leaf, on_device=on_device)
    depth, nodes, _, built_on_device = g.bvh_stats()
    assert built_on_device == (1 if on_device else 0)
    v9, _, bmin, bmax = cases.scene("chain")
    if on_device:
        assert (depth, nodes) == bs.lbvh_model(v9, bmin, bmax, leaf)[:2]
    print("chain of 200, leaf %d, %s: depth %d, wide depth %d" % (leaf, "device" if on_device else "host", depth, g.wide_tree_stats()[0]))
    for family in cases.RAY_FAMILIES:
        got = assert_traces(g, "chain", family, sa.MODE_BVH)
        hit = got["hit"].astype(bool)
        if family == "at_triangles":
            assert np.array_equal(np.unique(got["tri_index"][hit]), np.arange(cases.CHAIN_HITTABLE))
        else:
            assert not hit.any()
        if family == "through_point":
            print("  nodes visited by the rays through the point: %d .. %d" % (got["counters"][:, 1].min(), got["counters"][:, 1].max()))
            if not on_device:
                assert got["counters"][:, 1].max() >= depth - 1           # one inner node per level above the leaves
    small = gpu_scene("chain_hittable", (sa.MODE_BVH,), leaf, on_device=False)        # (64 triangles or fewer are built on the host)
    for family in cases.RAY_FAMILIES:
        got = assert_traces(small, "chain_hittable", family, sa.MODE_BVH)
        if family == "at_triangles":
            assert got["hit"].all() and np.array_equal(got["tri_index"], np.repeat(np.arange(cases.CHAIN_HITTABLE), 5))


def test_device_tree_at_the_depth_limit():
    """The Morton staircase, sized with the model: depth 62 exactly, the deepest tree sr_build accepts.  The private walks ask for all
    64 KB of LDS, k_shadow for its offset table on top of them."""
    g = gpu_scene("limit", (sa.MODE_BVH,), on_device=True)
    v9, _, bmin, bmax = cases.scene("limit")
    stats = g.bvh_stats()
    assert stats[:2] == bs.lbvh_model(v9, bmin, bmax, 4)[:2] and stats[0] == 62 and stats[3] == 1
    wide = g.wide_tree_stats()
    print("staircase of %d at the limit: depth %d, wide depth %d" % (cases.limit_staircase_length(), stats[0], wide[0]))
    assert wide[0] == bs.wide_depth_model(bs.lbvh_nodes(v9, bmin, bmax, 4), fp32=True)
    assert wide[0] >= 21 and wide[4] == v9.shape[0] and wide[3] == stats[1] + 1
    assert_frames(g, "limit", ("plain", "shadows"), sa.MODE_BVH)
    f = cases.frame("limit", "shadows")
    assert np.array_equal(render_with(g, f, sa.MODE_BVH, per_lane=True), cases.oracle_frame("limit", "shadows"))
    got = assert_traces(g, "limit", "at_triangles", sa.MODE_BVH)
    assert got["hit"].any()


# ---- a four-wide tree too deep for the packet walks (wide depth >= 41), and the deepest one they take (40) ----
def wide_tree_scene(name, modes=(sa.MODE_BVH,)):
    """The cluster staircase, device-built with one triangle per leaf; depth and wide depth are the models', asserted before anything runs."""
    g = gpu_scene(name, modes, leaf=cases.WIDE_LEAF, on_device=True)
    v9, _, bmin, bmax = cases.scene(name)
    depth, nodes, tris, on_device = g.bvh_stats()
    wide_depth = g.wide_tree_stats()[0]
    print("%s, %d triangles, leaf %d: depth %d, wide depth %d" % (name, tris, cases.WIDE_LEAF, depth, wide_depth))
    assert (depth, nodes) == bs.lbvh_model(v9, bmin, bmax, cases.WIDE_LEAF)[:2] and on_device == 1 and tris == v9.shape[0] <= 400
    assert wide_depth == bs.wide_depth_model(bs.lbvh_nodes(v9, bmin, bmax, cases.WIDE_LEAF), fp32=True)
    assert depth <= 62
    assert {"wide_deep": wide_depth >= 41, "wide_edge": wide_depth == 40, "private_edge": wide_depth == 20}[name]
    return g


@pytest.fixture(scope="module")
def wide_deep():
    return wide_tree_scene("wide_deep", (sa.MODE_BVH, sa.MODE_REF_TREE))


@pytest.mark.parametrize("frame_name", cases.DEEP_FRAMES)
def test_frames_on_a_wide_tree_too_deep_for_the_packet_walks(wide_deep, frame_name):
    """Every frame under every schedule: the defaults (the binary packet walks over the partitioned records and the cone records), the
    private walks, the hook's binary packet walks (records in build order), tiny candidate lists, one lane per hit point, the one-kernel
    renderer, and a reference-tree frame whose shadow rays take the shaft path."""
    g = wide_deep
    assert_frames(g, "wide_deep", (frame_name,), sa.MODE_BVH, caps_on=(frame_name,))
    f = cases.frame("wide_deep", frame_name)
    want = cases.oracle_frame("wide_deep", frame_name)
    assert np.array_equal(render_with(g, f, sa.MODE_BVH, per_lane=True), want)
    assert np.array_equal(render_with(g, f, sa.MODE_BVH, flags=L.F_SINGLE_KERNEL), want)
    assert_frames(g, "wide_deep", (frame_name,), sa.MODE_REF_TREE, switch_sets=((),), caps_on=())
    for family in cases.RAY_FAMILIES if frame_name == "plain" else ():
        got = assert_traces(g, "wide_deep", family, sa.MODE_BVH)
        if family == "through_point":
            visited = got["counters"][:, 1]
            print("  nodes visited by the rays through the point: %d .. %d" % (visited.min(), visited.max()))
            assert visited.max() >= g.wide_tree_stats()[0]


def test_too_deep_wide_tree_walks_no_ordered_copy():
    """The default schedule of a shadowed frame: the facing partition ran for the camera and the light (both ordered copies were fitted
    to its live runs: k_tight_boxes), and neither copy was walked: sr_debug_counters [5] is 0, the binary packet walks read the moved
    records.  On the deepest tree the packet walks take, the same frame walks both copies."""
    f = cases.frame("wide_deep", "shadows")
    for name in ("wide_deep", "wide_edge"):
        g = wide_tree_scene(name)                                        # (a scene's first frame: every record is made now)
        g.reset_kernel_times()
        g.debug_set(L.DBG_KERNEL_TIMING, 1)
        try:
            got = render_with(g, f, sa.MODE_BVH)
            times = g.kernel_times()
        finally:
            g.debug_set(L.DBG_KERNEL_TIMING, -1)
        assert np.array_equal(got, cases.oracle_frame(name, "shadows"))
        print("  %s: counters %s, kernels %s" % (name, list(g.debug_counters()), sorted(times)))
        assert times["k_tight_boxes"][1] == 2, times
        if name == "wide_deep":
            assert g.debug_counters()[5] == 0
        else:
            assert g.debug_counters()[5] & 7                             # (the light of these frames is outside the box on two axes)


def test_deepest_wide_tree_the_packet_walks_take():
    """Wide depth 40: (3 x 40 + 2) x 528 B = 64 416 B of LDS for a packet walk's stack, the largest request there is."""
    g = wide_tree_scene("wide_edge", (sa.MODE_BVH, sa.MODE_REF_TREE))
    assert_frames(g, "wide_edge", ("plain", "shadows"), sa.MODE_BVH, caps_on=("shadows",))
    assert_frames(g, "wide_edge", ("shadows",), sa.MODE_REF_TREE, switch_sets=((),), caps_on=())
    f = cases.frame("wide_edge", "shadows")
    assert np.array_equal(render_with(g, f, sa.MODE_BVH, per_lane=True), cases.oracle_frame("wide_edge", "shadows"))
    for family in cases.RAY_FAMILIES:
        assert_traces(g, "wide_edge", family, sa.MODE_BVH)


@pytest.mark.parametrize("frame_name", cases.DEEP_FRAMES)
def test_deepest_wide_tree_the_private_walks_take(frame_name):
    """Wide depth 20 under one triangle per leaf: (3 x 20 + 2) x 1 KB = 63 488 B of LDS, the largest stack a four-wide private walk asks
    for; one level more and the private walks leave the wide tree.  Every frame with private primary walks, private shaft walks in
    every round, one lane per hit point and the other schedules; the ray batches walk it privately too (sr_trace_rays)."""
    g = wide_tree_scene("private_edge", (sa.MODE_BVH, sa.MODE_REF_TREE))
    assert_frames(g, "private_edge", (frame_name,), sa.MODE_BVH, caps_on=(frame_name,))
    both = ((L.DBG_PER_LANE_PRIMARY, 1), (L.DBG_PER_LANE_SHAFT, 3))
    f = cases.frame("private_edge", frame_name)
    want = cases.oracle_frame("private_edge", frame_name)
    assert np.array_equal(render_with(g, f, sa.MODE_BVH, both), want)
    assert np.array_equal(render_with(g, f, sa.MODE_BVH, both, per_lane=True), want)
    assert np.array_equal(render_with(g, f, sa.MODE_BVH, flags=L.F_SINGLE_KERNEL), want)
    assert_frames(g, "private_edge", (frame_name,), sa.MODE_REF_TREE, switch_sets=((),), caps_on=())
    for family in cases.RAY_FAMILIES if frame_name == "plain" else ():
        assert_traces(g, "private_edge", family, sa.MODE_BVH)


class WidePair(seq.Pair):
    """sequence_cases' pair of a GpuScene and an oracle scene, the own BVH built on the device with one triangle per leaf."""

    def load(self, v9, argb, lo, hi):
        self.g.debug_set(L.DBG_BVH_LEAF, cases.WIDE_LEAF)
        for s in (self.g, self.o):
            s.set_triangles(v9, argb, lo, hi)
        self.g.build(self.modes, on_device=True)
        assert self.o.build_tree() == 0
        self.geometry = (len(v9), float(np.asarray(v9).sum()), ())


@pytest.mark.parametrize("size", [seq.SMALL, seq.PERSISTENT], ids=["small", "persistent_512x384"])
@pytest.mark.parametrize("scene_name", ["wide_deep", "wide_edge"])
def test_pose_sequence_on_the_deepest_wide_trees(scene_name, size):
    """A, B with the camera moved, A again; the light into the box and out of it on one axis; the partition switched off (hook 71) and on
    again: every frame against the oracle.  At 512 x 384 with hook 831 the four-wide shaft walk is the persistent one, with its umbra
    hints: on the deepest wide tree it takes, with the largest LDS request there is.  The tree too deep for it walks no ordered copy in
    any frame, and its binary packet shaft walk has no persistent form."""
    p = WidePair(*cases.scene(scene_name), hook=size["hook"])
    too_deep = scene_name == "wide_deep"
    assert (p.g.wide_tree_stats()[0] >= 41) if too_deep else (p.g.wide_tree_stats()[0] == 40)
    A, B = (135.0, -22.0, 0.0), (100.0, 15.0, 0.0)
    launches = []
    for label, pose, light in (("A", A, seq.L_OUT), ("B", B, seq.L_OUT), ("A again", A, seq.L_OUT), ("light inside", A, seq.L_IN), ("light out on x", A, seq.L_X)):
        _, c = p.render(seq.frame(size, pose, light), sa.MODE_BVH, None, label)
        assert not (too_deep and c[5]), (label, c)
        launches.append(c[6])
    p.g.debug_set(L.DBG_KERNEL_SWITCH, 71)
    try:
        p.render(seq.frame(size, A, seq.L_X), sa.MODE_BVH, None, "hook 71")
    finally:
        p.g.debug_set(L.DBG_KERNEL_SWITCH, size["hook"] if size["hook"] else -1)
    _, c = p.render(seq.frame(size, A, seq.L_X), sa.MODE_BVH, None, "hook 71 off")
    assert not (too_deep and c[5])
    print("  %s, hook %s: persistent shaft launches per frame %s" % (scene_name, size["hook"], launches))
    if too_deep or not size["hook"]:
        assert max(launches) == 0, launches
    else:
        assert min(launches) > 0, launches                               # the persistent shaft walk ran in every frame


GROWN_BY = 2.0 ** -10                         # 64 times the boxes' pad of 2^-16 of the root extent


def _moved_within_their_boxes(v9, step=2.0 ** -23, seed=99):
    """Every vertex moved towards the middle of its triangle's box by at most `step` (less than a quarter of a Morton cell of the
    unit box), never past it: the triangles stay inside the root box, and no box centre leaves its cell by more than that.  Such a
    move stays inside the old padded boxes, so it shows the records and slabs of a refit, not its node boxes: every second triangle
    with a box half extent of 0.02 or more is therefore scaled about its box centre until that extent has GROWN_BY more, far past the
    pad.  Their old boxes no longer hold them, and a node box the level-by-level kernels left alone anywhere above them cuts hits off."""
    v = np.asarray(v9, dtype=np.float64).reshape(-1, 3, 3)
    c = 0.5 * (v.min(axis=1) + v.max(axis=1))[:, None, :]
    u = np.random.RandomState(seed).random_sample(v.shape)
    moved = v + np.clip(c - v, -step, step) * u
    half = 0.5 * (v.max(axis=1) - v.min(axis=1)).max(axis=1)
    grown = np.flatnonzero(half >= 0.02)[::2]
    moved[grown] = c[grown] + (v[grown] - c[grown]) * (1.0 + GROWN_BY / half[grown])[:, None, None]
    return np.ascontiguousarray(moved), grown


@pytest.mark.parametrize("scene_name", ["wide_deep", "limit"])
def test_refit_of_a_deep_device_tree_to_moved_vertices(scene_name):
    """sr_refit_triangles_device with vertices that did move: frames and ray batches equal those of a scene built on the moved
    vertices, and the oracle's for them."""
    leaf = cases.WIDE_LEAF if scene_name == "wide_deep" else None
    v9, argb, bmin, bmax = cases.scene(scene_name)
    moved, grown = _moved_within_their_boxes(v9)
    assert grown.size >= 10 and np.all(moved.reshape(-1, 3) >= bmin) and np.all(moved.reshape(-1, 3) <= bmax)
    outgrown = np.abs(moved[grown] - v9[grown]).max(axis=(1, 2))
    assert np.all(outgrown > 32 * 2.0 ** -16) and not np.array_equal(np.delete(moved, grown, axis=0), np.delete(v9, grown, axis=0))
    g = gpu_scene(scene_name, (sa.MODE_BVH,), leaf, on_device=True)
    stats, wide = g.bvh_stats(), g.wide_tree_stats()
    assert np.array_equal(render_with(g, cases.frame(scene_name, "shadows"), sa.MODE_BVH), cases.oracle_frame(scene_name, "shadows"))
    g.refit_triangles_device(torch.from_numpy(moved).to(torch.device("cuda", 0)), None, bmin, bmax)
    torch.cuda.synchronize()
    assert g.bvh_stats() == stats and g.wide_tree_stats() == wide
    fresh = sa.GpuScene(0)
    fresh.set_triangles(moved, argb, bmin, bmax)
    if leaf is not None:
        fresh.debug_set(L.DBG_BVH_LEAF, leaf)
    fresh.build((sa.MODE_BVH,), on_device=True)
    o = orc.Scene()
    o.set_triangles(moved, argb, bmin, bmax)
    assert o.build_tree() == 0
    for frame_name in ("plain", "shadows"):
        f = cases.frame(scene_name, frame_name)
        want, _ = o.render(f, threads=cases.NCPU)
        for switches in SWITCHES:
            got = render_with(g, f, sa.MODE_BVH, switches)
            assert np.array_equal(got, render_with(fresh, f, sa.MODE_BVH, switches)), (frame_name, switches)
            assert np.array_equal(got, want), (frame_name, switches)
    families = cases.RAY_FAMILIES
    for family in families:
        s, d = cases.ray_batch(scene_name, family)
        got, again = g.trace(sa.MODE_BVH, s, d), fresh.trace(sa.MODE_BVH, s, d)
        want = o.trace(cases.ORC_TARGET["nearest"], s, d)
        for key in cases.TRACE_KEYS:
            assert np.array_equal(got[key], again[key]) and np.array_equal(got[key], want[key]), (family, key)


def _model_scenes():
    yield "soup", (bs.soup(1000, (0.0, 0.0, 0.0), 0.9, 21), None, bs.UNIT_MIN, bs.UNIT_MAX)
    for n in (65, 300, 4097):
        yield "same_centre_%d" % n, bs.same_centre(n)
    for name in ("duplicates", "flat_thin", "flat_thick"):
        yield name, cases.scene(name)
    for m in (20, 41, bs.STAIRCASE_MAX):
        yield "staircase_%d" % m, bs.morton_staircase(m, bs.soup(**cases.LIMIT_SOUP))


def test_device_and_model_agree_on_depth_and_nodes():
    for name, (v9, argb, bmin, bmax) in _model_scenes():
        if argb is None:
            argb = bs.colours(v9.shape[0])
        for leaf in (1, 4, 7):
            depth, nodes, _ = bs.lbvh_model(v9, bmin, bmax, leaf)
            g = sa.GpuScene(0)
            g.set_triangles(v9, argb, bmin, bmax)
            g.debug_set(L.DBG_BVH_LEAF, leaf)
            if depth > 62:                                               # (the longest staircase under one triangle per leaf)
                assert_code(lambda: g.build((sa.MODE_BVH,), on_device=True), L.SR_ERR_UNSUPPORTED)
                assert_code(g.bvh_stats, L.SR_ERR_NOT_BUILT)
                continue
            g.build((sa.MODE_BVH,), on_device=True)
            stats = g.bvh_stats()
            print("%s, leaf %d: depth %d, nodes %d, wide depth %d" % (name, leaf, stats[0], stats[1], g.wide_tree_stats()[0]))
            assert stats == (depth, nodes, v9.shape[0], 1), (name, leaf)
            wide = g.wide_tree_stats()                                   # raises on a broken link
            assert wide[4] == v9.shape[0] and wide[3] == nodes + 1 and wide[2] == wide[3] + wide[1] - 1, (name, leaf)
            if name.startswith("staircase"):                             # the collapse, restated (soups and ties compare areas that are equal or nearly so)
                assert wide[0] == bs.wide_depth_model(bs.lbvh_nodes(v9, bmin, bmax, leaf), fp32=True), (name, leaf)


@pytest.mark.parametrize("on_device", [False, True], ids=["host_built", "device_built"])
@pytest.mark.parametrize("scene_name", cases.TIE_SCENES)
def test_equal_keys_and_exact_ties(scene_name, on_device):
    g = gpu_scene(scene_name, (sa.MODE_BVH, sa.MODE_REF_TREE), on_device=on_device)
    assert g.bvh_stats()[3] == (1 if on_device else 0)
    assert_frames(g, scene_name, cases.TIE_FRAMES, sa.MODE_BVH)
    assert_frames(g, scene_name, cases.TIE_FRAMES, sa.MODE_REF_TREE)      # its shadow rays take the shaft path on the own BVH
    assert_frames(g, scene_name, cases.TIE_FRAMES, sa.MODE_BRUTE, switch_sets=((),), caps_on=())
    if scene_name == "duplicates":
        groups = bs.duplicate_groups(cases.scene("duplicates")[0])
        for mode in (sa.MODE_BVH, sa.MODE_REF_TREE, sa.MODE_BRUTE):
            got = assert_traces(g, "duplicates", "at_triangles", mode)
            hit = got["hit"].astype(bool)
            assert np.count_nonzero(hit) > 500
            assert np.array_equal(groups[got["tri_index"][hit]], got["tri_index"][hit])      # the lowest index of its group of copies


def _after_the_refusal(g, scene_name):
    """No own BVH: its frames are refused, the literal paths and brute force are untouched."""
    assert_code(g.bvh_stats, L.SR_ERR_NOT_BUILT)
    assert_code(g.wide_tree_stats, L.SR_ERR_NOT_BUILT)
    f = cases.frame(scene_name, "shadows")
    assert_code(lambda: g.render(as_sr(f, sa.MODE_BVH)), L.SR_ERR_NOT_BUILT)
    s, d = cases.ray_batch("chain", "through_point")
    assert_code(lambda: g.trace(sa.MODE_BVH, s, d), L.SR_ERR_NOT_BUILT)
    for mode in (sa.MODE_REF_TREE, sa.MODE_BRUTE):
        want = cases.oracle_frame(scene_name, "shadows", OMODE[mode])
        assert np.array_equal(render_with(g, cases.frame(scene_name, "shadows", OMODE[mode]), mode), want), mode


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one_device", "two_parts"])
def test_refused_build_leaves_no_tree_host_built(devices):
    g = gpu_scene("obj", (sa.MODE_BVH, sa.MODE_REF_TREE), on_device=False, devices=devices)
    for name in ("plain", "shadows"):
        assert np.array_equal(render_with(g, cases.frame("obj", name), sa.MODE_BVH), cases.oracle_frame("obj", name))
    g.set_triangles(*cases.scene("chain_refused"))
    assert_code(lambda: g.build((sa.MODE_BVH, sa.MODE_REF_TREE), on_device=False), L.SR_ERR_UNSUPPORTED)
    _after_the_refusal(g, "chain_refused")
    g.set_triangles(*cases.scene("deep"))
    g.build((sa.MODE_BVH, sa.MODE_REF_TREE), on_device=False)
    assert g.bvh_stats()[:3] == gpu_scene("deep", (sa.MODE_BVH,), on_device=False).bvh_stats()[:3]
    assert_frames(g, "deep", ("plain", "shadows"), sa.MODE_BVH, switch_sets=((),), caps_on=())


def test_refused_build_leaves_no_tree_device_built():
    """The same triangles rebuilt with one per leaf: the device build has overwritten the accepted tree's buffers when its depth is
    refused, so nothing of the old tree may be used again."""
    v9, _, bmin, bmax = cases.scene("limit")
    assert bs.lbvh_model(v9, bmin, bmax, 4)[0] == 62 and bs.lbvh_model(v9, bmin, bmax, 1)[0] > 62
    g = gpu_scene("limit", (sa.MODE_BVH, sa.MODE_REF_TREE), on_device=True)
    assert g.bvh_stats()[0] == 62
    assert_frames(g, "limit", ("plain", "shadows"), sa.MODE_BVH, switch_sets=((),), caps_on=())   # (and the per-frame copies of the tree exist)
    g.debug_set(L.DBG_BVH_LEAF, 1)
    assert_code(lambda: g.build((sa.MODE_BVH,), on_device=True), L.SR_ERR_UNSUPPORTED)
    _after_the_refusal(g, "limit")
    g.debug_set(L.DBG_BVH_LEAF, -1)
    g.build((sa.MODE_BVH,), on_device=True)
    assert g.bvh_stats()[:2] == bs.lbvh_model(v9, bmin, bmax, 4)[:2]
    assert_frames(g, "limit", ("plain", "shadows"), sa.MODE_BVH, switch_sets=((),), caps_on=())
