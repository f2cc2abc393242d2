"""The own BVH on adversarial geometry, on the GPU: trees as deep as the LDS traversal stacks allow (where the four-wide private walks
are switched off and the packet walks stay on), equal Morton keys, exact duplicates and ties, a flat root box, and builds the library
refuses.  Everything is bit for bit against the oracle, whose side tests/test_bvh_shapes_model.py settles on the CPU."""
import numpy as np
import pytest

import bvh_shape_cases as cases
import bvh_shapes as bs
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


def as_sr(frame, mode, per_lane=False):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = mode
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


def render_with(g, frame, mode, switches=(), per_lane=False):
    for key, value in switches:
        g.debug_set(key, value)
    try:
        got, _ = g.render(as_sr(frame, mode, per_lane))
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
    assert wide[0] >= 21 and wide[4] == v9.shape[0] and wide[3] == stats[1] + 1
    assert_frames(g, "limit", ("plain", "shadows"), sa.MODE_BVH)
    f = cases.frame("limit", "shadows")
    assert np.array_equal(render_with(g, f, sa.MODE_BVH, per_lane=True), cases.oracle_frame("limit", "shadows"))
    got = assert_traces(g, "limit", "at_triangles", sa.MODE_BVH)
    assert got["hit"].any()


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
