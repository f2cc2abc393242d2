"""Adversarial geometry for the own BVH, CPU side: the model of the device build on trees that can be written down, the generators'
promises, the host builder (through a host-only scene) on the deep and the tied scenes -- with the refused build that must leave no
tree behind, and with its restatement and that of the four-wide collapse pinned to sr_bvh_stats and sr_wide_tree_stats -- and the
oracle's agreement with itself on every scene, frame and ray batch tests/test_gpu_bvh_shapes.py compares the library with."""
import math

import numpy as np
import pytest

import bvh_shape_cases as cases
import bvh_shapes as bs
import softray_amd as sa
from helpers import orc

L = sa._lib


def _tiny_triangles_at_x_cells(cells):
    """One tiny triangle per entry, its box centre in x cell `c` (of 2^21 - 1) and in cell 0 of y and z: key = the bits of c on every third bit."""
    v = []
    for c in cells:
        x = -0.5 + (c + 0.5) / bs.MORTON_CELLS
        y = z = -0.5 + 0.5 / bs.MORTON_CELLS
        r = 1e-8
        v.append([[x - r, y - r, z - r], [x + r, y - r, z + r], [x, y + r, z - r]])
    return np.array(v), bs.UNIT_MIN, bs.UNIT_MAX


def test_model_on_trees_that_can_be_written_down():
    top = 1 << 18                                                        # x cells 0 .. 7 << 18: the three highest x bits = key bits 62, 59, 56
    # eight distinct three-bit prefixes, given out of order: the perfectly balanced tree
    perm = [5, 0, 7, 2, 1, 6, 3, 4]
    v9, bmin, bmax = _tiny_triangles_at_x_cells([p * top for p in perm])
    keys = bs.morton_keys(v9, bmin, bmax)
    assert [int(k) for k in keys] == [((p >> 2) & 1) << 62 | ((p >> 1) & 1) << 59 | (p & 1) << 56 for p in perm]
    for leaf, want in ((1, (4, 7)), (2, (3, 3)), (3, (3, 3)), (4, (2, 1)), (7, (2, 1))):
        depth, nodes, order = bs.lbvh_model(v9, bmin, bmax, leaf)
        assert (depth, nodes) == want, leaf
        assert [perm[i] for i in order] == list(range(8))
    # prefixes 000, 001, 010, 100: {0, 1, 2} | {4}, then {0, 1} | {2}, then {0} | {1}
    v9, bmin, bmax = _tiny_triangles_at_x_cells([0, top, 2 * top, 4 * top])
    assert bs.lbvh_model(v9, bmin, bmax, 1)[:2] == (4, 3)
    assert bs.lbvh_model(v9, bmin, bmax, 2)[:2] == (3, 2)
    assert bs.lbvh_model(v9, bmin, bmax, 3)[:2] == (2, 1)
    # equal keys keep their input order (stable sort) and split by position: 0 .. 3 | 4 for five of them
    v9, bmin, bmax = _tiny_triangles_at_x_cells([3 * top] * 5 + [0])
    depth, nodes, order = bs.lbvh_model(v9, bmin, bmax, 1)
    assert list(order) == [5, 0, 1, 2, 3, 4]
    assert (depth, nodes) == (5, 5)                                      # {0} | {1 .. 5}; the equal keys by their positions: {1, 2, 3} | {4, 5}, {1} | {2, 3}


@pytest.mark.parametrize("n,leaf1,leaf4", [(5, (4, 4), (2, 1)), (64, (7, 63), (5, 15)), (65, (8, 64), (6, 16))])
def test_model_on_equal_keys_is_the_balanced_position_tree(n, leaf1, leaf4):
    v9, _, bmin, bmax = bs.same_centre(n)
    assert len(set(bs.morton_keys(v9, bmin, bmax).tolist())) == 1
    for leaf, want in ((1, leaf1), (4, leaf4)):
        depth, nodes, order = bs.lbvh_model(v9, bmin, bmax, leaf)
        assert (depth, nodes) == want
        assert depth == bs.balanced_position_depth(n, leaf)
        assert np.array_equal(order, np.arange(n))
    assert bs.lbvh_model(v9, bmin, bmax, 1)[0] == math.ceil(math.log2(n)) + 1


def test_model_on_the_staircase_grows_by_one_per_triangle():
    for leaf in (1, 4, 7):
        for m in range(leaf + 1, bs.STAIRCASE_MAX + 1, 5):
            v9, _, bmin, bmax = bs.morton_staircase(m)
            depth, nodes, order = bs.lbvh_model(v9, bmin, bmax, leaf)
            assert (depth, nodes) == (m - leaf + 1, m - leaf), (m, leaf)      # one kept node per step until the leaf absorbs the tail
            assert np.array_equal(order, np.arange(m))
    m = cases.limit_staircase_length()
    v9, _, bmin, bmax = cases.scene("limit")
    assert v9.shape[0] > 64                                              # the device build takes it
    assert bs.lbvh_model(v9, bmin, bmax, 4)[0] == 62 and bs.lbvh_model(v9, bmin, bmax, 1)[0] > 62, m


def test_generators_keep_their_promises():
    def inside(v9, bmin, bmax):
        v = v9.reshape(-1, 3)
        return bool(np.all(v >= bmin) and np.all(v <= bmax))
    for name in ("deep", "chain", "chain_hittable", "chain_refused", "limit", "wide_deep", "wide_edge", "private_edge") + cases.TIE_SCENES:
        v9, argb, bmin, bmax = cases.scene(name)
        assert inside(v9, bmin, bmax), name
        assert len(set(argb.tolist())) == len(argb) == v9.shape[0], name
        again = cases.scene.__wrapped__(name)
        assert np.array_equal(again[0], v9) and np.array_equal(again[1], argb), name          # deterministic
    v9, _, bmin, bmax = bs.morton_staircase(bs.STAIRCASE_MAX)
    assert [int(k) for k in bs.morton_keys(v9, bmin, bmax)] == [2 ** j - 1 for j in range(bs.STAIRCASE_MAX)]
    assert not np.any(bs.morton_keys(bs.corner_cluster(9), bmin, bmax))
    for n in (65, 300, 4097):
        v9, _, bmin, bmax = bs.same_centre(n)
        lo, hi = v9.min(axis=1), v9.max(axis=1)
        assert np.all(0.5 * (lo + hi) == bs.SAME_CENTRE)                 # the same centre, bit for bit
        assert len(set(bs.morton_keys(v9, bmin, bmax).tolist())) == 1
        assert len(np.unique(v9.reshape(n, 9), axis=0)) == n
    v9, _, bmin, bmax = cases.scene("duplicates")
    groups = bs.duplicate_groups(v9)
    assert len(set(groups.tolist())) == 150 and np.all(np.bincount(groups)[np.unique(groups)] == 4)
    assert np.all(groups <= np.arange(600)) and not np.array_equal(np.sort(groups), groups)      # shuffled
    v9, _, bmin, bmax = cases.scene("flat_thin")
    assert bmin[2] == bmax[2] == 0.0 and not np.any(v9[:, :, 2])
    assert not np.any(bs.morton_keys(v9, bmin, bmax) & np.uint64(0x1249249249249249))           # no z bit
    v9, _, bmin, bmax = cases.scene("flat_thick")
    assert bmax[2] - bmin[2] == 1.0 and np.all(0.5 * (v9[:, :, 2].min(axis=1) + v9[:, :, 2].max(axis=1)) == 0.0)
    assert len(set((bs.morton_keys(v9, bmin, bmax) & np.uint64(0x1249249249249249)).tolist())) == 1
    assert cases.chain_hittable() == cases.CHAIN_HITTABLE


def test_cluster_staircase_is_a_path_with_a_cluster_on_every_node():
    """One kept node per step under one triangle per leaf, a cluster's three equal keys two levels below it; the steps' boxes shrink
    towards the point, so the wide tree (wide_depth_model) is nearly as deep: the two scenes' depths are those the GPU test prints."""
    for m in (9, cases.PRIVATE_EDGE_STEPS, cases.WIDE_EDGE_STEPS, cases.WIDE_DEEP_STEPS):
        v9, _, bmin, bmax = bs.cluster_staircase(m)
        keys = bs.morton_keys(v9, bmin, bmax).reshape(m + 1, 3)
        assert np.all(keys == keys[:, :1]) and len(set(keys[:, 0].tolist())) == m + 1
        point = int(keys[m, 0])
        assert [(int(k) ^ point).bit_length() - 1 for k in keys[:m, 0]] == [61 - i for i in range(m)]      # step i leaves the path at key bit 61 - i
        depth, nodes, _ = bs.lbvh_model(v9, bmin, bmax, 1)
        assert (depth, nodes) == (m + 3, 3 * (m + 1) - 1)
    for name, want_depth, want_wide in (("wide_deep", 60, 48), ("wide_edge", 52, 40), ("private_edge", 32, 20)):
        v9, _, bmin, bmax = cases.scene(name)
        assert v9.shape[0] <= 400
        depth, nodes, _ = bs.lbvh_model(v9, bmin, bmax, cases.WIDE_LEAF)
        tree = bs.lbvh_nodes(v9, bmin, bmax, cases.WIDE_LEAF)
        assert len(tree) == nodes and depth == want_depth <= 62
        assert bs.wide_depth_model(tree, fp32=True) == bs.wide_depth_model(tree) == want_wide      # no comparison of areas is close
    assert (3 * 40 + 2) * 528 <= 65536 < (3 * 41 + 2) * 528              # wide_edge: the deepest tree the packet walks take in its four-wide form
    assert (3 * 20 + 2) * 1024 <= 65536 < (3 * 21 + 2) * 1024            # private_edge: ... and the private walks


# ---- the host builder, through a host-only scene ----
def host_scene(name, leaf=None, threads=None):
    s = sa.GpuScene(device=-1)
    s.set_triangles(*cases.scene(name))
    if leaf is not None:
        s.debug_set(L.DBG_BVH_LEAF, leaf)
    if threads is not None:
        s.debug_set(L.DBG_BUILD_THREADS, threads)
    return s


def test_host_builder_on_the_shrinking_chain():
    """200 triangles: (depth, wide depth) = (52, 17) with 4 triangles per leaf and (54, 23) with 1.  (52, 17) and the 54 are the
    figures of a build in the box [-0.5, 0.5]^3 too; the wide depth with one triangle per leaf was 25 there and is 23 in the chain's
    own box [-0.5, 0.75] x [-0.5, 0.5]^2 (the boxes' pad follows the root box), so it is pinned by the bound it has to meet: >= 21,
    where the four-wide private walks no longer fit LDS.  With the soup of the frames: (53, 18) and (55, 23)."""
    for leaf, want_depth, want_wide in ((4, 52, 17), (1, 54, None)):
        digests = set()
        for threads in (1, 4):
            s = host_scene("chain", leaf, threads)
            s.build((sa.MODE_BVH,))
            depth, nodes, tris, on_device = s.bvh_stats()
            wide = s.wide_tree_stats()
            assert depth == want_depth and depth <= 62 and tris == 200 and on_device == 0
            assert wide[4] == 200 and wide[3] == nodes + 1
            if want_wide is not None:
                assert wide[0] == want_wide
            else:
                assert wide[0] >= 21
            digests.add(s.bvh_digest())
        assert len(digests) == 1
    s = host_scene("deep", 1)
    s.build((sa.MODE_BVH,))
    assert s.bvh_stats()[0] <= 62 and s.wide_tree_stats()[0] >= 21
    s = host_scene("deep", 4)
    s.build((sa.MODE_BVH,))
    assert s.bvh_stats()[0] <= 62 and s.wide_tree_stats()[0] < 21


@pytest.mark.parametrize("leaf", [1, 4])
@pytest.mark.parametrize("name", ["soup", "deep", "chain", "limit", "wide_deep", "same_centre", "duplicates", "flat_thin", "flat_thick"])
def test_wide_depth_model_equals_the_host_collapse(name, leaf):
    """sah_nodes restates the host builder and wide_depth_model the collapse: depth, inner nodes and the wide depth of sr_bvh_stats and
    sr_wide_tree_stats on host-only, host-built scenes."""
    if name == "soup":
        tris = (bs.soup(1000, (0.0, 0.0, 0.0), 0.9, 21), bs.colours(1000), bs.UNIT_MIN, bs.UNIT_MAX)
    else:
        tris = cases.scene(name)
    s = sa.GpuScene(device=-1)
    s.set_triangles(*tris)
    s.debug_set(L.DBG_BVH_LEAF, leaf)
    s.build((sa.MODE_BVH,))
    nodes, depth = bs.sah_nodes(tris[0], tris[2], tris[3], leaf)
    assert s.bvh_stats()[:2] == (depth, len(nodes))
    assert s.wide_tree_stats()[0] == bs.wide_depth_model(nodes)


def test_rays_through_the_point_cross_every_level():
    """A ray that hits nothing visits a node on every level whose box it crosses.  The host-built chains: one of the rays through the
    point the chain converges to crosses depth - 1 levels of inner nodes; the cluster staircases: every ray through their point crosses
    all of them, more than the wide depth, and the rays that see the steps from behind hit nothing (bvh_shapes.cluster_staircase).
    The oracle's own counters cannot say this: its nearest mode tests every triangle and its tree mode walks the reference tree, so the
    levels are counted on the restated trees here, and the library's counters are asserted on the GPU."""
    for name in ("chain", "deep"):
        v9, _, bmin, bmax = cases.scene(name)
        s, d = cases.ray_batch(name, "through_point")
        miss = np.flatnonzero(~cases.oracle_trace(name, "through_point")["hit"].astype(bool))
        for leaf in (1, 4):
            nodes, depth = bs.sah_nodes(v9, bmin, bmax, leaf)
            assert max(bs.levels_crossed_model(nodes, bmin, bmax, s[i], d[i]) for i in miss) >= depth - 1, (name, leaf)
    for name in ("wide_deep", "wide_edge", "private_edge"):
        v9, _, bmin, bmax = cases.scene(name)
        nodes = bs.lbvh_nodes(v9, bmin, bmax, cases.WIDE_LEAF)
        depth, wide = bs.lbvh_model(v9, bmin, bmax, cases.WIDE_LEAF)[0], bs.wide_depth_model(nodes, fp32=True)
        s, d = cases.ray_batch(name, "through_point")
        miss = np.flatnonzero(~cases.oracle_trace(name, "through_point")["hit"].astype(bool))
        assert miss.size >= 4
        for i in miss:
            assert bs.levels_crossed_model(nodes, bmin, bmax, s[i], d[i]) >= depth - 1 > wide, (name, i)


def _assert_no_tree(s):
    for call in (s.bvh_stats, s.bvh_digest, s.wide_tree_stats):
        with pytest.raises(sa.SoftrayError) as e:
            call()
        assert e.value.code == L.SR_ERR_NOT_BUILT, call.__name__


@pytest.mark.parametrize("leaf", [4, 1])
@pytest.mark.parametrize("earlier", [None, "obj", "chain"])
def test_refused_host_build_leaves_no_tree(earlier, leaf):
    """400 triangles of the chain are 102 / 104 levels: refused, and nothing of the refused tree -- or of the accepted tree of an
    earlier model -- is left.  The next accepted build is that of a fresh scene."""
    s = sa.GpuScene(device=-1)
    s.debug_set(L.DBG_BVH_LEAF, leaf)
    if earlier:
        s.set_triangles(*cases.scene(earlier))
        s.build((sa.MODE_BVH, sa.MODE_REF_TREE))
        assert s.bvh_stats()[2] == cases.scene(earlier)[0].shape[0]
    s.set_triangles(*cases.scene("chain_refused"))
    with pytest.raises(sa.SoftrayError) as e:
        s.build((sa.MODE_BVH, sa.MODE_REF_TREE))
    assert e.value.code == L.SR_ERR_UNSUPPORTED
    _assert_no_tree(s)
    assert s.tree_stats()[0] > 0                                         # the reference tree of the same call stands
    with pytest.raises(sa.SoftrayError) as e:                           # ... and again, now with nothing to drop
        s.build((sa.MODE_BVH,))
    assert e.value.code == L.SR_ERR_UNSUPPORTED
    _assert_no_tree(s)
    s.set_triangles(*cases.scene("deep"))
    s.build((sa.MODE_BVH,))
    fresh = host_scene("deep", leaf)
    fresh.build((sa.MODE_BVH,))
    assert s.bvh_digest() == fresh.bvh_digest() and s.bvh_stats() == fresh.bvh_stats() and s.wide_tree_stats() == fresh.wide_tree_stats()


@pytest.mark.parametrize("name", cases.TIE_SCENES)
def test_host_builder_on_equal_centres(name):
    n = cases.scene(name)[0].shape[0]
    for leaf in (1, 4, 7):
        s = host_scene(name, leaf)
        s.build((sa.MODE_BVH,))
        depth, nodes, tris, _ = s.bvh_stats()
        wide_depth, wide_nodes, slots, leaves, leaf_tris = s.wide_tree_stats()          # raises on a broken link
        assert tris == leaf_tris == n
        assert leaves == nodes + 1 and slots == leaves + wide_nodes - 1
        if leaf == 1:
            assert nodes == n - 1
        if name == "same_centre":
            assert depth <= math.ceil(math.log2(n)) + 1                  # the nth_element fallback halves the range


# ---- the oracle agrees with itself on everything the GPU tests use ----
FRAME_CASES = [("deep", f) for f in cases.DEEP_FRAMES] + [("limit", f) for f in ("plain", "shadows")] + \
              [(s, f) for s in ("wide_deep", "private_edge") for f in cases.DEEP_FRAMES] + [("wide_edge", f) for f in ("plain", "shadows")] + \
              [(s, f) for s in cases.TIE_SCENES for f in cases.TIE_FRAMES] + [("chain_refused", "shadows"), ("obj", "plain"), ("obj", "shadows")]


@pytest.mark.parametrize("scene_name,frame_name", FRAME_CASES)
def test_oracle_modes_agree_on_the_frames(scene_name, frame_name):
    """Tree, brute force and nearest mode give one frame -- except in the root box without thickness.  The tree and the nearest mode
    clip every ray to the root box first (2e-10 thick there) and brute force does not: some grazing rays lose their hit to the clip,
    and where coplanar triangles overlap, the rounding of rayFrac along the clipped ray picks another winner than along the whole ray.
    There the GPU's brute-force frames have the oracle's brute-force frame to meet, the others the common frame of the other two."""
    want = cases.oracle_frame(scene_name, frame_name)
    brute = cases.oracle_frame(scene_name, frame_name, orc.MODE_BRUTE)
    if scene_name == "flat_thin":
        differ = brute != want
        assert 0 < np.count_nonzero(differ) < want.size // 10
    else:
        assert np.array_equal(brute, want)
    assert np.array_equal(cases.oracle_frame(scene_name, frame_name, orc.MODE_REF_TREE), want)
    assert 0 < np.count_nonzero(want != cases.BACKGROUND) < want.size


@pytest.mark.parametrize("scene_name", ["deep", "limit", "chain_refused", "wide_deep", "wide_edge", "private_edge"] + list(cases.TIE_SCENES))
def test_frames_show_background_lit_and_shadowed_pixels(scene_name):
    background, lit, shadowed = cases.pixel_classes(scene_name)
    assert background > 20 and lit > 20 and shadowed > 20, (background, lit, shadowed)
    if scene_name == "deep":
        assert np.count_nonzero(cases.oracle_frame("deep", "mirror") != cases.oracle_frame("deep", "plain")) > 20


RAY_CASES = [(s, f) for s in ("chain", "chain_hittable") for f in cases.RAY_FAMILIES] + [("limit", "at_triangles")] + \
            [(s, f) for s in ("wide_deep", "wide_edge", "private_edge") for f in cases.RAY_FAMILIES]


@pytest.mark.parametrize("scene_name,family", RAY_CASES)
def test_oracle_modes_agree_on_the_ray_batches(scene_name, family):
    """Tree and nearest mode clip the ray to the root box first, brute force does not: the first two agree in everything, brute force
    in what does not depend on where the ray starts."""
    near = cases.oracle_trace(scene_name, family, "nearest")
    tree = cases.oracle_trace(scene_name, family, "tree")
    brute = cases.oracle_trace(scene_name, family, "brute")
    for key in cases.TRACE_KEYS:
        assert np.array_equal(tree[key], near[key]), key
    for key in ("hit", "tri_index", "color", "normal"):
        assert np.array_equal(brute[key], near[key]), key
    hit = near["hit"].astype(bool)
    if family == "at_triangles" and scene_name == "limit":
        # the low steps of the staircase are smaller than 1e-7: "zero" normals like the chain's small end (cases.chain_hittable), never hit
        m = cases.limit_staircase_length()
        assert len(np.unique(near["tri_index"][hit & (near["tri_index"] < m)])) >= 20
    elif scene_name in cases.WIDE_STEPS:
        # the steps hide one another; the small ones have "zero" normals like the chain's small end
        stairs = 3 * (cases.WIDE_STEPS[scene_name] + 1)                   # (a fifth of them: half face away from the rays' start, the larger hide the smaller)
        assert len(np.unique(near["tri_index"][hit])) >= (10 if family == "through_point" else stairs // 5)
        assert (~hit).sum() >= (4 if family == "through_point" else 1)
    elif family == "at_triangles":
        n = cases.CHAIN_HITTABLE                                          # of the 200 as of the 29: triangles 0 .. 28
        aimed = np.repeat(np.arange(cases.scene(scene_name)[0].shape[0]), 5)
        assert np.array_equal(np.unique(near["tri_index"][hit]), np.arange(n))               # every triangle that can be hit is hit ...
        assert np.all(near["tri_index"][hit] == aimed[hit])                                  # ... by the rays aimed at it,
        assert np.array_equal(hit, aimed < n)                                                # by all of them, and no other ray hits
    else:
        assert not hit.any()                   # the point the chain converges to lies in no triangle; the near misses miss


def test_oracle_returns_the_lowest_copy_of_a_duplicate():
    """Exact copies tie in everything: every mode of the oracle reports the copy with the lowest TriangleIndex, as the reference's
    strict `<` over the triangles in index order does."""
    groups = bs.duplicate_groups(cases.scene("duplicates")[0])
    near = cases.oracle_trace("duplicates", "at_triangles", "nearest")
    hit = near["hit"].astype(bool)
    assert np.count_nonzero(hit) > 500 and len(np.unique(near["tri_index"][hit])) > 50
    for target in ("nearest", "tree", "brute"):
        res = cases.oracle_trace("duplicates", "at_triangles", target)
        assert np.array_equal(res["hit"], near["hit"]) and np.array_equal(res["tri_index"], near["tri_index"]), target
        assert np.array_equal(res["color"], near["color"]), target
    assert np.array_equal(groups[near["tri_index"][hit]], near["tri_index"][hit])
