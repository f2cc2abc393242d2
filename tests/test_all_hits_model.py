"""The inputs of the all-hits tests, pinned on the CPU with the model of tests/all_hits_model.py (the oracle's one-triangle and one-primitive
scenes), so that tests/test_gpu_all_hits.py cannot pass on empty ground: how many hits, ties and overfull rows every ray set holds, and that the
model's first entry is the whole scene's nearest hit."""
import os

import numpy as np
import pytest

import all_hits_cases as ahc
import all_hits_model as ahm
import gbuffer_cases as gbc
import occluded_rays_cases as occ
from helpers import ROOT, orc

_CAND = {}


def candidates(scene, name, brute=False):
    key = (scene, name, brute)
    if key not in _CAND:
        tris, prims = ahc.scene_data(scene)
        rs = ahc.ray_set(scene, name)
        reg = ahc.regular(rs, None)
        _CAND[key] = (ahm.Candidates(tris, (), np.ascontiguousarray(rs.starts[reg]), np.ascontiguousarray(rs.D[reg]), brute), reg)
    return _CAND[key]


def counts(lists):
    return np.array([f.shape[0] for f, _ in lists])


def test_layers_is_the_scene_the_issue_describes():
    v9, argb, lo, hi = ahc.layers_scene()
    assert v9.shape == (360, 9) and argb.shape == (360,) and np.all(lo == -0.5) and np.all(hi == 0.5)
    t = v9.reshape(-1, 3, 3)
    nz = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])[:, 2]
    assert (nz > 0).sum() == 280 and (nz < 0).sum() == 80                     # ten of the forty layers are wound the other way
    assert len({r.tobytes() for r in v9}) == 320                               # five layers twice
    assert np.abs(t[:, :, 2]).max() < 0.45 and np.abs(t[:, :, :2]).max() == 0.4 and len(set(t[:, 0, 2].tolist())) == 40


@pytest.mark.parametrize("name", ["through", "far_through"])
def test_through_sets_are_deep_and_tied(name):
    c, _ = candidates("layers", name)
    L = c.lists()
    n = counts(L)
    assert n.shape == (256,) and n.min() >= 4 and n.max() == 35
    assert (n > 32).sum() >= 50 and ahm.tied(L).sum() >= 60
    if name == "far_through":                                                 # the start lies outside the box: every ray_frac carries an offset
        assert min(f[0] for f, _ in L) > 2.9


def test_oblique_set():
    c, _ = candidates("layers", "oblique")
    L = c.lists()
    assert (counts(L) > 16).sum() >= 50 and ahm.tied(L).sum() >= 100


def test_edges_set():
    c, _ = candidates("layers", "edges")
    n = counts(c.lists())
    assert n.shape == (20,) and n.min() >= 20 and (n > 64).sum() >= 5 and n.max() == 210


def test_small_segments_cross_more_than_one_triangle():
    c, _ = candidates("small", "segments")
    assert (counts(c.lists()) >= 2).sum() >= 100


@pytest.mark.parametrize("scene", ahc.SCENES)
def test_the_first_entry_is_the_whole_scenes_nearest_hit(scene):
    tris, _ = ahc.scene_data(scene)
    whole = orc.Scene()
    whole.set_triangles(*tris)
    assert whole.build_tree() == 0
    brute = orc.Scene()
    brute.set_triangles(*tris)
    for name in ahc.sets_of(scene):
        rs = ahc.ray_set(scene, name)
        for is_brute, o, target in ((False, whole, ahm.TRACE_NEAREST), (True, brute, ahm.TRACE_BRUTE)):
            c, reg = candidates(scene, name, is_brute)
            L = c.lists()
            near = o.trace(target, np.ascontiguousarray(rs.starts[reg]), np.ascontiguousarray(rs.D[reg]))
            hit = np.asarray(near["hit"]).astype(bool)
            assert np.array_equal(counts(L) > 0, hit), (name, is_brute)
            first = np.array([f[0] if f.shape[0] else 0.0 for f, _ in L])
            assert np.array_equal(first, np.where(hit, near["ray_frac"], 0.0)), (name, is_brute)
            untied = hit & ~ahm.first_tied(L)
            idx = np.array([ix[0] if ix.shape[0] else -1 for _, ix in L])
            assert np.array_equal(idx[untied], np.asarray(near["tri_index"])[untied]), (name, is_brute)


def test_one_primitive_scenes_answer_like_the_root_geometry():
    """The extra elements of "cube" through the oracle's one-primitive scenes: where an element is the root geometry's nearest hit, the
    ray_frac is the same."""
    tris, prims = ahc.scene_data("cube")
    rs = ahc.ray_set("cube", "segments")
    c = ahm.Candidates(tris, prims, rs.starts, rs.D, False)
    assert c.index[:3].tolist() == [-2, -3, -4] and c.hit[:3].any(axis=1).sum() >= 2
    tree, _ = gbc.oracle_scenes("cube")
    root = tree.trace(ahm.TRACE_ROOT_TREE, rs.starts, rs.D)
    on_extra = np.asarray(root["hit"]).astype(bool) & (np.asarray(root["tri_index"]) < 0)
    assert on_extra.sum() > 20
    best = np.where(c.hit[:3], c.frac[:3], np.inf).min(axis=0)
    assert np.array_equal(best[on_extra], np.asarray(root["ray_frac"])[on_extra])


def test_the_kernels_and_the_call_are_where_the_documents_say():
    src = open(os.path.join(ROOT, "softray_amd", "csrc", "sr_allhits.hip")).read()
    assert "void k_ah_walk(" in src and "void k_ah_loop(" in src
    kernels = open(os.path.join(ROOT, "softray_amd", "csrc", "sr_kernels.hip")).read()
    assert 'case K_ALL_HITS: return "k_all_hits";' in kernels and 'case K_ALL_HITS_SORT: return "k_all_hits_sort";' in kernels
    assert "sr_allhits.hip" in open(os.path.join(ROOT, "softray_amd", "csrc", "Makefile")).read()
    assert occ.SETS == ahc.sets_of("small") == ahc.sets_of("cube")


def test_inside_outside_recipe_on_the_torus():
    """tests/mesh_cases.py's torus is closed and wound outward: with one-sided triangles (exits - entries) is 1 for a point inside the tube and 0
    outside.  Entries: the hits of the ray (p, d) with no limit; exits: those of the segment from p + L d back to p."""
    import mesh_cases as mc
    tris = mc.scene("torus")
    p, d, inside = ahc.torus_points()
    far = p + ahc.TORUS_REACH * d
    assert (np.abs(far).max(axis=1) > 0.5).all() and np.abs(p).max() < 0.5
    entries = counts(ahm.Candidates(tris, (), p, d, False).lists())
    exits = counts(ahm.Candidates(tris, (), far, np.ascontiguousarray(p - far), False).lists(np.ones(p.shape[0])))
    assert np.array_equal(exits.astype(int) - entries.astype(int), inside.astype(int))
    assert inside.sum() == 48 and (entries > 0).sum() > 20 and exits.max() >= 2
