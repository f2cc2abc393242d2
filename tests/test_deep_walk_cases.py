"""The inputs of tests/test_gpu_deep_walks.py are not vacuous: checked on the CPU with the oracle and the models alone.

Every outcome class of a call's answer holds at least 5 % of its batch.  The exception is `chain`, by its geometry: its triangles are
coplanar, disjoint and one-sided, so no ray has two hits on it and no ray from a light reaches a point of it through another triangle;
there the other class is checked to be empty, so that a second hit or a shadow the library reports is a wrong answer, not a missing case."""
import numpy as np
import pytest

import all_hits_model as ahm
import bvh_shape_cases as bsc
import closest_points_cases as cpc
import closest_points_model as cpm
import deep_walk_cases as dw
import occluded_rays_cases as occ
import shadow_points_model as spm

SHARE = 0.05


def both(mask):
    return SHARE <= dw.share(mask) <= 1.0 - SHARE


@pytest.mark.parametrize("scene", list(dw.SCENES))
def test_ray_batches_hit_and_miss(scene):
    s, d = dw.ray_batch(scene)
    assert s.shape == d.shape and s.shape[0] <= 4096
    res = dw.oracle_batch(scene)
    assert both(res["hit"]), dw.share(res["hit"])
    assert both(occ.model(res, dw.batch_limits(scene)))                  # occluded / not under the rotated limits
    for origin in dw.ORIGINS:
        assert dw.origin_dirs(scene, origin).shape[0] <= 4096
        assert both(dw.oracle_origin(scene, origin)["hit"]), origin
    bmin, bmax = bsc.scene(scene)[2:]
    assert all(not (bmin[a] <= dw.ORIGINS["outside"][a] <= bmax[a]) for a in range(3))
    assert all(bmin[a] < dw.ORIGINS["inside"][a] < bmax[a] for a in range(3))


@pytest.mark.parametrize("scene", list(dw.SCENES))
def test_all_hits_rows_are_empty_and_hold_two(scene):
    s, d = dw.ray_batch(scene)
    count = ahm.rows(ahm.Candidates(bsc.scene(scene), (), s, d, False).lists(None), 8)["count"]
    assert dw.share(count == 0) >= SHARE
    if scene == "chain":
        assert count.max() == 1
    else:
        assert dw.share(count >= 2) >= SHARE


@pytest.mark.parametrize("scene", list(dw.SCENES))
def test_closest_points_answer_and_refuse(scene):
    points = dw.closest_points(scene)
    a = cpm.Answers(points, bsc.scene(scene)[0])
    assert not a.nan_pairs.any() and (a.tri >= 0).all()
    out = a.outputs(cpc.limit_kinds(a.dist)[0])
    assert both(out["tri_index"] >= 0)
    assert len(np.unique(a.tri)) >= 20


@pytest.mark.parametrize("scene", list(dw.SCENES))
def test_surface_points_are_lit_and_shadowed(scene):
    pos, nrm, col = dw.surface_points(scene)
    assert 100 <= pos.shape[0] <= 4096
    f = dw.frame(scene, shadows=True, shadow_samples=dw.SHADOW_SAMPLES)
    esc = spm.escapes(bsc.oracle_scene(scene), f, pos, nrm, dw.TRACE_NEAREST)
    if scene == "chain":
        assert (esc == dw.SHADOW_SAMPLES).all()
    else:
        assert both(esc == dw.SHADOW_SAMPLES), dw.share(esc == dw.SHADOW_SAMPLES)
