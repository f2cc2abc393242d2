"""The ray sets of the any-hit tests (tests/occluded_rays_cases.py) against the oracle, on the CPU: the model of sr_occluded_rays is
hit & (ray_frac <= limit) over the oracle's trace of (start, D) with D = end - start done in numpy.  Between 10 % and 90 % of the regular rays of
every set are occluded, every kind of limit and every kind of irregular ray occurs, and the far set's clip offset exceeds some limits."""
import numpy as np
import pytest

import gbuffer_cases as gbc
import occluded_rays_cases as occ
import pathtrace_model as ptm


@pytest.fixture(scope="module")
def oracles():
    return {name: gbc.oracle_scenes(name) for name in occ.SCENES}


@pytest.mark.parametrize("scene", occ.SCENES)
def test_between_a_tenth_and_nine_tenths_of_every_set_are_occluded(oracles, scene):
    tree, brute = oracles[scene]
    prims = gbc.scene_data(scene)[1]
    for name in occ.SETS:
        rs = occ.ray_set(scene, name)
        for variant in rs.limits:
            reg = rs.regular(variant)
            lim = rs.limit_array(variant)
            for mode in ("tree", "brute", "bvh"):
                res = occ.oracle_trace(tree, brute, mode, False, prims, rs.starts, rs.D)
                got = occ.model(res, lim)
                assert set(np.unique(got)) <= {0, 1}
                k = int(got[reg].sum())
                total = int(reg.sum())
                if total >= 16:
                    assert 0.1 * total < k < 0.9 * total, (scene, name, variant, mode, k, total)
                # the limits that can never admit a hit, and the one that admits every hit
                with np.errstate(invalid="ignore"):
                    never = np.isnan(lim) | (lim < 0.0)
                assert not got[never].any()
                assert np.array_equal(got[lim == np.inf], np.asarray(res["hit"])[lim == np.inf])


@pytest.mark.parametrize("scene", occ.SCENES)
def test_every_kind_of_limit_and_of_irregular_ray_occurs(scene):
    for name in occ.SETS:
        rs = occ.ray_set(scene, name)
        kinds = [occ.LIMIT_KINDS[occ.limit_kind(i)] for i in range(rs.n)]
        if rs.n >= 63:
            assert set(kinds) == set(occ.LIMIT_KINDS), name
            hits = rs.f != 1.0
            assert {k for k, h in zip(kinds, hits) if h} == set(occ.LIMIT_KINDS), name      # ... each of them on a ray that hits
    for name, want in (("irregular", occ.IRREGULAR_DIR_KINDS), ("irregular_ends", occ.IRREGULAR_END_KINDS)):
        rs = occ.ray_set(scene, name)
        assert {k for k in rs.kinds if k} == set(want)
        # by direction and start alone every marked ray is irregular and no other is; the rotation adds the NaN and -inf limits
        by_ray = occ.regular(rs.starts, rs.dirs, rs.endpoints, None)
        assert np.array_equal(~by_ray, np.array([bool(k) for k in rs.kinds]))
        lim = rs.limits["rot"]
        reg = rs.regular("rot")
        assert np.array_equal(reg, by_ray & ~np.isnan(lim) & (lim != -np.inf))
        marked = [i for i, k in enumerate(rs.kinds) if k]
        assert {occ.LIMIT_KINDS[occ.limit_kind(i)] for i in marked} == set(occ.LIMIT_KINDS), name
    assert occ.ray_set(scene, "irregular_ends").endpoints and not occ.ray_set(scene, "irregular").endpoints


@pytest.mark.parametrize("scene", occ.SCENES)
def test_set_sizes_and_the_far_sets_clip_offsets(scene):
    for n in (1, 63, 64, 65, 449):
        assert occ.ray_set(scene, "n%d" % n).n == n
    rs = occ.ray_set(scene, "far")
    lo, hi = occ.box(scene)
    assert np.all((rs.starts < lo - (hi - lo)) | (rs.starts > hi + (hi - lo)))                # far outside on every axis
    # the distance to the box over |D| bounds the clip offset from below: it exceeds the small limits of rays that do hit
    gap = np.linalg.norm(np.maximum(np.maximum(lo - rs.starts, rs.starts - hi), 0.0), axis=1) / np.linalg.norm(rs.D, axis=1)
    lim = rs.limits["rot"]
    hits = rs.f != 1.0
    with np.errstate(invalid="ignore"):
        assert (hits & (lim >= 0.0) & (lim < gap)).sum() > 20 and (hits & (lim > gap) & np.isfinite(lim)).sum() > 20
    assert np.all(rs.f[hits] > gap[hits])
    # the shadow segments end PROBE_OFFSET above the surface the grid hit, the probes start there
    sh, pr = occ.ray_set(scene, "shadow"), occ.ray_set(scene, "probes")
    assert sh.endpoints and not pr.endpoints and np.array_equal(sh.dirs, pr.starts) and sh.n == pr.n >= 64
    assert np.all((pr.dirs * occ.grid_hits(scene)[1]).sum(axis=1) >= 0.0)


def test_the_model_is_the_comparison_of_the_issue():
    res = dict(hit=np.array([1, 1, 1, 0, 1, 1], dtype=np.uint8), ray_frac=np.array([0.5, 0.5, 0.5, 0.0, 0.5, 0.0]))
    lim = np.array([0.5, np.nextafter(0.5, 0.0), np.nan, 1.0, np.inf, 0.0])
    assert occ.model(res, lim).tolist() == [1, 0, 0, 0, 1, 1]
    assert ptm.TRACE_NEAREST == 3
