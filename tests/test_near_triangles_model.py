"""The model of sr_near_triangles (tests/near_triangles_model.py) and the radii of tests/near_triangles_cases.py, pinned on the CPU so that no
GPU test can pass vacuously: what the scenes hold under the radius extent / 8 and under the rotating radii, the ties across the K = 4 cut,
neighbours with distinct d2 and one rounded distance, the NaN pairs, the model's slot 0 against the model of sr_closest_points; and the
list of softray_amd/csrc/sr_near_list.h, built into a stand-alone host program (tests/cpp/near_list_check.cpp, its own main, no library)
with g++ -ffp-contract=off under the address and undefined-behaviour sanitizers, against the model in every byte."""
import os
import subprocess

import numpy as np
import pytest

import closest_points_cases as cpc
import closest_points_model as cpm
import near_triangles_cases as ntc
import near_triangles_model as ntm
from helpers import GOLDEN, ROOT

# scene: points with count > 64 under the radius extent / 8 (elsewhere none)
OVER_64 = {"layers": 66, "torus": 1575, "slivers": 2018, "limit": 61, "duplicates": 9}
# scene: points whose 4th and 5th smallest d2 are one finite number -- the index decides who is inside the K = 4 cut
TIES_AT_4 = {"layers": 585, "torus": 1652, "slivers": 226, "flat_thin": 97, "degenerate": 77}


@pytest.mark.parametrize("scene", ntc.SCENES)
def test_what_the_scenes_hold(scene):
    m = ntc.model(scene)
    none, radii, e8 = m.sets["none"], m.sets["radii"], m.sets["extent8"]
    P = m.points.shape[0]
    T = cpc.scene(scene)[0].shape[0]
    # the radius extent / 8: empty sets, and sets beyond the K = 4 row
    assert (e8 == 0).sum() >= 300 and (e8 > 4).sum() >= 700
    if scene == "cut":
        assert (e8 == 0).sum() == 302
    if scene == "small":
        assert (e8 > 4).sum() == 741
    assert (e8 > 64).sum() == OVER_64.get(scene, 0)
    if scene == "slivers":
        assert e8.max() == 2048
    # ties across the K = 4 cut
    tie = (none.count >= 5) & (none.d2[:, 3] == none.d2[:, 4]) & np.isfinite(none.d2[:, 4])
    if scene in TIES_AT_4:
        assert tie.sum() == TIES_AT_4[scene]
        assert (none.index[tie, 3] < none.index[tie, 4]).all()
    # neighbouring entries with distinct d2 and one rounded distance (points with such a pair in the 64 slots of the row without a limit)
    both = (none.index[:, 1:] >= 0) & (none.index[:, :-1] >= 0)
    twins = both & (none.d2[:, 1:] != none.d2[:, :-1]) & (none.dist[:, 1:] == none.dist[:, :-1])
    equal = both & (none.d2[:, 1:] == none.d2[:, :-1])
    assert twins.any(axis=1).sum() >= (5 if scene != "duplicates" else 1) and equal.any()
    if scene == "layers":
        assert twins.any(axis=1).sum() >= 300
    # NaN pairs that must be skipped
    assert (m.nan_pairs > 0).sum() >= 3
    if scene == "degenerate":
        assert (m.nan_pairs > 0).sum() == 2869
    assert np.array_equal(none.count, T - m.nan_pairs)
    # rows: ordered by (d2, index), padded, dist non-decreasing
    for rows in (none, radii):
        kept = rows.index >= 0
        assert np.array_equal(kept.sum(axis=1), np.minimum(rows.count, ntm.SLOTS))
        assert not (kept[:, 1:] & ~kept[:, :-1]).any()
        pair = kept[:, 1:]
        d_lo, d_hi, j_lo, j_hi = rows.d2[:, :-1][pair], rows.d2[:, 1:][pair], rows.index[:, :-1][pair], rows.index[:, 1:][pair]
        assert ((d_lo < d_hi) | ((d_lo == d_hi) & (j_lo < j_hi))).all()
        assert (rows.dist[:, :-1][pair] <= rows.dist[:, 1:][pair]).all()
        assert not rows.dist[~kept].any() and not rows.pos[~kept].any() and not rows.uv[~kept].any()
    # the rotating radii: what each kind admits
    has = none.count > 0
    for k, name in enumerate(ntc.RADIUS_KINDS):
        sel = m.kind == k
        cnt = radii.count[sel & has]
        assert sel.sum() >= 230
        if name == "inf":
            assert np.array_equal(cnt, none.count[sel & has])
        elif name in ("nan", "-inf", "negative"):
            assert not radii.count[sel].any()
        elif name == "zero":
            assert (cnt > 0).any() and (cnt == 0).any()
        elif name in ("nearest", "double"):
            assert (cnt >= 1).all()
        elif name == "fourth":
            assert (cnt >= 4).all()
        elif name == "below_fourth":
            assert (cnt <= 3).all() and ((cnt == 3).any() or scene == "duplicates")         # (duplicates: four copies share the 4th distance)
        else:
            assert (cnt == 0).any() and (cnt > 4).any()
    assert (radii.count > 64).sum() >= 300 or scene == "small"
    assert P <= 4096 and T <= 2200


@pytest.mark.parametrize("scene", ntc.SCENES)
def test_slot_0_is_the_model_of_closest_points(scene):
    m = ntc.model(scene)
    a = cpm.Answers(m.points, cpc.scene(scene)[0])
    for which in ("none", "radii"):
        want = a.outputs(m.limit(which))
        got = m.sets[which].closest()
        for k in ("tri_index", "dist", "pos", "uv"):
            assert cpm.same_bits(got[k], want[k]), (scene, which, k)
        assert np.array_equal(m.sets[which].count > 0, want["tri_index"] >= 0)


def test_rows_of_k_cut_the_model_rows():
    m = ntc.model("small")
    for k in ntc.KS:
        r = m.want("radii", k)
        assert {key: r[key].shape for key in ntm.KEYS} == ntm.shapes(m.points.shape[0], k)
        assert all(r[key].dtype == ntm.NP_TYPES[key] for key in ntm.KEYS)
        assert np.array_equal((r["index"] >= 0).sum(axis=1), np.minimum(r["count"], k))


# (the sanitizers' runtimes are linked statically: the program must start whatever else the loader has been told to load first)
SANITIZED = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g")


def test_the_header_list_equals_the_model(tmp_path):
    """The stand-alone host program (its own main, nothing loaded into Python): the header's list and threshold over the routine's results,
    rows in host memory between guard words, K = 1, 4 and 64, without limits and under the rotating radii -- every byte against the model."""
    path = os.path.join(GOLDEN, cpc.CHECK_FILE)
    tris, pts = cpc.read_check_file(path)
    P = pts.shape[0]
    limits = np.zeros(P)

    def make(first, block):
        lim, _ = ntc.radius_kinds(first, block.dist[:, 0], block.dist[:, 3], 0.25)
        limits[first:first + lim.shape[0]] = lim
        return {"radii": lim}

    sets = ntm.near_sets(pts, tris, make)
    exe = str(tmp_path / "near_list_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", *SANITIZED, "-o", exe, os.path.join(ROOT, "tests", "cpp", "near_list_check.cpp")])
    lim_file, out = str(tmp_path / "limits.bin"), str(tmp_path / "out.bin")
    limits.tofile(lim_file)
    r = subprocess.run([exe, path, lim_file, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, dtype=np.uint8)
    at = 0
    for which in ("none", "radii"):
        for k in (1, 4, 64):
            want = sets[which].rows(k)
            for key in ntm.KEYS:
                size = want[key].size * want[key].itemsize
                got = raw[at:at + size].view(ntm.NP_TYPES[key]).reshape(want[key].shape)
                assert ntm.same_bits(got, want[key]), (which, k, key, np.argwhere(got != want[key])[:4])
                at += size
    assert at == raw.size
    r = sets["radii"]
    assert (r.count == 0).sum() > 30 and (r.count > 4).sum() > 15
    assert (sets["nan_pairs"] > 0).any() and np.isinf(sets["none"].dist).any()
