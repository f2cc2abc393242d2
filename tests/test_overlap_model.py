"""The model of sr_overlap_triangles (tests/overlap_model.py) and the queries of tests/overlap_cases.py, pinned on the CPU so that no GPU test
can pass on nothing.
(a) On lattice triangles with coordinates in {-2 .. 2}, where FP64 is exact and touching, collinear edges and shared vertices are everywhere,
    the model equals an exact test in integers that is written independently: the two sections of the triangles with each other's plane, as
    rational intervals on the common line, and closed interval overlap -- not the edge test.  No coplanar pair is reported.
(b) The header softray_amd/csrc/sr_tri_overlap.h, built into a stand-alone host program (tests/cpp/tri_overlap_check.cpp, its own main, no
    library) with g++ -ffp-contract=off under the address and undefined-behaviour sanitizers, gives the model's masks for all pairs of every
    scene's queries and the model's rows, with the triangles offered in ascending and in descending order.
(c) What the sets hold.  Measured with this generator (default_rng(5)): every set of every scene holds queries with count 0 and with
    count >= 1, except the ones of ONE_SIDED below (a mesh of separate sheets has no neighbours, every triangle of a closed mesh has some);
    `probes` reaches counts of 264 (layers), 2049 (slivers), 114 (torus) and 116 (duplicates); the torus' full self-query has 12 or 11 per
    triangle, a zero diagonal, every pair that shares one vertex, and a mask matrix that equals its transpose with the halves swapped;
    a triangle of `duplicates` never reports its copies."""
import os
import subprocess

import numpy as np
import pytest

import closest_points_cases as cpc
import overlap_cases as oc
import overlap_model as om
from helpers import ROOT


# ---- (a) the exact test: sections and interval overlap, in int64 (|coordinate| <= 2: every product below stays under 2^40) ----
def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def _dot(u, v):
    return (u * v).sum(axis=1)


def _section(d, p):
    """The section of a triangle with a plane, on a line: d [N][3] the vertices' signed plane distances, p [N][3] their positions along the line
    (integers).  Returns (lo_num, lo_den, hi_num, hi_den, have): the rational interval of the points of the triangle in the plane."""
    N = d.shape[0]
    lo_n, lo_d = np.zeros(N, dtype=np.int64), np.ones(N, dtype=np.int64)
    hi_n, hi_d = np.zeros(N, dtype=np.int64), np.ones(N, dtype=np.int64)
    have = np.zeros(N, dtype=bool)
    cands = [(p[:, i], np.ones(N, dtype=np.int64), d[:, i] == 0) for i in range(3)]                      # a vertex in the plane
    for i, j in ((0, 1), (1, 2), (2, 0)):                                                                  # an edge through the plane
        num, den = p[:, j] * d[:, i] - p[:, i] * d[:, j], d[:, i] - d[:, j]
        neg = den < 0
        cands.append((np.where(neg, -num, num), np.where(neg, -den, den), d[:, i] * d[:, j] < 0))
    for num, den, valid in cands:
        den = np.where(valid, den, 1)
        lower = valid & (~have | (num * lo_d < lo_n * den))
        higher = valid & (~have | (num * hi_d > hi_n * den))
        lo_n, lo_d = np.where(lower, num, lo_n), np.where(lower, den, lo_d)
        hi_n, hi_d = np.where(higher, num, hi_n), np.where(higher, den, hi_d)
        have |= valid
    return lo_n, lo_d, hi_n, hi_d, have


def exact_classes(A, B):
    """A, B int64 [N][3][3] -> (degenerate, coplanar, intersect) [N]."""
    nA, nB = _cross(A[:, 1] - A[:, 0], A[:, 2] - A[:, 0]), _cross(B[:, 1] - B[:, 0], B[:, 2] - B[:, 0])
    degenerate = ~nA.any(axis=1) | ~nB.any(axis=1)
    dA = np.stack([_dot(nB, A[:, i] - B[:, 0]) for i in range(3)], axis=1)                               # A's vertices against B's plane
    dB = np.stack([_dot(nA, B[:, i] - A[:, 0]) for i in range(3)], axis=1)
    coplanar = ~degenerate & ~dA.any(axis=1)
    apart = (dA > 0).all(axis=1) | (dA < 0).all(axis=1) | (dB > 0).all(axis=1) | (dB < 0).all(axis=1)
    D = _cross(nA, nB)                                                                                   # the common line's direction
    pA = np.stack([_dot(D, A[:, i]) for i in range(3)], axis=1)
    pB = np.stack([_dot(D, B[:, i]) for i in range(3)], axis=1)
    alo_n, alo_d, ahi_n, ahi_d, have_a = _section(dA, pA)
    blo_n, blo_d, bhi_n, bhi_d, have_b = _section(dB, pB)
    meet = have_a & have_b & (alo_n * bhi_d <= bhi_n * alo_d) & (blo_n * ahi_d <= ahi_n * blo_d)
    return degenerate, coplanar, ~degenerate & ~coplanar & ~apart & meet


def test_the_model_equals_exact_arithmetic_on_lattice_pairs():
    rng = np.random.default_rng(11)
    pairs = rng.integers(-2, 3, size=(260000, 2, 3, 3))
    flat = rng.integers(-2, 3, size=(6000, 2, 3, 3))                                                     # six points in one lattice plane
    axis = rng.integers(0, 3, size=6000)
    flat[np.arange(6000), :, :, axis] = rng.integers(-2, 3, size=6000)[:, None, None]
    pairs = np.concatenate([pairs, flat]).astype(np.int64)
    A, B = pairs[:, 0], pairs[:, 1]
    degenerate, coplanar, want = exact_classes(A, B)
    got = om.pair_masks(A.astype(np.float64), B.astype(np.float64))
    proper = ~degenerate & ~coplanar
    assert proper.sum() >= 100000 and want[proper].sum() >= 30000 and (~want[proper]).sum() >= 30000
    assert np.array_equal(got[proper] != 0, want[proper]), np.flatnonzero(proper & ((got != 0) != want))[:8]
    assert coplanar.sum() >= 3000 and not got[coplanar].any()
    # touching is everywhere in this set: pairs that meet in a shared lattice vertex only, and edges that lie in the other's plane
    shared = (A[:, :, None, :] == B[:, None, :, :]).all(axis=-1).any(axis=(1, 2))
    assert (proper & shared & want).sum() >= 5000
    # swapping the roles swaps the halves
    assert np.array_equal(om.pair_masks(B.astype(np.float64), A.astype(np.float64)), om.swap_halves(got))


def test_the_rule_of_equal_points_and_special_values():
    a, b, c, d = (np.array(p, dtype=np.float64) for p in ((0.1, 0.2, 0.3), (0.7, -0.4, 0.9), (-0.3, 0.8, 0.5), (0.25, 0.35, -0.45)))
    assert om.vol(a, b, c, d) != 0.0
    for pts in ((a, a, c, d), (a, b, a, d), (a, b, c, a), (a, b, b, d), (a, b, c, b), (a, b, c, c)):
        assert om.vol(*pts) == 0.0
    t = np.array([a, b, c])
    assert om.pair_masks(t, t)[0] == 0 and om.pair_masks(t, t[[1, 2, 0]])[0] == 0                        # itself, and itself renamed
    nan = t.copy(); nan[1, 2] = np.nan
    inf = t.copy(); inf[0, 0] = np.inf
    other = np.array([d, (0.3, 0.1, 0.9), (0.2, 0.3, 0.1)])
    for q in (nan, inf):
        assert om.pair_masks(q, other)[0] == 0 and om.pair_masks(other, q)[0] == 0
    # a needle through a triangle: bit 0 alone; the other way round: bit 3 alone
    tri = np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)])
    needle = np.array([(0.25, 0.25, -1.0), (0.25, 0.25, 1.0), (0.25, 0.25, 1.0)])
    assert om.pair_masks(needle, tri)[0] == 0b000101 and om.pair_masks(tri, needle)[0] == 0b101000       # (edges 0 and 2 of the needle are the same segment)
    far = needle + np.array([5.0, 0.0, 0.0])
    assert om.pair_masks(far, tri)[0] == 0


# ---- (c) what the sets hold ----
# (scene, set): only count 0, or only count >= 1
ONE_SIDED = {("layers", "self"): 0, ("layers", "moved"): 0, ("flat_thin", "self"): 0, ("flat_thin", "moved"): 0, ("torus", "self"): 1}
PROBES_OVER_64 = {"layers": (17, 264), "slivers": (23, 2049), "torus": (8, 114), "duplicates": (8, 116), "cube": (5, 100), "far_probe": (1, 72)}


@pytest.mark.parametrize("scene", oc.SCENES)
def test_what_the_sets_hold(scene):
    m = oc.model(scene)
    v9, _, bmin, bmax = cpc.scene(scene)
    n, T = m.queries.shape[0], v9.shape[0]
    assert n <= 1024 and T <= 2200
    count = m.rows.count
    for name, sl in oc.slices(scene).items():
        none, some = int((count[sl] == 0).sum()), int((count[sl] > 0).sum())
        if (scene, name) in ONE_SIDED:
            assert (none, some)[1 - ONE_SIDED[(scene, name)]] == 0 and none + some >= 48
        else:
            assert none > 0 and some > 0, (scene, name, none, some)
    probes = count[oc.slices(scene)["probes"]]
    over, most = PROBES_OVER_64.get(scene, (0, None))
    assert int((probes > 64).sum()) == over
    if most is not None:
        assert int(probes.max()) == most
    if scene in ("layers", "slivers", "torus", "duplicates"):
        assert probes.max() > 64
    # rows: ascending indices, padded, a mask per kept index
    kept = m.rows.index >= 0
    assert np.array_equal(kept.sum(axis=1), np.minimum(count, om.SLOTS))
    assert not (kept[:, 1:] & ~kept[:, :-1]).any()
    assert (m.rows.index[:, :-1][kept[:, 1:]] < m.rows.index[:, 1:][kept[:, 1:]]).all()
    assert (m.rows.mask[kept] != 0).all() and not m.rows.mask[~kept].any()
    # the walk and the loop both have work: regular and irregular queries, and among the irregular ones some that report
    reg = oc.regular(m.queries, bmin, bmax)
    assert reg.sum() >= 700 and (~reg).sum() >= 90 and (count[~reg] > 0).sum() >= 10
    # both halves of the mask occur alone
    masks = m.rows.mask[kept]
    assert ((masks & 7) == 0).any() and ((masks >> 3) == 0).any()


def test_the_torus_against_itself():
    v9 = cpc.scene("torus")[0]
    T = v9.shape[0]
    m = np.concatenate([om.masks(v9[lo:lo + 200], v9) for lo in range(0, T, 200)])
    count = (m != 0).sum(axis=1)
    assert set(count.tolist()) == {11, 12}
    assert not m.diagonal().any()
    assert np.array_equal(m.T, om.swap_halves(m))
    shared = np.zeros((T, T), dtype=np.int64)
    for a in range(3):
        for b in range(3):
            shared += (v9[:, None, a, :] == v9[None, :, b, :]).all(axis=-1)
    assert (shared == 1).sum() == 14400 and (m[shared == 1] != 0).all()
    assert (shared == 2).sum() == 4800 and 4700 <= (m[shared == 2] != 0).sum() <= 4800
    assert not m[shared == 0].any() and (np.flatnonzero(shared == 3) == np.flatnonzero(np.eye(T, dtype=bool))).all()


def test_duplicates_never_report_their_copies():
    v9 = cpc.scene("duplicates")[0]
    T = v9.shape[0]
    m = om.masks(v9, v9)
    copies = (v9[:, None] == v9[None, :]).all(axis=(2, 3))
    assert (copies.sum(axis=1) >= 2).sum() >= 100                         # there are copies
    assert not m[copies].any()
    assert (m != 0).any()


def test_rows_of_k_cut_the_model_rows():
    m = oc.model("small")
    for k in oc.KS:
        r = m.want(k)
        assert {key: r[key].shape for key in om.KEYS} == om.shapes(m.queries.shape[0], k)
        assert all(r[key].dtype == om.NP_TYPES[key] for key in om.KEYS)
        assert np.array_equal((r["index"] >= 0).sum(axis=1), np.minimum(r["count"], k))
    assert np.array_equal(m.any()["count"], (m.rows.count > 0).astype(np.uint32))


# ---- (b) the header on the host ----
# (the sanitizers' runtimes are linked statically: the program must start whatever else the loader has been told to load first)
SANITIZED = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g")


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("overlap") / "tri_overlap_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", *SANITIZED, "-o", exe, os.path.join(ROOT, "tests", "cpp", "tri_overlap_check.cpp")])
    return exe


@pytest.mark.parametrize("scene", oc.SCENES)
def test_the_header_equals_the_model(check_program, tmp_path, scene):
    m = oc.model(scene)
    v9 = cpc.scene(scene)[0]
    n, T = m.queries.shape[0], v9.shape[0]
    path, out = str(tmp_path / "queries.bin"), str(tmp_path / "out.bin")
    oc.write_check_file(path, v9, m.queries)
    r = subprocess.run([check_program, path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, dtype=np.uint8)
    want_all = np.concatenate([om.masks(m.queries[lo:lo + om.CHUNK], v9) for lo in range(0, n, om.CHUNK)])
    assert om.same_bits(raw[:n * T].reshape(n, T), want_all), np.argwhere(raw[:n * T].reshape(n, T) != want_all)[:4]
    at = n * T
    for order in ("ascending", "descending"):
        for k in (1, 4, 64):
            want = m.want(k)
            for key in om.KEYS:
                size = want[key].size * want[key].itemsize
                got = raw[at:at + size].view(om.NP_TYPES[key]).reshape(want[key].shape)
                assert om.same_bits(got, want[key]), (order, k, key, np.argwhere(got != want[key])[:4])
                at += size
    assert at == raw.size
