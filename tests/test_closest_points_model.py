"""The model of sr_closest_points (tests/closest_points_model.py) and the point sets of tests/closest_points_cases.py, pinned on the CPU: the
model's answers on a right triangle with power-of-two coordinates are the hand-computed ones for each of the seven regions; on random
triangles no point of a 64 x 64 barycentric sampling is nearer than the model's answer; the header routine
(softray_amd/csrc/sr_closest.h), built into a stand-alone host program with g++ -ffp-contract=off (and once more under the address and
undefined-behaviour sanitizers), equals the model bit for bit on the committed point file; and the sets hold what the GPU tests rely on."""
import os
import subprocess

import numpy as np
import pytest

import closest_points_cases as cpc
import closest_points_model as cpm
from helpers import GOLDEN, ROOT

TIE_SCENES = ("layers", "torus", "slivers", "duplicates")
RIGHT = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], dtype=np.float64)
# point, region, d2, closest point, (v, w): half a unit above the plane, every number exact in binary
BY_HAND = [
    ((-1, -1, .5), "A", 2.25, (0, 0, 0), (0, 0)),
    ((2, -.5, .5), "B", 1.5, (1, 0, 0), (1, 0)),
    ((-.5, 2, .5), "C", 1.5, (0, 1, 0), (0, 1)),
    ((.25, -1, .5), "AB", 1.25, (.25, 0, 0), (.25, 0)),
    ((-1, .75, .5), "AC", 1.25, (0, .75, 0), (0, .75)),
    ((1, 1, .5), "BC", .75, (.5, .5, 0), (.5, .5)),
    ((.25, .25, .5), "face", .25, (.25, .25, 0), (.25, .25)),
]


def test_the_seven_regions_by_hand():
    q = np.array([c[0] for c in BY_HAND], dtype=np.float64)
    c, v, w, region = cpm.closest_pairs(q, RIGHT)
    d2 = cpm.squared_distance(q, c)
    for i, (_, name, want_d2, pos, vw) in enumerate(BY_HAND):
        assert cpm.REGIONS[region[i, 0]] == name
        assert d2[i, 0] == want_d2 and tuple(c[i, 0]) == tuple(float(x) for x in pos) and (v[i, 0], w[i, 0]) == tuple(float(x) for x in vw), name
    a = cpm.Answers(q, RIGHT)
    assert (a.tri == 0).all() and cpm.same_bits(a.dist, np.sqrt(np.array([c[2] for c in BY_HAND])))
    # in a vertex region the point is the vertex itself, bit for bit, also where the coordinates are no round numbers
    t = np.array([[0.1, 0.2, 0.3, 1.1, 0.25, 0.35, 0.15, 1.3, 0.2]])
    far = np.array([(-5.0, -5.0, 0.3), (9.0, 0.25, 0.35), (0.15, 9.0, 0.2)])
    c, v, w, region = cpm.closest_pairs(far, t)
    assert list(region[:, 0]) == [0, 1, 2]
    assert cpm.same_bits(c[:, 0], t.reshape(3, 3))


def test_no_sampled_point_is_nearer_than_the_answer():
    rng = np.random.default_rng(99)
    tris = rng.uniform(-1.0, 1.0, size=(24, 9))
    pts = rng.uniform(-2.0, 2.0, size=(48, 3))
    c, v, w, region = cpm.closest_pairs(pts, tris)
    d2 = cpm.squared_distance(pts, c)
    g = np.arange(64) / 63.0
    gv, gw = (x.reshape(-1) for x in np.meshgrid(g, g, indexing="ij"))
    keep = gv + gw <= 1.0
    gv, gw = gv[keep], gw[keep]
    t = tris.reshape(-1, 3, 3)
    samples = t[:, None, 0] + (t[:, None, 1] - t[:, None, 0]) * gv[None, :, None] + (t[:, None, 2] - t[:, None, 0]) * gw[None, :, None]    # [T][S][3]
    diff = pts[:, None, None, :] - samples[None]
    sampled = (diff * diff).sum(axis=-1).min(axis=-1)                                        # [P][T]
    assert (d2 <= sampled * (1.0 + 1e-12)).all()
    assert (sampled <= d2 + 0.2).all()                                                       # (the sampling comes close: the answer is no far-off point)
    assert set(np.unique(region)) == set(range(7))
    assert (v >= 0).all() and (w >= 0).all() and (v + w <= 1.0 + 1e-15).all()


def build_check(tmp_path, flags=()):
    exe = str(tmp_path / ("closest_point_check" + ("_san" if flags else "")))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", *flags, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "closest_point_check.cpp")])
    return exe


# (the sanitizers' runtimes are linked statically: the program must start whatever else the loader has been told to load first)
SANITIZED = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g")


@pytest.mark.parametrize("flags", [(), SANITIZED], ids=["plain", "sanitized"])
def test_the_header_routine_equals_the_model(tmp_path, flags):
    """The stand-alone host program (its own main, nothing loaded into Python) against the model, every pair and every bit."""
    path = os.path.join(GOLDEN, cpc.CHECK_FILE)
    tris, pts = cpc.read_check_file(path)
    made_t, made_p = cpc.check_file_contents()
    assert cpm.same_bits(tris, made_t) and cpm.same_bits(pts, made_p)                       # the committed file is the one the cases module describes
    exe = build_check(tmp_path, flags)
    out = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.float64).reshape(pts.shape[0], tris.shape[0], 7)
    c, v, w, region = cpm.closest_pairs(pts, tris)
    d2 = cpm.squared_distance(pts, c)
    want = np.concatenate([region.astype(np.float64)[..., None], c, v[..., None], w[..., None], d2[..., None]], axis=-1)
    # NaN results agree in being NaN (the sign and payload of a NaN an operation makes are not pinned by IEEE 754), everything else in every bit
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w)
    assert cpm.same_bits(np.where(nan_g, 0.0, got), np.where(nan_w, 0.0, want))
    assert set(np.unique(region)) == set(range(7)) and nan_w[..., 6].any() and np.isinf(want[..., 6]).any()


@pytest.fixture(scope="module")
def answers():
    made = {}

    def get(scene):
        if scene not in made:
            made[scene] = cpm.Answers(cpc.points(scene), cpc.scene(scene)[0])
        return made[scene]
    return get


@pytest.mark.parametrize("scene", cpc.SCENES)
def test_what_the_sets_hold(answers, scene):
    v9, _, bmin, bmax = cpc.scene(scene)
    pts = cpc.points(scene)
    sl = cpc.slices(scene)
    a = answers(scene)
    assert pts.shape[0] <= 4096 and v9.shape[0] <= 2200
    reg = cpm.regular(pts, bmin, bmax)
    # every region is the answer for some regular point
    assert set(np.unique(a.region[reg & (a.tri >= 0)])) == set(range(7))
    # the vertices lie on the mesh
    assert (a.dist[sl["vertices"]] == 0.0).all() and (a.tri[sl["vertices"]] >= 0).all()
    # ties between different indices, where triangles share vertices or are there twice (a soup of random triangles has none)
    if scene in TIE_SCENES:
        assert a.ties[reg].sum() >= 50
    # the regular / irregular rule: 2^10, 2^19 and 2^18 diagonals walk, 2^21 and 2^40 do not, nor does any point of "irregular"
    far = reg[sl["far"]].reshape(len(cpc.FAR), -1)
    assert far[:3].all() and not far[3:].any() and not reg[sl["irregular"]].any()
    assert reg[sl["vertices"]].all() and reg[sl["offsets"]].all() and reg[sl["lattice"]].all() and reg[sl["between"]].all()
    # a NaN point has no answer; the other irregular points may have one
    assert (a.tri[sl["irregular"]][:3] == -1).all()
    # every limit kind produces both outcomes where it can
    lim, kind = cpc.limit_kinds(a.dist)
    out = a.outputs(lim)
    has = a.tri >= 0
    kept = out["tri_index"] >= 0
    for k, name in enumerate(cpc.LIMIT_KINDS):
        m = has & (kind == k)
        assert m.sum() > 50
        if name in ("inf", "exact", "double"):
            assert kept[m].all(), name
        elif name in ("nan", "-inf", "negative"):
            assert not kept[m].any(), name
        elif name == "zero":
            assert kept[m].any() and not kept[m].all()                                      # (kept: the points on the mesh)
            assert (a.dist[m & kept] == 0.0).all()
        else:                                                                                # one ulp below: cut (at distance 0 nextafter gives -5e-324, a negative limit)
            assert not kept[m].any()
    assert cpm.same_bits(a.outputs(None)["tri_index"], a.tri)


def test_a_nan_distance_is_skipped(answers):
    """On "degenerate" the triangles with vertex 1 == vertex 2 divide 0 by 0 for most points: skipped, and never the answer there."""
    v9, _, bmin, bmax = cpc.scene("degenerate")
    a = answers("degenerate")
    pts = cpc.points("degenerate")
    reg = cpm.regular(pts, bmin, bmax)
    assert ((a.nan_pairs > 0) & reg & (a.tri >= 0)).sum() > 1000
    c, v, w, region = cpm.closest_pairs(pts[reg][:256], v9[cpc.DEGENERATE_AT:])
    d2 = cpm.squared_distance(pts[reg][:256], c)
    assert np.isnan(d2[:, :2]).any() and not np.isnan(d2[:, 2]).any()
    assert (a.tri >= cpc.DEGENERATE_AT).sum() > 10                                           # an area-less triangle with a numeric distance can win


def test_duplicates_and_layers_tie():
    for scene in ("duplicates", "layers"):
        a = cpm.Answers(cpc.points(scene)[cpc.slices(scene)["between"]], cpc.scene(scene)[0])
        assert a.ties.sum() > 50, scene
