"""The structured meshes of tests/mesh_cases.py are not vacuous, shown with the CPU oracle alone: each tree builds, the 117 x 91 frame
at the scene's pose has between 10 % and 90 % hit pixels, the 17-sample soft-shadow frame has fully lit, partly shadowed and fully
shadowed hit pixels, and the property the class is built for holds -- (probe point, other triangle) pairs with G0 and K0 near zero at
ten times the soup's rate or more, records in each special class of edge_on's three lights with hit points lit through them, rays at
vertices and edge midpoints that land on an incident triangle.  The thresholds are conditions on the cases, not measurements of the library.

Figures found (117 x 91, 17 samples; triangles / hit pixels / fully lit, penumbra, fully shadowed / near pairs per hit point):
    terrain     8192 / 3416 / 2930  389   97 / 1.119        torus       9216 / 3014 / 2520  214  280 / 0.846
    fine       11520 / 4524 / 2366  235 1923 / 1.387        slivers     2178 / 2754 / 2093  464  197 / 3.190
    room        4014 / 6627 / 2330 3586  711 / 0.280        room_flush  4014 / 6466 / 2210 3564  692 / 0.287
    edge_on     7204 / 5212 / 2228  615 2369 / 0.282
The control, unit_cube_scene(6000), has 0.0184 near pairs per hit point at the default pose (108 over 5876), 0.0196 at terrain's, 0.0192 at
the room's, 0.0190 at edge_on's: the meshes have 14 to 170 times as many.  `fine`: 2822 hit points on the torus, 1702 on the shell's inside;
all 2822 probe points lie within the tolerance of a shell triangle's plane.
edge_on's lights (records with |GL| <= R, with an edge line through the ball, with GL == 0; hit points lit through the class's plates):
    in_plane  2880  635  720;   980 of 5212        straddle  3600 1487    0;  3990        pierced  2880 1789    0;  3694
Rays at vertices / edge midpoints that land on an incident triangle, brute force | nearest hit, and the cracks (misses) of both:
    terrain, outside, 4096 vertices 2986 | 3163, cracks 757 | 581; 4096 edges 3168 | 3335, cracks 573 | 403
    terrain, centre,  4096 vertices 2865 | 2865, cracks  13 |  13; 4096 edges 2991 | 2991, cracks 354 | 354
    torus, outside, 2048 vertices 1501 | 1609, cracks 483 | 375; 2048 edges 1675 | 1773, cracks 307 | 212
    torus, centre,  2048 vertices 1632 | 1632, cracks  23 |  23; 2048 edges 1813 | 1813, cracks 235 | 235
    room, outside, 1024 vertices 609 | 629, 1024 edges 666 | 699; centre, 640 | 640, 854 | 854; no cracks"""
import numpy as np
import pytest

import mesh_cases as mc
from ao_model import modulate
from helpers import camera_rays, orc

NCPU = 8
RES = (117, 91)
SAMPLES = 17
BACKGROUND = 0xff00ff
FACTOR = 10.0                               # near pairs per hit point: mesh >= FACTOR x soup
MIN_RECORDS, MIN_LIT_THROUGH = 8, 50
_ORACLES, _CONTROL = {}, {}


def oracle_scene(name):
    if name not in _ORACLES:
        o = orc.Scene()
        o.set_triangles(*(mc.soup_control() if name == "soup" else mc.scene(name)))
        assert o.build_tree() == 0, name
        _ORACLES[name] = o
    return _ORACLES[name]


def frames(name, **kw):
    """(lit, hard, soft): shadows off, the hard shadows of a zero table, the soft shadows of the scene's table."""
    o = oracle_scene(name)
    table, zeros = mc.offset_table(name, SAMPLES), mc.offset_table(name, SAMPLES, zero=True)
    lit, _ = o.render(mc.frame(name, *RES, **kw), threads=NCPU)
    hard, _ = o.render(mc.frame(name, *RES, table=zeros, shadows=True, shadow_samples=SAMPLES, **kw), threads=NCPU)
    soft, _ = o.render(mc.frame(name, *RES, table=table, shadows=True, shadow_samples=SAMPLES, **kw), threads=NCPU)
    return lit, hard, soft


@pytest.mark.parametrize("name", mc.NAMES)
def test_scene_is_not_vacuous(name):
    v9 = mc.scene(name)[0]
    lit, hard, soft = frames(name)
    hit = (lit & 0xFFFFFF) != BACKGROUND
    white = modulate(lit, 255)                                          # what ShadowMethod leaves of a pixel all of whose samples escape
    full = hit & (soft == hard) & (hard == white)
    umbra = hit & (soft == hard) & (hard != white)                      # as dark as the hard shadow: no sample escapes
    penumbra = hit & (soft != hard)
    print("%-10s triangles %5d hit %5d of %d lit %5d penumbra %5d shadowed %5d" % (name, len(v9), hit.sum(), hit.size, full.sum(), penumbra.sum(), umbra.sum()))
    assert 0.1 * hit.size <= hit.sum() <= 0.9 * hit.size, (name, int(hit.sum()))
    assert full.sum() > 0 and penumbra.sum() > 0 and umbra.sum() > 0, (name, int(full.sum()), int(penumbra.sum()), int(umbra.sum()))


@pytest.mark.parametrize("name", mc.NAMES)
def test_near_pairs_are_ten_times_the_soups(name):
    """The soup is rendered at the mesh's own pose (scenes that share a pose share the control's figure).  `fine` has its pairs from the
    shell that lies one probe offset around the torus: the tolerance scales with the box, the probe offset does not."""
    pairs, points = mc.near_pairs(name, oracle_scene(name), mc.frame(name, *RES))
    pose = tuple(sorted(mc.SCENES[name]["pose"].items()))
    if pose not in _CONTROL:
        _CONTROL[pose] = mc.near_pairs(mc.soup_control(), oracle_scene("soup"), mc.make_frame(*RES, **dict(pose)))
    cpairs, cpoints = _CONTROL[pose]
    print("%-10s near pairs %6d over %5d hit points = %.4f each; soup %5d over %5d = %.4f each" % (name, pairs, points, pairs / points, cpairs, cpoints, cpairs / cpoints))
    assert points > 0 and cpoints > 500 and cpairs > 0
    assert pairs / points >= FACTOR * (cpairs / cpoints), (name, pairs / points, cpairs / cpoints)


def test_fine_probe_points_land_in_the_shell():
    """Every probe point of a hit on the scaled torus lies within the near-pair tolerance of the plane of a shell triangle, and most lie
    over one: G0 ~ 0 against triangles several of the torus's edges away from the surface the point left."""
    v9, _, lo, hi = mc.scene("fine")
    torus = 2 * 96 * 48
    assert len(v9) == torus + 2 * mc.SHELL_MAJOR * mc.SHELL_MINOR
    pos, nrm, tri = mc.camera_hits(oracle_scene("fine"), mc.frame("fine", *RES))
    on_torus = tri < torus
    probe = (pos + mc.PROBE_OFFSET * nrm)[on_torus]
    n = mc.face_normals(v9[torus:])
    g = np.abs(probe @ n.T - (n * v9[torus:, 0]).sum(axis=1)[None, :]).min(axis=1)
    tol = mc.NEAR_TOL * float((hi - lo).max())
    print("fine: hits on the torus %d, on the shell's inside %d; probe points within the tolerance of a shell plane %d" % (on_torus.sum(), (~on_torus).sum(), (g <= tol).sum()))
    assert on_torus.sum() >= 2000 and (g <= tol).all()


def test_fine_is_finer_than_the_probe_offset():
    v9 = mc.scene("fine")[0][:2 * 96 * 48]                               # (the torus; the shell's cells are twice as wide)
    edges = np.sqrt(((v9 - np.roll(v9, 1, axis=1)) ** 2).sum(axis=2))
    print("fine: edges %.3g .. %.3g" % (edges.min(), edges.max()))
    assert edges.max() < 0.5 * mc.PROBE_OFFSET
    assert np.array_equal(mc.scene("torus")[0] * mc.FINE, v9[:2 * 96 * 48])


def test_shared_vertices_are_bit_equal():
    """Every scene but the comb and the plates is one vertex array indexed by faces: terrain's x and z are multiples of 2^-7, the torus is
    closed (every edge has exactly two faces, one in each direction)."""
    v9 = mc.scene("terrain")[0]
    xz = v9[:, :, (0, 2)] * 128.0
    assert np.array_equal(xz, np.round(xz)) and np.ptp(v9[:, :, 0]) == 0.875 and len(v9) == 2 * 64 * 64
    for v9 in (mc.scene("torus")[0], mc.scene("fine")[0][:2 * 96 * 48]):
        verts, idx = mc.mesh_vertices(v9)
        assert len(verts) == 96 * 48 and len(idx) == 2 * 96 * 48
        directed = np.concatenate([idx[:, (0, 1)], idx[:, (1, 2)], idx[:, (2, 0)]])
        assert len(np.unique(directed, axis=0)) == len(directed)                    # no directed edge twice: consistent orientation
        assert np.array_equal(np.unique(directed, axis=0), np.unique(directed[:, ::-1], axis=0))      # ... and each has its opposite: closed


def test_orientation_is_consistent():
    n = mc.face_normals(mc.scene("terrain")[0])
    assert (n[:, 1] > 0.0).all()
    v9 = mc.scene("room")[0]
    walls = v9[:10]
    assert ((mc.face_normals(walls) * (0.0 - walls.mean(axis=1))).sum(axis=1) > 0.0).all()          # inward
    for name in ("room", "room_flush"):
        edges = np.sqrt(((mc.scene(name)[0] - np.roll(mc.scene(name)[0], 1, axis=1)) ** 2).sum(axis=2))
        print(name, "edges %.3g .. %.3g" % (edges.min(), edges.max()))
        assert edges.min() < 2e-3 and edges.max() > 0.96
    flush = mc.scene("room_flush")[0][:10]
    assert (np.abs(flush) == 0.5).any(axis=2).all()                                 # every wall vertex lies on the root box


def test_slivers_keep_their_records():
    """The fan's triangles are 1000 times as long as high and still far above make_slab's needle rule; the comb's blades are thinner than
    a pixel's footprint at the pose."""
    v9 = mc.scene("slivers")[0]
    fan = v9[2:2 + mc.FAN_N]
    assert np.array_equal(fan[:, 0], np.broadcast_to(fan[0, 0], (mc.FAN_N, 3)))     # one centre vertex (whichever corner order)
    n = np.cross(v9[:, 1] - v9[:, 0], v9[:, 2] - v9[:, 0])
    nl = np.sqrt((n * n).sum(axis=1))
    edges = np.sqrt(((v9 - np.roll(v9, 1, axis=1)) ** 2).sum(axis=2))
    emax = edges.max(axis=1)
    aspect = emax * emax / nl                                                       # longest edge / the height over it
    print("slivers: fan aspect %.0f .. %.0f, |n| %.3g .. %.3g" % (aspect[2:2 + mc.FAN_N].min(), aspect[2:2 + mc.FAN_N].max(), nl.min(), nl.max()))
    assert aspect[2:2 + mc.FAN_N].min() >= 1000.0
    assert (np.abs(n).max(axis=1) >= mc.SLAB_ZERO_NORMAL).all() and (nl > mc.SLAB_NEEDLE * emax * emax).all()
    f = mc.frame("slivers", *RES)
    footprint = f.position_z / f.fov_depth / RES[0]
    blades = v9[2 + mc.FAN_N:]
    assert len(blades) == 2 * mc.COMB_N and np.sqrt(2.0) * mc.COMB_WIDTH < 0.5 * footprint


def test_edge_on_camera_lies_in_the_central_planes():
    f = mc.frame("edge_on", *RES)
    start, dirs = camera_rays(f)
    assert start[0] == 0.0 and start[1] == 0.0 and start[2] < -0.5
    v9 = mc.scene("edge_on")[0]
    n = np.cross(v9[:, 1] - v9[:, 0], v9[:, 2] - v9[:, 0])
    g1 = (n * (start - v9[:, 0])).sum(axis=1)
    assert (g1 == 0.0).sum() == 4 * mc.PLATES_PER_PLANE                             # the plates of x = 0 and y = 0, two triangles each
    f2 = mc.frame("edge_on", 96, 80)                                                # an even frame has a pixel column and a row through the centre
    _, d2 = camera_rays(f2)
    assert (d2[:, 0] == 0.0).sum() == 80 and (d2[:, 1] == 0.0).sum() == 96         # ... whose rays travel in those planes


@pytest.mark.parametrize("which", sorted(mc.EDGE_ON_LIGHTS))
def test_edge_on_lights(which):
    light = np.array(mc.EDGE_ON_LIGHTS[which])
    v9 = mc.scene("edge_on")[0]
    table = mc.offset_table("edge_on", SAMPLES)
    f = mc.frame("edge_on", *RES, light_model=light)
    assert np.array_equal(mc.light_model_of(f)[:2], light[:2])                      # (the pose's rotation is the identity: x and y arrive exactly)
    planes, pierced, exact = mc.light_classes(v9, light, mc.TABLE_RADIUS)
    plates = np.arange(len(v9)) >= 4                                                # (not the floor and the wall)
    cls = {"in_plane": exact, "straddle": planes & plates, "pierced": pierced & plates}[which]
    pos, nrm, _ = mc.camera_hits(oracle_scene("edge_on"), f)
    through = mc.lit_through(v9, cls, light, table, pos, nrm)
    print("%-8s |GL| <= R %2d, pierced %2d, GL == 0 %2d; class records %2d, hit points lit through them %d of %d" %
          (which, planes.sum(), pierced.sum(), exact.sum(), cls.sum(), through, len(pos)))
    assert (exact.sum() >= MIN_RECORDS) == (which == "in_plane")
    assert planes.sum() >= MIN_RECORDS and pierced.sum() >= (MIN_RECORDS if which == "pierced" else 0)
    assert cls.sum() >= MIN_RECORDS and through >= MIN_LIT_THROUGH
    lit, hard, soft = frames("edge_on", light_model=light)
    hit = (lit & 0xFFFFFF) != BACKGROUND
    assert (hit & (soft != hard)).sum() > 0


@pytest.mark.parametrize("name", sorted(mc.VERTEX_RAY_CASES))
def test_vertex_rays_hit_incident_triangles(name):
    """The scenes, counts and both origins tests/test_gpu_meshes.py traces: from each, half of the rays or more land on a triangle incident
    to the vertex / edge they aim at, in brute-force and in nearest-hit mode; the cracks are printed."""
    count = mc.VERTEX_RAY_CASES[name]
    for label, origin in zip(("outside", "centre"), mc.outside_origin(name)):
        fig = mc.tied_vertex_rays(name, origin, count, oracle_scene(name))
        for half in ("vertex", "edge"):
            brute, nearest, crack_b, crack_n, m = fig[half]
            print("%-8s %-7s %-6s rays %4d incident %4d | %4d cracks %3d | %3d" % (name, label, half, m, brute, nearest, crack_b, crack_n))
            assert m == count
            assert 2 * brute >= m and 2 * nearest >= m, (name, label, half, fig[half])
