"""Structured meshes (tests/test_mesh_cases.py on the CPU oracle alone, tests/test_gpu_meshes.py on the device): connected surfaces
with shared, bit-equal vertices, the geometry a host feeds the library, where every other scene of the suite is a soup of independent
triangles.  On a mesh the quantities the fast path's bounds are about come close to zero systematically: a hit point near a shared edge
has K0 ~ 0 for the neighbour, a tessellation finer than the 0.001 probe offset puts the probe point several triangles away, a camera or
a light can lie exactly in a triangle's plane, a ray at a vertex ties every incident triangle at one rayFrac.  Numpy and the oracle only:
no library calls are made here.

Every generator returns (v9 [n, 3, 3], argb, box_min, box_max), deterministic, a distinct colour per triangle (bvh_shapes.colours),
faces oriented consistently (the normal (v2 - v1) x (v3 - v1) points to the side the surface is seen from), exactly degenerate triangles
dropped."""
import math

import numpy as np

from bvh_shapes import colours
from helpers import camera_rays, make_frame, orc, unit_cube_scene

SEED = 1234567890                           # make_frame's random_seed: the offset table is derived from it
PROBE_OFFSET = 0.001                        # ShadowMethod's probe point: hit + 0.001 n
NEAR_TOL = 2.0e-3                           # near_pairs: x the box extent
TABLE_RADIUS = 0.2                          # |offset| of every entry of the area light's table (orc.area_light_offsets), at scale 1
SLAB_ZERO_NORMAL = 1e-10                    # make_slab (softray_amd/csrc/sr_lbvh.hip): every |component| of (v2 - v1) x (v3 - v1) below it: no record
SLAB_NEEDLE = 1e-12                         # ... and |n| <= 1e-12 x (longest edge)^2: no record
FINE = 1.0 / 64
TRACE_BRUTE, TRACE_TREE, TRACE_NEAREST = 0, 1, 3
UNIT_LO, UNIT_HI = np.array([-0.5] * 3), np.array([0.5] * 3)

# name: scale of the model (camera depth, light and offset table follow it as placement_cases does for `small`), camera pose at scale 1,
# model-space position of the point light at scale 1 (None: the frame's default light)
SCENES = {
    "terrain":    dict(s=1.0, pose=dict(yaw_deg=-60.0, pitch_deg=-30.0, depth=1.5), light=None),       # (the light stands in view space: from here the peak and the hills shadow the valleys before the camera)
    "torus":      dict(s=1.0, pose=dict(yaw_deg=135.0, pitch_deg=-22.0, depth=1.5), light=None),
    "fine":       dict(s=FINE, pose=dict(yaw_deg=135.0, pitch_deg=-22.0, depth=1.5), light=None),
    "room":       dict(s=1.0, pose=dict(yaw_deg=14.0, pitch_deg=-11.0, depth=1.25), light=(0.18, 0.3, 0.12)),
    "room_flush": dict(s=1.0, pose=dict(yaw_deg=14.0, pitch_deg=-11.0, depth=1.25), light=(0.18, 0.3, 0.12)),
    "slivers":    dict(s=1.0, pose=dict(yaw_deg=135.0, pitch_deg=-22.0, depth=1.5), light=None),
    "edge_on":    dict(s=1.0, pose=dict(yaw_deg=0.0, pitch_deg=0.0, depth=1.5), light=None),
}
NAMES = tuple(SCENES)
SCALE_ONE = tuple(n for n in NAMES if SCENES[n]["s"] == 1.0)
PLATE_STEP = 0.125                          # edge_on: plates at x = k / 8 and y = k / 8
# edge_on's three lights (model space).  The plates of x = 1/8 span y in [-5/16, 5/16], z in [-5/16, -1/32] and [1/32, 5/16].
EDGE_ON_LIGHTS = {
    "in_plane": (0.125, 0.40625, -0.4375),  # x equals the plane of the plates at x = 1/8: GL = 0 exactly
    "straddle": (0.171875, 0.28125, -0.4375),  # 3/64 from that plane, 5/64 from x = 1/4: the ball (radius 0.2) straddles both
    "pierced":  (0.15625, 0.34375, -0.1875),  # 1/32 from the plane and 1/32 above the plates' border edge y = 5/16: that edge line pierces the ball
}
# rays at vertices and edge midpoints: scene -> rays of each kind, from both origins of outside_origin (a closed surface shows an origin at
# most half of its vertices: the torus is asked for the 2048 that face it, the room for 1024)
VERTEX_RAY_CASES = {"terrain": 4096, "torus": 2048, "room": 1024}
_MADE = {}


# ---- meshes: (vertices [nv, 3], faces [nf, 3]) -> triangles ----
def _orient(tris, outward):
    """Flip the triangles whose normal points against `outward` [n, 3]; drop the exactly degenerate ones."""
    n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    keep = (n != 0.0).any(axis=1)
    tris, n, outward = tris[keep], n[keep], np.broadcast_to(outward, (keep.size, 3))[keep]
    flip = (n * outward).sum(axis=1) < 0.0
    tris[flip] = tris[flip][:, (0, 2, 1)]
    return tris


def _grid_faces(rows, cols, wrap_rows=False, wrap_cols=False):
    """Two triangles per cell of a rows x cols vertex grid (index r * cols + c); wrapped axes join the last row / column to the first:
    the seam's vertices are the same entries of the vertex array, not recomputed ones."""
    r, c = np.meshgrid(np.arange(rows if wrap_rows else rows - 1), np.arange(cols if wrap_cols else cols - 1), indexing="ij")
    r, c = r.ravel(), c.ravel()
    r1, c1 = (r + 1) % rows, (c + 1) % cols
    a, b, d, e = r * cols + c, r1 * cols + c, r1 * cols + c1, r * cols + c1
    return np.concatenate([np.stack([a, b, d], axis=1), np.stack([a, d, e], axis=1)])


def terrain_heights(x, z, second=False):
    """Smooth hills plus one narrow peak; `second`: the heights the refit test moves the mesh to (x and z stay)."""
    if second:
        return -0.22 + 0.11 * np.sin(7.0 * x - 0.4) * np.cos(5.0 * z + 0.2) + 0.05 * np.cos(11.0 * (x - z)) + 0.3 * np.exp(-((x + 0.12) ** 2 + (z - 0.1) ** 2) / 0.004)
    return -0.22 + 0.13 * np.sin(6.0 * x + 0.3) * np.cos(5.0 * z) + 0.05 * np.sin(13.0 * (x + z)) + 0.4 * np.exp(-((x - 0.08) ** 2 + (z + 0.06) ** 2) / 0.002)


def terrain(second=False):
    """A 64 x 64-cell height field, two triangles per cell, 0.875 of the box wide.  x and z are multiples of 2^-7: 48 cells are two such
    steps wide and every fourth is one step (48 x 2 + 16 = 112 steps = 0.875), so cells of three shapes share edges."""
    steps = np.concatenate([[0], np.cumsum(np.where(np.arange(64) % 4 == 3, 1, 2))])
    assert steps[-1] == 112
    axis = (steps - 56) / 128.0
    x, z = np.meshgrid(axis, axis, indexing="ij")
    verts = np.stack([x, terrain_heights(x, z, second), z], axis=-1).reshape(-1, 3)
    assert np.abs(verts).max() < 0.5
    tris = _orient(verts[_grid_faces(65, 65)], np.array([0.0, 1.0, 0.0]))
    return _pack(tris, UNIT_LO, UNIT_HI)


def _torus_tris(major=0.3, minor=0.12, n_major=96, n_minor=48):
    u = 2.0 * math.pi * np.arange(n_major) / n_major
    v = 2.0 * math.pi * np.arange(n_minor) / n_minor
    uu, vv = np.meshgrid(u, v, indexing="ij")
    ring = major + minor * np.cos(vv)
    verts = np.stack([ring * np.cos(uu), minor * np.sin(vv), ring * np.sin(uu)], axis=-1).reshape(-1, 3)
    tris = verts[_grid_faces(n_major, n_minor, True, True)]
    cen = tris.mean(axis=1)
    flat = np.sqrt(cen[:, 0] ** 2 + cen[:, 2] ** 2)
    core = np.stack([cen[:, 0] / flat * major, np.zeros(len(cen)), cen[:, 2] / flat * major], axis=1)     # the nearest point of the centre circle
    return _orient(tris, cen - core)


def torus():
    """A closed 96 x 48 torus about the y axis (R 0.3, r 0.12), concave: the inner ring is shadowed by the far side, and half of the
    surface faces away from the camera and from the light."""
    return _pack(_torus_tris(), UNIT_LO, UNIT_HI)


SHELL_MAJOR, SHELL_MINOR = 48, 24


def fine():
    """The torus and its box scaled by 1 / 64 (a power of two: exact): edges of 2e-4 .. 5e-4, below the 0.001 probe offset.  Around it, at the
    same scale, a concentric shell of 48 x 24 cells whose minor radius is larger by the probe offset (0.12 + 0.064 before scaling) and whose
    faces look inwards: from outside it does not show and stops no ray on the way in, and the probe point of every hit on the torus lands
    in the shell's surface -- within a few 1e-5 of the planes of shell triangles it has never touched, G0 ~ 0 for each."""
    shell = _torus_tris(0.3, 0.12 + PROBE_OFFSET / FINE, SHELL_MAJOR, SHELL_MINOR)[:, (0, 2, 1)]
    return _pack(np.concatenate([_torus_tris(), shell]) * FINE, UNIT_LO * FINE, UNIT_HI * FINE)


def _quad(p, du, dv, outward):
    """Two triangles of the parallelogram p, p + du, p + du + dv, p + dv, facing `outward`."""
    p, du, dv = np.asarray(p, dtype=np.float64), np.asarray(du, dtype=np.float64), np.asarray(dv, dtype=np.float64)
    q = np.array([[p, p + du, p + du + dv], [p, p + du + dv, p + dv]])
    return _orient(q, np.asarray(outward, dtype=np.float64))


def _box_tris(lo, hi):
    """The 12 triangles of an axis-aligned box, facing outwards."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        du, dv = np.zeros(3), np.zeros(3)
        du[b], dv[c] = hi[b] - lo[b], hi[c] - lo[c]
        for side, sign in ((lo, -1.0), (hi, 1.0)):
            p, n = lo.copy(), np.zeros(3)
            p[a], n[a] = side[a], sign
            out.append(_quad(p, du, dv, n))
    return np.concatenate(out)


def _sphere_tris(centre, radius, rings, segments):
    """A closed lat-long sphere, outward normals; the poles' degenerate halves are dropped."""
    th = math.pi * np.arange(rings + 1) / rings
    ph = 2.0 * math.pi * np.arange(segments) / segments
    tt, pp = np.meshgrid(th, ph, indexing="ij")
    st = np.sin(tt)
    st[0], st[-1] = 0.0, 0.0                # the poles: one point each, exactly
    verts = np.stack([radius * st * np.cos(pp), radius * np.cos(tt), radius * st * np.sin(pp)], axis=-1).reshape(-1, 3) + np.asarray(centre)
    tris = verts[_grid_faces(rings + 1, segments, False, True)]
    return _orient(tris, tris.mean(axis=1) - np.asarray(centre))


def room(inset=2.0 ** -6):
    """Five inward-facing walls of two triangles each (floor, ceiling, two sides and the wall z = -0.5 + inset), `inset` from the box
    faces, open at z = 0.5; inside three box pillars and a sphere of radius 0.1 tessellated 32 x 64.  Edges from 0.97 down to 1e-3 (at
    the sphere's poles; 1e-2 at its equator) in one tree.  The camera stands outside z = -0.5: triangles are one-sided, so the wall
    before it does not show, every other surface of the room does, and the open side shows the background.  (A box seen from outside
    fills its silhouette with its far walls: with the opening before the camera no pixel is background at any distance at which the
    sphere is more than a few pixels wide.)"""
    h = 0.5 - inset
    w = 2.0 * h
    parts = [_quad((-h, -h, -h), (w, 0, 0), (0, 0, w), (0, 1, 0)), _quad((-h, h, -h), (w, 0, 0), (0, 0, w), (0, -1, 0)),
             _quad((-h, -h, -h), (0, w, 0), (0, 0, w), (1, 0, 0)), _quad((h, -h, -h), (0, w, 0), (0, 0, w), (-1, 0, 0)),
             _quad((-h, -h, -h), (w, 0, 0), (0, w, 0), (0, 0, 1))]
    parts += [_box_tris((-0.34, -h, 0.05), (-0.22, 0.18, 0.17)), _box_tris((0.2, -h, 0.18), (0.3, 0.02, 0.28)), _box_tris((-0.06, -h, 0.26), (0.04, 0.3, 0.36))]
    parts.append(_sphere_tris((0.05, -0.04, -0.36), 0.1, 32, 64))
    return _pack(np.concatenate(parts), UNIT_LO, UNIT_HI)


def room_flush():
    """The room with its walls exactly on the box faces: no record of a wall is interior, and hit points lie on the root box."""
    return room(0.0)


FAN_N, FAN_STEP, FAN_RADIUS = 2048, 2.0 ** -11, 0.42
COMB_N, COMB_WIDTH = 64, 2.0 ** -11


def slivers():
    """A floor; above it a fan of 2048 triangles from one centre vertex -- an arc of 1 radian, each triangle 2^-11 radians wide: longest edge
    over height is above 1000 -- whose rim undulates, so that neighbours are not coplanar; and a comb of 64 upright blades 2^-11
    wide, thinner than a pixel's footprint at the pose (1.5 / fov depth / 117 = 0.0106)."""
    parts = [_quad((-0.45, -0.4, -0.45), (0.9, 0, 0), (0, 0, 0.9), (0, 1, 0))]
    ang = 0.5 * (math.pi - FAN_N * FAN_STEP) + FAN_STEP * np.arange(FAN_N + 1)
    apex = np.array([0.0, -0.12, -0.35])
    rim = apex + np.stack([FAN_RADIUS * np.cos(ang), 0.06 + 0.01 * np.sin(40.0 * ang), FAN_RADIUS * np.sin(ang)], axis=1)
    fan = np.stack([np.broadcast_to(apex, (FAN_N, 3)), rim[:-1], rim[1:]], axis=1)
    parts.append(_orient(fan.copy(), np.array([0.0, 1.0, 0.0])))
    toward_camera = np.array([-1.0, 0.3, 1.0])
    for k in range(COMB_N):
        x = -0.4 + k * (0.5 / COMB_N)
        parts.append(_quad((x, -0.4, 0.38 - 0.5 * (x + 0.4)), (COMB_WIDTH, 0, COMB_WIDTH), (0, 0.22 + 0.001 * k, 0), toward_camera))
    return _pack(np.concatenate(parts), UNIT_LO, UNIT_HI)


PLATE_SIDE = 0.03125                        # edge_on: every plate is a square of this side
PLATES_PER_PLANE = 20 * 18


def _tiles(p, du, dv, nu, nv, outward):
    """nu x nv square plates of two triangles each from corner p, sides du and dv: neighbours share bit-equal vertices (dyadic coordinates)."""
    p, du, dv = np.asarray(p, dtype=np.float64), np.asarray(du, dtype=np.float64), np.asarray(dv, dtype=np.float64)
    return np.concatenate([_quad(p + i * du + j * dv, du, dv, outward) for i in range(nu) for j in range(nv)])


def edge_on():
    """Axis-aligned square plates of side 1/32, two triangles each, tiling the planes x = k / 8 and y = k / 8, k = -2 .. 2, over 5/8 x (9/32
    + 9/32: z in [-5/16, -1/32] and [1/32, 5/16]), crossing each other, over a floor at y = -7/16 and before a wall at z = 7/16.  Each
    plate faces the axis x = y = 0 the camera stands on (the central ones +x / +y), so the camera sees the central plates exactly edge-on.
    Small plates put a border or a diagonal within reach of most hit points; the crossings alone are near 3 % of them."""
    a, z0, z1, d = 0.3125, 0.03125, 0.3125, PLATE_SIDE
    parts = [_quad((-0.4375, -0.4375, -0.4375), (0.875, 0, 0), (0, 0, 0.875), (0, 1, 0)), _quad((-0.4375, -0.4375, 0.4375), (0.875, 0, 0), (0, 0.875, 0), (0, 0, -1))]
    for k in range(-2, 3):
        c = k * PLATE_STEP
        face = -1.0 if k > 0 else 1.0
        for zs in (-z1, z0):
            parts.append(_tiles((c, -a, zs), (0, d, 0), (0, 0, d), 20, 9, (face, 0, 0)))
            parts.append(_tiles((-a, c, zs), (d, 0, 0), (0, 0, d), 20, 9, (0, face, 0)))
    return _pack(np.concatenate(parts), UNIT_LO, UNIT_HI)


def _pack(tris, lo, hi):
    v9 = np.ascontiguousarray(tris, dtype=np.float64)
    assert v9.shape[0] <= 12000 and (v9 >= lo).all() and (v9 <= hi).all()
    return v9, colours(v9.shape[0]), np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)


def scene(name):
    """(v9, argb, box_min, box_max) of the scene, made once; read-only."""
    if name not in _MADE:
        made = {"terrain": terrain, "torus": torus, "fine": fine, "room": room, "room_flush": room_flush, "slivers": slivers, "edge_on": edge_on}[name]()
        for a in made:
            a.setflags(write=False)
        _MADE[name] = made
    return _MADE[name]


# ---- frames: tests/placement_cases.py's rules ----
def pose(name):
    p = SCENES[name]
    return dict(p["pose"], depth=p["pose"]["depth"] * p["s"])


def offset_table(name, samples, zero=False):
    """The area light's offsets at the scene's scale (the caller keeps the array alive while a frame points at it)."""
    t = orc.area_light_offsets(SEED, samples) * SCENES[name]["s"]
    return np.ascontiguousarray(t * 0.0 if zero else t)


def set_light(f, light_model):
    """Put the point light at a model-space position, through the frame's transform."""
    t = [f.transform[i] for i in range(12)]
    m = light_model
    for r in range(3):
        f.light_pos_view[r] = t[4 * r] * m[0] + t[4 * r + 1] * m[1] + t[4 * r + 2] * m[2] + t[4 * r + 3]
    return f


def frame(name, w, h, table=None, light_model=None, **kw):
    """make_frame at the scene's pose, the light's position, the focal depth and the blur scaled with the model; `table`: the offset table
    of a soft-shadow frame (offset_table); `light_model`: a model-space position of the point light (default: the scene's, if it has one)."""
    f = make_frame(w, h, **dict(pose(name), **kw))
    s = SCENES[name]["s"]
    for i in range(3):
        f.light_pos_view[i] *= s
    f.focal_depth, f.focal_blur_strength = (SCENES[name]["pose"]["depth"] + 0.5) * s, 10.0 * s
    if light_model is None and SCENES[name]["light"] is not None:
        light_model = np.array(SCENES[name]["light"]) * s
    if light_model is not None:
        set_light(f, light_model)
    if table is not None:
        f.area_light_offsets = table.ctypes.data
    return f


def light_model_of(f):
    """The model-space position of the frame's point light."""
    t = np.array([f.transform[i] for i in range(12)]).reshape(3, 4)
    it = np.array([f.inv_transform[i] for i in range(12)]).reshape(3, 4)
    return it[:, :3] @ (np.array([f.light_pos_view[i] for i in range(3)]) - t[:, 3])


def light_inside(box_min, box_max):
    """A model-space light position inside the root box: centre + 0.1 x extent."""
    lo, hi = np.asarray(box_min), np.asarray(box_max)
    return 0.5 * (lo + hi) + 0.1 * (hi - lo)


# ---- vertices, rays at them ----
def mesh_vertices(v9):
    """(distinct vertices [nv, 3], index [n, 3] of every triangle corner in them): bit-equal corners are one vertex."""
    flat = np.ascontiguousarray(np.asarray(v9, dtype=np.float64).reshape(-1, 3)) + 0.0          # (-0.0 -> 0.0)
    verts, inv = np.unique(flat, axis=0, return_inverse=True)
    return verts, inv.reshape(-1, 3)


def face_normals(v9):
    n = np.cross(v9[:, 1] - v9[:, 0], v9[:, 2] - v9[:, 0])
    return n / np.sqrt((n * n).sum(axis=1))[:, None]


def vertex_points(name):
    """(pos [nv, 3], normal [nv, 3], colour [nv]): the distinct vertices of the mesh with the normalised sum of the unit normals of their
    incident faces, and a colour each -- what a host that lights a mesh per vertex hands to the point calls."""
    v9 = scene(name)[0]
    verts, idx = mesh_vertices(v9)
    fn = face_normals(v9)
    acc = np.zeros_like(verts)
    for k in range(3):
        np.add.at(acc, idx[:, k], fn)
    ln = np.sqrt((acc * acc).sum(axis=1))
    keep = ln > 1e-6                                                    # (plates that cross: opposite faces may cancel)
    return np.ascontiguousarray(verts[keep]), np.ascontiguousarray(acc[keep] / ln[keep, None]), colours(int(keep.sum()), first=20000)


def vertex_rays(name, origin, count):
    """FP64, unnormalised directions from `origin`: v - origin for `count` distinct mesh vertices (those whose vertex normal faces the
    origin first, evenly thinned), then 0.5 (v_a + v_b) - origin for as many distinct mesh edges.  Returns (dirs [2 m, 3], target [2 m, 2]:
    the vertex indices (a, a) or (a, b) into mesh_vertices, m = min(count, vertices, edges))."""
    v9 = scene(name)[0]
    origin = np.asarray(origin, dtype=np.float64)
    verts, idx = mesh_vertices(v9)
    fn = face_normals(v9)
    acc = np.zeros_like(verts)
    for k in range(3):
        np.add.at(acc, idx[:, k], fn)
    edges = np.unique(np.sort(np.concatenate([idx[:, (0, 1)], idx[:, (1, 2)], idx[:, (2, 0)]]), axis=1), axis=0)
    m = min(count, verts.shape[0], edges.shape[0])

    def pick(facing, m):
        order = np.concatenate([np.flatnonzero(facing), np.flatnonzero(~facing)])
        pool = order[:max(m, int(facing.sum()))]
        return pool[(np.arange(m) * pool.size) // m]

    vi = pick((acc * (origin - verts)).sum(axis=1) > 0.0, m)
    mid = 0.5 * (verts[edges[:, 0]] + verts[edges[:, 1]])
    ei = pick(((acc[edges[:, 0]] + acc[edges[:, 1]]) * (origin - mid)).sum(axis=1) > 0.0, m)
    dirs = np.concatenate([verts[vi] - origin, mid[ei] - origin])
    target = np.concatenate([np.stack([vi, vi], axis=1), edges[ei]])
    return np.ascontiguousarray(dirs), target


def outside_origin(name):
    """An origin outside the root box on all three axes (the camera's corner), and the box centre."""
    lo, hi = scene(name)[2:]
    c, e = 0.5 * (lo + hi), hi - lo
    return c + e * np.array([-0.9, 0.8, 1.1]), c


def tied_vertex_rays(name, origin, count, o=None):
    """Of the rays of vertex_rays, per half (vertices, edges): how many hit a triangle incident to the targeted vertex / edge in the oracle's
    brute-force mode and in its nearest-hit mode, and how many miss everything -- a crack; cracks are legal, the device must reproduce them.
    Returns dict(vertex=(brute, nearest, cracks_brute, cracks_nearest, m), edge=...)."""
    v9, argb, lo, hi = scene(name)
    if o is None:
        o = orc.Scene()
        o.set_triangles(v9, argb, lo, hi)
    dirs, target = vertex_rays(name, origin, count)
    _, idx = mesh_vertices(v9)
    starts = np.ascontiguousarray(np.tile(np.asarray(origin, dtype=np.float64), (dirs.shape[0], 1)))
    m = dirs.shape[0] // 2
    out = {}
    res = {t: o.trace(t, starts, dirs) for t in (TRACE_BRUTE, TRACE_NEAREST)}
    for half, rows in (("vertex", slice(0, m)), ("edge", slice(m, 2 * m))):
        fig = []
        for t in (TRACE_BRUTE, TRACE_NEAREST):
            hit = res[t]["hit"][rows].astype(bool)
            corners = idx[np.where(hit, res[t]["tri_index"][rows], 0)]
            tg = target[rows]
            incident = hit & (corners == tg[:, :1]).any(axis=1) & (corners == tg[:, 1:]).any(axis=1)
            fig += [int(incident.sum()), int((~hit).sum())]
        out[half] = (fig[0], fig[2], fig[1], fig[3], m)
    return out


# ---- predicates on the shadow stage's quantities ----
def camera_hits(o, f):
    """The oracle's nearest hits of the frame's one-sample-per-pixel camera rays: (pos, unit normal, tri_index) of the hit pixels."""
    start, dirs = camera_rays(f)
    hits = o.trace(TRACE_NEAREST, np.broadcast_to(start, dirs.shape), dirs)
    vis = hits["hit"] == 1
    return hits["pos"][vis], hits["normal"][vis], hits["tri_index"][vis]


def _records(v9):
    """Unit normal, and per edge k the in-plane unit normal pointing at the opposite vertex with its base point: make_slab's planes in FP64."""
    n = face_normals(v9)
    ms = []
    for k in range(3):
        p0, p1, p2 = v9[:, k], v9[:, (k + 1) % 3], v9[:, (k + 2) % 3]
        m = np.cross(n, p1 - p0)
        m /= np.sqrt((m * m).sum(axis=1))[:, None]
        m *= np.where((m * (p2 - p0)).sum(axis=1) < 0.0, -1.0, 1.0)[:, None]
        ms.append(m)
    return n, ms


def near_pairs(name_or_scene, o, f):
    """(pairs, hit points): over the camera hit points of the frame, the (probe point E' = hit + 0.001 n, other triangle) pairs with E' within
    NEAR_TOL x the box extent of the triangle's plane and inside all three edge planes widened by the same amount: the pairs whose G0 and
    K0_k the classification sees near zero."""
    v9, _, lo, hi = scene(name_or_scene) if isinstance(name_or_scene, str) else name_or_scene
    tol = NEAR_TOL * float((hi - lo).max())
    pos, nrm, tri = camera_hits(o, f)
    probe = pos + PROBE_OFFSET * nrm
    n, ms = _records(v9)
    d = (n * v9[:, 0]).sum(axis=1)
    pairs = 0
    for a in range(0, probe.shape[0], 2048):
        e = probe[a:a + 2048]
        g = e @ n.T - d[None, :]
        pi, ti = np.nonzero(np.abs(g) <= tol)
        keep = ti != tri[a:a + 2048][pi]
        pi, ti = pi[keep], ti[keep]
        inside = np.ones(pi.size, dtype=bool)
        for k in range(3):
            inside &= (ms[k][ti] * (e[pi] - v9[ti, k])).sum(axis=1) >= -tol
        pairs += int(inside.sum())
    return pairs, int(probe.shape[0])


def light_classes(v9, light, radius):
    """Per record, for the light ball (centre `light`, radius `radius`): (|GL| <= R: the ball straddles or touches the triangle's plane, an
    edge line with rho = sqrt(GL^2 + KL_k^2) <= R: it pierces the ball, GL == 0: the centre lies in the plane) -- the classes of DESIGN 5.2."""
    light = np.asarray(light, dtype=np.float64)
    n, ms = _records(v9)
    gl = (n * (light - v9[:, 0])).sum(axis=1)
    pierced = np.zeros(v9.shape[0], dtype=bool)
    for k in range(3):
        kl = (ms[k] * (light - v9[:, k])).sum(axis=1)
        pierced |= np.sqrt(gl * gl + kl * kl) <= radius
    return np.abs(gl) <= radius, pierced, gl == 0.0


def lit_through(v9, records, light, table, pos, nrm, reach=2.0 * TABLE_RADIUS, chunk=256):
    """How many of the surface points are lit through the given records (those of them whose centroid is within `reach` of the light):
    at least one of the table's sample rays (light + offset -> E') is stopped by one of them (one-sided, FP64, rayFrac in (0, 1]) and
    at least one passes them all."""
    light = np.asarray(light, dtype=np.float64)
    rec = np.flatnonzero(records & (np.sqrt(((v9.mean(axis=1) - light) ** 2).sum(axis=1)) <= reach))
    n = np.cross(v9[rec, 1] - v9[rec, 0], v9[rec, 2] - v9[rec, 0])
    count = 0
    for a in range(0, pos.shape[0], chunk):
        probe = pos[a:a + chunk] + PROBE_OFFSET * nrm[a:a + chunk]
        blocked = np.zeros(probe.shape[0], dtype=np.int64)
        for s in range(table.shape[0]):
            src = light + table[s]
            d = probe - src                                                         # [p, 3]
            den = d @ n.T                                                           # [p, r]
            num = ((v9[rec, 0] - src) * n).sum(axis=1)[None, :]
            with np.errstate(divide="ignore", invalid="ignore"):
                t = num / den
            pi, ri = np.nonzero((den < 0.0) & (t > 0.0) & (t <= 1.0))
            x = src[None, :] + t[pi, ri][:, None] * d[pi]
            ok = np.ones(pi.size, dtype=bool)
            for k in range(3):
                p0, p1 = v9[rec[ri], k], v9[rec[ri], (k + 1) % 3]
                ok &= (np.cross(p1 - p0, x - p0) * n[ri]).sum(axis=1) >= 0.0
            stopped = np.zeros(probe.shape[0], dtype=bool)
            stopped[pi[ok]] = True
            blocked += stopped
        count += int(((blocked > 0) & (blocked < table.shape[0])).sum())
    return count


def soup_control():
    """The control of near_pairs: the suite's usual soup."""
    return unit_cube_scene(6000)
