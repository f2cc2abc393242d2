"""CPU model of the reference's colour light field (rayTraceLightField with LightFieldStoresTriangles = false: LightFieldColorMethod.cs:92-217,
LightField4D.cs:175-206, 253-273, 304-344, Sphere.cs:69-142), composed only of what the oracle already exports:
pathtrace_model.camera_samples, Scene.trace (one ray -> nearest hit) and shade_points (ShadingMethod's colour step).

For every camera sample (model space; sphere of radius 0.866 about the origin):
  d     = dir * (1.0 / |dir|);  proj = start . d;  term = proj * proj - start . start + R * R;  term < 1e-10 -> the background colour
  p1,p2 = start + d * (-proj -/+ sqrt(term));  h = atan2(p.x, p.z), w = asin(p.y / R) (not clamped)
  u,v,s,t = h1 / pi * 0.5 + 0.5, w1 / pi + 0.5, h2 / pi * 0.5 + 0.5, w2 / pi + 0.5
  cell  = ((byte)(u * (2N - 1)), (byte)(v * (N - 1)), (byte)(s * (2N - 1)), (byte)(t * (N - 1))), a NaN coordinate -> 0
  index = u * N * N * N * 2 + v * N * N * 2 + s * N + t   into 4 N^4 uint32 entries, 0 = empty
An empty entry is filled with the colour of the cell's CANONICAL ray -- from P(u, v) towards P(s, t), the centres of the two sphere
patches -- traced through the frame's root geometry and shaded as the frame says (the background on a miss; a colour 0 is stored as 1).
Within a frame the colour of a cell is therefore a function of the cell alone: which sample fills it, and in which order, does not
matter (a shaded colour also carries the pose and lights of the frame that filled the cell).  The model keeps the
cache between calls, as a Renderer does, sparsely (a dict), so that N = 128 needs no 4 GiB.
"""
import math

import numpy as np

import pathtrace_model as ptm
from helpers import orc

F_LIGHT_FIELD = 1 << 15                      # SR_F_LIGHT_FIELD (include/softray.h)
RADIUS = 0.866                               # LightField4D's bounding sphere
EPSILON = 1e-10                              # Sphere.IntersectLine
TRACE_ROOT_TREE, TRACE_NEAREST = ptm.TRACE_ROOT_TREE, ptm.TRACE_NEAREST


def cache_entries(n):
    return 4 * n ** 4


def sphere_points(n):
    """P(i, j) for i < 2N, j < N as [2N, N, 3] (Coord4DToRay + Sphere.ConvertLine): math.sin / math.cos, one value at a time."""
    p = np.zeros((2 * n, n, 3))
    max_h, max_w = float(2 * n - 1), float(n - 1)
    for i in range(2 * n):
        h = ((i + 0.5) / max_h - 0.5) * math.pi * 2 if max_h else float("nan")
        for j in range(n):
            w = ((j + 0.5) / max_w - 0.5) * math.pi if max_w else float("nan")
            horiz = math.cos(w) * RADIUS
            p[i, j] = (math.sin(h) * horiz, math.sin(w) * RADIUS, math.cos(h) * horiz)
    return p


def _to_byte(x):
    """(byte) of a double that is in range by construction; NaN -> 0."""
    x = np.where(np.isnan(x), 0.0, x)
    return x.astype(np.int64) & 255


def _margin(x):
    """Distance of every scaled coordinate from the nearest integer (NaN: none)."""
    x = x[~np.isnan(x)]
    return float(np.abs(x - np.rint(x)).min()) if x.size else float("inf")


def sample_cells(starts, dirs, n):
    """Cache index of every sample (-1: it misses the sphere), the smallest coordinate margin and the smallest |term - 1e-10|."""
    inv = 1.0 / np.sqrt((dirs[:, 0] * dirs[:, 0] + dirs[:, 1] * dirs[:, 1]) + dirs[:, 2] * dirs[:, 2])
    d = dirs * inv[:, None]
    proj = (starts[:, 0] * d[:, 0] + starts[:, 1] * d[:, 1]) + starts[:, 2] * d[:, 2]
    dist2 = (starts[:, 0] * starts[:, 0] + starts[:, 1] * starts[:, 1]) + starts[:, 2] * starts[:, 2]
    term = proj * proj - dist2 + RADIUS * RADIUS
    inside = ~(term < EPSILON)
    term_margin = float(np.abs(term - EPSILON).min()) if term.size else float("inf")
    idx = np.full(starts.shape[0], -1, dtype=np.int64)
    k = np.nonzero(inside)[0]
    if k.size == 0:
        return idx, float("inf"), term_margin
    root = np.sqrt(term[k])
    coords = []
    with np.errstate(invalid="ignore"):
        for frac in (-proj[k] - root, -proj[k] + root):
            p = starts[k] + d[k] * frac[:, None]
            h = np.arctan2(p[:, 0], p[:, 2])
            w = np.arcsin(p[:, 1] / RADIUS)
            coords += [(h / math.pi * 0.5 + 0.5) * (n * 2 - 1), (w / math.pi + 0.5) * (n - 1)]
    u, v, s, t = (_to_byte(c) for c in coords)
    idx[k] = u * n * n * n * 2 + v * n * n * 2 + s * n + t
    return idx, min(_margin(c) for c in coords), term_margin


def decode(index, n):
    """(u, v, s, t) of cache indices: the index is injective for coordinates in range (u, s < 2N; v, t < N)."""
    index = np.asarray(index, dtype=np.int64)
    return index // (2 * n ** 3), (index // (2 * n * n)) % n, (index // n) % (2 * n), index % n


class LightFieldModel:
    """One Renderer's LightFieldColorMethod at resolution `n`: the cache lives as long as the object."""

    def __init__(self, n=64):
        self.n = n
        self.cache = {}                # index -> colour (never 0)
        self.points = sphere_points(n)
        self.filled = np.zeros(0, dtype=np.int64)       # indices the last frame filled, ascending
        self.coord_margin = float("inf")                # of the last frame
        self.term_margin = float("inf")

    def reset(self):
        self.cache = {}

    def dense(self):
        out = np.zeros(cache_entries(self.n), dtype=np.uint32)
        if self.cache:
            out[np.fromiter(self.cache.keys(), dtype=np.int64)] = np.fromiter(self.cache.values(), dtype=np.uint32)
        return out

    def entries(self, index):
        return np.array([self.cache.get(int(i), 0) for i in index], dtype=np.uint32)

    def fill(self, scene, f, index, target):
        u, v, s, t = decode(index, self.n)
        start = self.points[u, v]
        dirs = self.points[s, t] - start
        res = scene.trace(target, np.ascontiguousarray(start), np.ascontiguousarray(dirs))
        hit = res["hit"].astype(bool)
        col = np.full(index.size, (f.background_argb | 0xFF000000) & 0xFFFFFFFF, dtype=np.uint32)
        if hit.any():
            own = res["color"][hit]
            if f.flags & orc.F_SHADING:
                own = orc.shade_points(f, res["pos"][hit], res["normal"][hit], own)
            col[hit] = own
        col[col == 0] = 1
        for i, c in zip(index.tolist(), col.tolist()):
            self.cache[i] = c

    def sample_colors(self, scene, f, target=TRACE_ROOT_TREE):
        starts, dirs = ptm.camera_samples(f)
        idx, self.coord_margin, self.term_margin = sample_cells(starts, dirs, self.n)
        col = np.full(idx.size, (f.background_argb | 0xFF000000) & 0xFFFFFFFF, dtype=np.uint32)
        inside = idx >= 0
        cells = np.unique(idx[inside])
        self.filled = np.array([c for c in cells.tolist() if c not in self.cache], dtype=np.int64)
        if self.filled.size:
            self.fill(scene, f, self.filled, target)
        if cells.size:
            values = self.entries(cells)
            col[inside] = values[np.searchsorted(cells, idx[inside])]
        return col

    def render(self, scene, f, target=TRACE_ROOT_TREE):
        """The rows start_row..end_row of the frame as ARGB [rows, width] (alpha 0xFF after the resolve of sub-pixel samples)."""
        W, n = f.width, f.sub_pixel_res
        col = self.sample_colors(scene, f, target)
        if n == 1:
            return col.reshape(-1, W)
        c = col.reshape(-1, n * n).astype(np.int64)
        r = ((c >> 16) & 255).sum(1) // (n * n)
        g = ((c >> 8) & 255).sum(1) // (n * n)
        bl = (c & 255).sum(1) // (n * n)
        return (0xFF000000 | (r << 16) | (g << 8) | bl).astype(np.uint32).reshape(-1, W)


def lf_frame(f):
    """`f` with the light-field bit OR-ed in."""
    f.flags |= F_LIGHT_FIELD
    return f


# ---- the reference's goldens that need neither shadows nor AO (RendererTests.cs:234-241, 100x100, obj.3ds) ----
GOLDENS = [("%s_lightFieldColor%s" % (shade, suffix), dict(shading=shade == "shading", **kw))
           for shade in ("noShading", "shading")
           for suffix, kw in (("", {}), ("_4xAA", dict(sub_pixel_res=4)), ("_focalBlurx2", dict(focal_blur=True, sub_pixel_res=2)),
                              ("_focalBlurx4", dict(focal_blur=True, sub_pixel_res=4)))]


# ---- the frames tests/test_gpu_lightfield.py renders: name -> (model file, extra geometry, N, width, height, make_frame keywords).  A frame
#      may be compared on the device only when no sample of it sits on a cell boundary or on the sphere test's threshold
#      (tests/test_lightfield_model.py checks both margins for every entry): above them the device's atan2 / asin cannot move a sample ----
POSES = [dict(), dict(yaw_deg=100.0, pitch_deg=-15.0), dict(yaw_deg=60.0, pitch_deg=20.0)]
GPU_FRAMES = {
    "contention": ("obj.3ds", (), 4, 64, 48, dict(sub_pixel_res=4)),
    "small_blur": ("obj2.3DS", (), 8, 64, 48, dict(focal_blur=True, sub_pixel_res=2)),
    "far": ("obj.3ds", (), 64, 37, 29, dict(depth=3.0)),
    "far_n16": ("obj.3ds", (), 16, 37, 29, dict(depth=3.0)),
    "far_primitives": ("obj.3ds", ptm.PRIMITIVES, 16, 37, 29, dict(depth=3.0, start_row=5, end_row=17)),
    "inside_sphere": ("obj.3ds", (), 64, 100, 100, dict(depth=0.6)),
    "res128": ("obj.3ds", (), 128, 50, 50, dict()),
    "res128_high": ("obj.3ds", (), 128, 50, 50, dict(yaw_deg=-45.0)),    # entries beyond 2^29: byte offsets beyond 2^31
    "unit_cube": ("unit_cube_2000", (), 32, 96, 64, dict(yaw_deg=25.0, pitch_deg=12.0, depth=1.6)),
}
for _i, _pose in enumerate(POSES):
    GPU_FRAMES["view%d_n64" % _i] = ("obj.3ds", (), 64, 100, 100, dict(_pose))
    GPU_FRAMES["view%d_n8" % _i] = ("obj.3ds", (), 8, 64, 48, dict(_pose, sub_pixel_res=2))
for _name, _kw in GOLDENS:
    GPU_FRAMES[_name] = ("obj.3ds", (), 64, 100, 100, dict(_kw))
MARGIN = 1e-9                                # both input conditions


def gpu_frame(name):
    """(model file, extra geometry, N, frame) of a GPU_FRAMES entry."""
    from helpers import make_frame
    model, prims, n, w, h, kw = GPU_FRAMES[name]
    return model, prims, n, lf_frame(make_frame(w, h, **kw))


# ---- what SR_F_LIGHT_FIELD is refused with (include/softray.h): changes to a light-field frame, each SR_ERR_UNSUPPORTED ----
REFUSED = [dict(flags=1 << 1), dict(flags=(1 << 1) | (1 << 5)),            # SR_F_SHADOWS, dynamic and static
           dict(flags=1 << 13), dict(flags=1 << 6), dict(flags=1 << 7),    # SR_F_AMBIENT_OCCLUSION, SR_F_PATH_TRACING, SR_F_VOXELS
           dict(max_bounces=1), dict(flags=1 << 8), dict(strips=(16, 2, 0))]   # mirror bounces, SR_F_SINGLE_KERNEL, caller-made strips


def apply_change(f, change):
    f.flags |= change.get("flags", 0)
    f.max_bounces = change.get("max_bounces", 0)
    if "strips" in change:
        f.strip_rows, f.strip_count, f.strip_index = change["strips"]
    return f
