"""CPU model and ray sets of sr_light_field_rays: LightFieldColorMethod.IntersectRay for lines the caller supplies.  The model is
tests/lightfield_model.py's -- sample_cells for the cell of a line, LightFieldModel.fill (or its shadowed subclass's) for an empty entry --
applied to given rays instead of a frame's camera samples; with interpolation it is LightFieldInterpModel.sample_colors fed with the
device's coordinates (sr_light_field_coords), as for an interpolating frame.

The tests are bit-exact.  The only tolerance is the input condition of the light-field tests: the device's atan2 / asin may differ from
numpy's by ulps, so a ray is compared only when
  * every scaled coordinate lies at least lightfield_model.MARGIN from an integer (a NaN coordinate counts as clear: cell 0 on both sides), and
  * |term - 1e-10| >= MARGIN (a NaN term counts as clear: "term < 1e-10" is false on both sides, and the coordinates are NaN).
`usable` removes the other rays from a set on the CPU before any call; tests/test_lightfield_rays_model.py caps what it may remove.
"""
import math

import numpy as np

import lightfield_interp_model as lim
import lightfield_model as lfm
import pathtrace_model as ptm
import softray_amd as sa

RESOLUTIONS = (2, 3, 4, 8, 16, 64)
SEED = 20261020
PANORAMA_EYE = (0.11, -0.07, 0.23)


# ---- the ray sets ----
def segments(count=20000):
    """`count` segments between points uniform in [-1.5, 1.5]^3: about half pierce the sphere."""
    rng = np.random.default_rng(SEED)
    a = rng.uniform(-1.5, 1.5, (count, 3))
    b = rng.uniform(-1.5, 1.5, (count, 3))
    return np.ascontiguousarray(a), np.ascontiguousarray(b - a)


def panorama(width=128, height=64, eye=PANORAMA_EYE):
    """An equirectangular panorama from `eye`, row-major: every line pierces the sphere (the eye is inside)."""
    i, j = np.meshgrid(np.arange(width), np.arange(height))
    T = (i.reshape(-1) + 0.5) / width * (2 * math.pi)
    P = ((j.reshape(-1) + 0.5) / height - 0.5) * math.pi
    dirs = np.stack([np.sin(T) * np.cos(P), np.sin(P), np.cos(T) * np.cos(P)], axis=1)
    starts = np.tile(np.array(eye, dtype=np.float64), (dirs.shape[0], 1))
    return np.ascontiguousarray(starts), np.ascontiguousarray(dirs)


def camera(name):
    """The camera samples of a lightfield_model.GPU_FRAMES entry: (N, frame, starts, dirs)."""
    _, _, n, f = lfm.gpu_frame(name)
    starts, dirs = ptm.camera_samples(f)
    return n, f, np.ascontiguousarray(starts), np.ascontiguousarray(dirs)


SPECIALS = (0.0, float("nan"), float("inf"), float("-inf"), 1e300, 1e-300, -1e300)


def irregular():
    """Eight ordinary segments, each with one component of the start or of the direction replaced by every special value in turn."""
    a, d = segments(8)
    starts, dirs = [], []
    for k in range(a.shape[0]):
        for comp in range(6):
            for x in SPECIALS:
                s, e = a[k].copy(), d[k].copy()
                (s if comp < 3 else e)[comp % 3] = x
                starts.append(s)
                dirs.append(e)
    return np.ascontiguousarray(np.array(starts)), np.ascontiguousarray(np.array(dirs))


# ---- the input condition, per ray ----
def ray_margins(starts, dirs, n):
    """Per ray: the smallest distance of a scaled coordinate of the nearest lookup from an integer (inf: none -- a miss, or NaN coordinates) and
    |term - 1e-10| (inf for a NaN term).  lightfield_model.sample_cells' arithmetic, kept per ray."""
    with np.errstate(all="ignore"):
        inv = 1.0 / np.sqrt((dirs[:, 0] * dirs[:, 0] + dirs[:, 1] * dirs[:, 1]) + dirs[:, 2] * dirs[:, 2])
        d = dirs * inv[:, None]
        proj = (starts[:, 0] * d[:, 0] + starts[:, 1] * d[:, 1]) + starts[:, 2] * d[:, 2]
        dist2 = (starts[:, 0] * starts[:, 0] + starts[:, 1] * starts[:, 1]) + starts[:, 2] * starts[:, 2]
        term = proj * proj - dist2 + lfm.RADIUS * lfm.RADIUS
        inside = ~(term < lfm.EPSILON)
        term_margin = np.where(np.isnan(term), np.inf, np.abs(term - lfm.EPSILON))
        coord_margin = np.full(starts.shape[0], np.inf)
        root = np.sqrt(np.where(inside, term, 0.0))
        for frac in (-proj - root, -proj + root):
            p = starts + d * frac[:, None]
            h = np.arctan2(p[:, 0], p[:, 2])
            w = np.arcsin(p[:, 1] / lfm.RADIUS)
            for c in ((h / math.pi * 0.5 + 0.5) * (n * 2 - 1), (w / math.pi + 0.5) * (n - 1)):
                m = np.where(np.isnan(c), np.inf, np.abs(c - np.rint(c)))
                coord_margin = np.where(inside, np.minimum(coord_margin, m), coord_margin)
    return coord_margin, term_margin, inside


def usable(starts, dirs, resolutions):
    """(starts, dirs, removed): the rays that meet the input condition at every resolution of `resolutions`.  N = 1 needs none: every line
    inside the sphere is cell 0 -- but the sphere test's threshold still applies."""
    keep = np.ones(starts.shape[0], dtype=bool)
    for n in resolutions:
        cm, tm, _ = ray_margins(starts, dirs, n)
        keep &= tm >= lfm.MARGIN
        if n > 1:
            keep &= cm >= lfm.MARGIN
    return np.ascontiguousarray(starts[keep]), np.ascontiguousarray(dirs[keep]), int((~keep).sum())


def cells(starts, dirs, n):
    """lightfield_model.sample_cells' index per ray (-1: the line misses the sphere)."""
    with np.errstate(all="ignore"):
        return lfm.sample_cells(starts, dirs, n)[0]


# ---- the model ----
class LightFieldRaysModel:
    """sr_light_field_rays over `table`, a lfm.LightFieldModel (or its shadowed subclass): the table and its fills are the frame's."""

    def __init__(self, table):
        self.table = table
        self.n = table.n
        self.filled = np.zeros(0, dtype=np.int64)        # indices the last call filled, ascending
        self.touched = np.zeros(0, dtype=np.int64)       # indices the last call read, ascending

    def background(self, f):
        return (f.background_argb | 0xFF000000) & 0xFFFFFFFF

    def rays(self, scene, f, starts, dirs, target=lfm.TRACE_ROOT_TREE):
        """(out uint32 [m], inside uint8 [m], filled) of the nearest lookup."""
        starts = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
        dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
        idx = cells(starts, dirs, self.n)
        col = np.full(idx.size, self.background(f), dtype=np.uint32)
        inside = idx >= 0
        self.touched = np.unique(idx[inside])
        self.filled = np.array([c for c in self.touched.tolist() if c not in self.table.cache], dtype=np.int64)
        if self.filled.size:
            self.table.fill(scene, f, self.filled, target)
        if self.touched.size:
            values = self.table.entries(self.touched)
            col[inside] = values[np.searchsorted(self.touched, idx[inside])]
        return col, inside.astype(np.uint8), int(self.filled.size)

    def rays_interpolated(self, scene, f, coords, inside, target=lfm.TRACE_ROOT_TREE):
        """(out, filled) of the quad-linear blend; coords / inside: RayToFloat4D of the rays as the device computes it."""
        m = lim.LightFieldInterpModel(self.table)
        col = m.sample_colors(scene, f, coords, inside, target)
        self.filled, self.touched = m.filled, m.touched
        return col, int(m.filled.size)

    def traced(self):
        """Canonical rays the last call traced: one per cell filled, none for a NaN ray (N = 1)."""
        if not self.filled.size:
            return 0
        u, v, s, t = lfm.decode(self.filled, self.n)
        start = self.table.points[u, v]
        d = self.table.points[s, t] - start
        return int((~np.isnan(start.sum(axis=1) + d.sum(axis=1))).sum())


def resolve(col, f):
    """The integer resolve of a frame's sample colours: ARGB [rows, width]."""
    W, n = f.width, f.sub_pixel_res
    if n == 1:
        return col.reshape(-1, W)
    c = col.reshape(-1, n * n).astype(np.int64)
    r = ((c >> 16) & 255).sum(1) // (n * n)
    g = ((c >> 8) & 255).sum(1) // (n * n)
    bl = (c & 255).sum(1) // (n * n)
    return (0xFF000000 | (r << 16) | (g << 8) | bl).astype(np.uint32).reshape(-1, W)


# ---- what the call refuses after its arguments, with the whole message of sr_last_error: changes to a good frame, each SR_ERR_UNSUPPORTED ----
MESSAGES = [
    (dict(flags=sa._lib.F_AMBIENT_OCCLUSION), "sr_light_field_rays: ambient occlusion (SR_F_AMBIENT_OCCLUSION) needs a surface point per ray; a cell stores a colour"),
    (dict(flags=sa._lib.F_PATH_TRACING), "sr_light_field_rays: path tracing (SR_F_PATH_TRACING) needs a surface point per ray; a cell stores a colour"),
    (dict(flags=sa._lib.F_VOXELS), "sr_light_field_rays: voxel rendering (SR_F_VOXELS) replaces the root geometry the canonical rays are traced through"),
    (dict(flags=sa._lib.F_SINGLE_KERNEL), "sr_light_field_rays: the light field is not built into the one-kernel renderer (SR_F_SINGLE_KERNEL)"),
    (dict(max_bounces=1), "sr_light_field_rays: mirror bounces (max_bounces > 0) need a surface point per ray; a cell stores a colour"),
    (dict(strip_rows=16, strip_count=2, strip_index=0), "sr_light_field_rays: row strips (strip_count > 0) divide a frame's rows, not a batch of rays"),
]
TRIANGLES_MESSAGE = ("sr_light_field_rays: the triangle light field (sr_set_light_field_triangles) runs LightFieldTriMethod's three stages per ray, "
                     "which is not part of this call")
SHADOWS_MESSAGE = "light field together with shadows (dynamic or static) is not supported (a cell stores a colour, not a surface point)"


def changed(good, **kw):
    f = sa.Frame.from_buffer_copy(bytes(good))
    f.flags |= kw.pop("flags", 0)
    for k, v in kw.items():
        setattr(f, k, v)
    return f
