"""CPU model of the colour light field with quad-linear interpolation (LightFieldColorMethod.Interpolate, LightFieldColorMethod.cs:142-181;
sr_set_light_field_interpolation), on top of tests/lightfield_model.py, which keeps the table and fills its cells.

  F      = RayToFloat4D (LightField4D.cs:214-245) = (u * (2N), v * N, s * (2N), t * N); u, v, s, t and the sphere test as for the nearest lookup
  b_k    = (byte)F_k (truncate, & 255, NaN -> 0);  frac_k = F_k - b_k
  for du, dv, ds, dt in {0, 1} (du outermost, dt innermost):
      c   = entry of cell ((b_u + du) % 2N, (b_v + dv) % N, (b_s + ds) % 2N, (b_t + dt) % N), an empty one filled first
      acc = acc + ((((byte(c) / 255.0) * wu) * wv) * ws) * wt     per channel; w = frac for offset 1, 1 - frac for offset 0; acc from 0
  sample = 0xFF000000 | (byte)(r * 255.0) << 16 | (byte)(g * 255.0) << 8 | (byte)(b * 255.0)

The blend TAKES the coordinates F as input.  Where the 16 entries are equal, acc * 255 lands within rounding of an integer, and one ulp in atan2 /
asin flips the byte: numpy's angles cannot reproduce a device frame bit for bit, the device's own coordinates (sr_light_field_coords) can.
`float4d` is numpy's RayToFloat4D, for the CPU-side figures and for checking the device's coordinates on their own.  Every line of `blend` is
one IEEE operation per element, in the order above.
"""
import math

import numpy as np

import lightfield_model as lfm
import pathtrace_model as ptm


def float4d(starts, dirs, n):
    """numpy's RayToFloat4D: (F [m, 4] -- 0 for a line that misses --, inside [m] bool, term [m])."""
    inv = 1.0 / np.sqrt((dirs[:, 0] * dirs[:, 0] + dirs[:, 1] * dirs[:, 1]) + dirs[:, 2] * dirs[:, 2])
    d = dirs * inv[:, None]
    proj = (starts[:, 0] * d[:, 0] + starts[:, 1] * d[:, 1]) + starts[:, 2] * d[:, 2]
    dist2 = (starts[:, 0] * starts[:, 0] + starts[:, 1] * starts[:, 1]) + starts[:, 2] * starts[:, 2]
    term = proj * proj - dist2 + lfm.RADIUS * lfm.RADIUS
    inside = ~(term < lfm.EPSILON)
    F = np.zeros((starts.shape[0], 4))
    k = np.nonzero(inside)[0]
    if k.size:
        root = np.sqrt(term[k])
        with np.errstate(invalid="ignore"):
            for j, frac in enumerate((-proj[k] - root, -proj[k] + root)):
                p = starts[k] + d[k] * frac[:, None]
                F[k, 2 * j] = (np.arctan2(p[:, 0], p[:, 2]) / math.pi * 0.5 + 0.5) * (n * 2)
                F[k, 2 * j + 1] = (np.arcsin(p[:, 1] / lfm.RADIUS) / math.pi + 0.5) * n
    return F, inside, term


def base_cells(coords):
    """(byte)F_k as int64 [m, 4]."""
    return lfm._to_byte(coords)


def wrap_counts(coords, inside, n):
    """Per axis (u, v, s, t): the samples inside the sphere whose upper neighbour wraps, (b_k + 1) % res_k != b_k + 1."""
    b = base_cells(coords)[inside]
    res = np.array([2 * n, n, 2 * n, n], dtype=np.int64)
    return [int(np.count_nonzero(b[:, k] + 1 >= res[k])) for k in range(4)]


def neighbour_cells(coords, n):
    """Table indices of the 16 cells of every sample, [m, 16], column du * 8 + dv * 4 + ds * 2 + dt."""
    b = base_cells(coords)
    out = np.zeros((coords.shape[0], 16), dtype=np.int64)
    for k in range(16):
        u = (b[:, 0] + (k >> 3 & 1)) % (2 * n)
        v = (b[:, 1] + (k >> 2 & 1)) % n
        s = (b[:, 2] + (k >> 1 & 1)) % (2 * n)
        t = (b[:, 3] + (k & 1)) % n
        out[:, k] = u * n * n * n * 2 + v * n * n * 2 + s * n + t
    return out


def blend(coords, entries):
    """Sample colours (uint32 [m]) of coordinates [m, 4] and their 16 entries (uint32 [m, 16]); also the largest channel value x * 255."""
    frac = coords - base_cells(coords).astype(np.float64)
    one_minus = 1 - frac
    acc = [np.zeros(coords.shape[0]) for _ in range(3)]
    for k in range(16):
        wu = frac[:, 0] if k & 8 else one_minus[:, 0]
        wv = frac[:, 1] if k & 4 else one_minus[:, 1]
        ws = frac[:, 2] if k & 2 else one_minus[:, 2]
        wt = frac[:, 3] if k & 1 else one_minus[:, 3]
        c = entries[:, k].astype(np.int64)
        for ch, shift in enumerate((16, 8, 0)):
            x = ((c >> shift) & 255).astype(np.float64) / 255.0
            x = x * wu
            x = x * wv
            x = x * ws
            x = x * wt
            acc[ch] = acc[ch] + x
    scaled = [a * 255.0 for a in acc]
    r, g, b = (lfm._to_byte(x) for x in scaled)
    color = (0xFF000000 | (r << 16) | (g << 8) | b).astype(np.uint32)
    lo = min(float(x.min()) for x in scaled) if coords.shape[0] else 0.0
    hi = max(float(x.max()) for x in scaled) if coords.shape[0] else 0.0
    return color, lo, hi


class LightFieldInterpModel:
    """LightFieldColorMethod with Interpolate = true over `table`, a lfm.LightFieldModel (or its shadowed subclass): the table, its fills and its
    running state are the nearest lookup's."""

    def __init__(self, table):
        self.table = table
        self.n = table.n
        self.filled = np.zeros(0, dtype=np.int64)        # indices the last frame filled, ascending
        self.touched = np.zeros(0, dtype=np.int64)       # indices the last frame read, ascending
        self.channel_range = (0.0, 0.0)                  # of x * 255 over the last frame's samples and channels
        self.coord_max = 0.0

    def sample_colors(self, scene, f, coords, inside, target=lfm.TRACE_ROOT_TREE):
        coords = np.asarray(coords, dtype=np.float64).reshape(-1, 4)
        inside = np.asarray(inside, dtype=bool)
        col = np.full(inside.size, (f.background_argb | 0xFF000000) & 0xFFFFFFFF, dtype=np.uint32)
        self.filled = self.touched = np.zeros(0, dtype=np.int64)
        self.channel_range, self.coord_max = (0.0, 0.0), 0.0
        if not inside.any():
            return col
        F = coords[inside]
        self.coord_max = float(np.nanmax(F))
        cells = neighbour_cells(F, self.n)
        self.touched = np.unique(cells)
        self.filled = np.array([c for c in self.touched.tolist() if c not in self.table.cache], dtype=np.int64)
        if self.filled.size:
            self.table.fill(scene, f, self.filled, target)
        values = self.table.entries(self.touched)
        col[inside], lo, hi = blend(F, values[np.searchsorted(self.touched, cells)])
        self.channel_range = (lo, hi)
        return col

    def render(self, scene, f, coords, inside, target=lfm.TRACE_ROOT_TREE):
        """The rows start_row..end_row as ARGB [rows, width]; coords / inside: RayToFloat4D of ptm.camera_samples(f), in that order."""
        W, n = f.width, f.sub_pixel_res
        col = self.sample_colors(scene, f, coords, inside, target)
        if n == 1:
            return col.reshape(-1, W)
        c = col.reshape(-1, n * n).astype(np.int64)
        r = ((c >> 16) & 255).sum(1) // (n * n)
        g = ((c >> 8) & 255).sum(1) // (n * n)
        bl = (c & 255).sum(1) // (n * n)
        return (0xFF000000 | (r << 16) | (g << 8) | bl).astype(np.uint32).reshape(-1, W)

    def conditions_hold(self):
        """The inputs for which colours and tables are pinned: every F_k < 256, every channel value x * 255 in [0, 256)."""
        return self.coord_max < 256.0 and 0.0 <= self.channel_range[0] and self.channel_range[1] < 256.0


# ---- the frames tests/test_gpu_lightfield_interp.py renders: name -> (model file, extra geometry, N, frame) ----
POSE_UP = dict(pitch_deg=80.0, yaw_deg=200.0, depth=3.0)
POSE_DOWN = dict(pitch_deg=-80.0, yaw_deg=200.0, depth=3.0)
# per frame: samples inside the sphere and the wraps per axis (u, v, s, t) that must be there, None = not pinned; from numpy's coordinates
REQUIRED = {
    "contention": dict(wraps=(None, None, 20650, None), s_at_2n=True),
    "unit_cube": dict(wraps=(13, None, None, None)),
    "far_primitives": dict(misses=True),
    "pose_up": dict(inside=1701, samples=3072, wraps=(152, None, 238, 538)),
    "pose_down": dict(wraps=(None, 1196, None, None)),
    "blur_x2": dict(),
}


def gpu_frames():
    from helpers import make_frame
    out = {name: lfm.gpu_frame(name) for name in ("contention", "unit_cube", "far_primitives")}
    out["pose_up"] = ("obj.3ds", (), 4, lfm.lf_frame(make_frame(64, 48, **POSE_UP)))
    out["pose_down"] = ("obj.3ds", (), 4, lfm.lf_frame(make_frame(64, 48, **POSE_DOWN)))
    out["blur_x2"] = ("obj2.3DS", (), 8, lfm.lf_frame(make_frame(64, 48, focal_blur=True, sub_pixel_res=2)))
    return out


def frame_figures(name):
    """numpy's view of a frame: (coords, inside, term, wraps per axis)."""
    _, _, n, f = gpu_frames()[name]
    coords, inside, term = float4d(*ptm.camera_samples(f), n)
    return coords, inside, term, wrap_counts(coords, inside, n)
