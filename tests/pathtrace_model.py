"""CPU model of the reference's path tracing (PathTracingMethod.cs, Renderer.cs:1613-1618, 1700-1829), composed only of what the
oracle already exports: Scene.trace (one ray -> nearest hit), Random (System.Random) and shade_points (ShadingMethod's colour step).

For every camera sample that hits, in scan order (row, column, subX, subY) inside its row block:
  k        = hitting samples before it in the block; every block restarts Random(random_seed) (Renderer.cs:1655-1666, 1693)
  d        = (2 u[3k] - 1, 2 u[3k+1] - 1, 2 u[3k+2] - 1), negated when d . n < 0, normalised (multiply by 1 / length)
  incoming = colour of the nearest hit of the ray (pos + n * 0.001, d) through the same geometry, black on a miss
  out      = incoming * (n . d) + own colour, normalised when a channel exceeds 1.0, bytes by truncation
Misses draw nothing and keep the background.  Sub-pixel samples are averaged per channel with a truncating divide.
"""
import numpy as np

from helpers import orc

F_PATH_TRACING = 1 << 6                      # SR_F_PATH_TRACING (include/softray.h)
TRACE_ROOT_TREE = 2                          # Scene.trace target: extra geometry + the reference tree (SR_MODE_REF_TREE frames)
TRACE_NEAREST = 3                            # ... the global nearest triangle hit (the own BVH's semantics; no extra geometry)


def _mul3(it, x, y, z):
    """Instance.TransformDirection: row r = x * m[r][0] + y * m[r][1] + z * m[r][2], left to right."""
    return np.stack([x * it[r, 0] + y * it[r, 1] + z * it[r, 2] for r in range(3)], axis=-1)


def camera_samples(f):
    """Origins and directions of every camera sample of the frame's rows start_row..end_row in scan order (Renderer.cs:1717-1790):
    arrays [rows * width * n * n, 3]."""
    it = np.array([f.inv_transform[i] for i in range(12)]).reshape(3, 4)[:, :3]
    W, H, n = f.width, f.height, f.sub_pixel_res
    a = min(max(0, f.start_row), H - 1)
    b = min(max(0, f.end_row), H - 1)
    asp = H / W
    start0 = _mul3(it, np.float64(0.0), np.float64(0.0), np.float64(-f.position_z))
    rows, cols = np.mgrid[a:b + 1, 0:W]
    rows = rows.reshape(-1).astype(np.float64)
    cols = cols.reshape(-1).astype(np.float64)
    npx = rows.size
    if n == 1:
        d = _mul3(it, -(cols / W - 0.5), -(rows / H - 0.5) * asp, np.full(npx, f.fov_depth))
        return np.broadcast_to(start0, (npx, 3)).copy(), d
    sub = np.arange(n, dtype=np.float64) / (n - 1) - 0.5
    fx = np.repeat(sub, n)                                           # subX outer, subY inner (:1761-1763)
    fy = np.tile(sub, n)
    if f.flags & orc.F_FOCAL_BLUR:
        dv = _mul3(it, -(cols / W - 0.5), -(rows / H - 0.5) * asp, np.full(npx, f.fov_depth))
        focal = dv * f.focal_depth + start0                          # [npx, 3]
        s = _mul3(it, fx / W * f.focal_blur_strength, fy / H * f.focal_blur_strength, np.full(n * n, -f.position_z))   # [n2, 3]
        starts = np.broadcast_to(s[None, :, :], (npx, n * n, 3))
        dirs = focal[:, None, :] - starts
        return starts.reshape(-1, 3).copy(), dirs.reshape(-1, 3)
    cx = -((cols[:, None] + fx[None, :]) / W - 0.5)
    cy = -((rows[:, None] + fy[None, :]) / H - 0.5) * asp
    d = _mul3(it, cx.reshape(-1), cy.reshape(-1), np.full(npx * n * n, f.fov_depth))
    return np.broadcast_to(start0, (npx * n * n, 3)).copy(), d


def _unpack(c):
    c = c.astype(np.uint32)
    return np.stack([((c >> 16) & 255) / 255.0, ((c >> 8) & 255) / 255.0, (c & 255) / 255.0], axis=-1)


def hit_indices(hit, row_samples, num_rows, concurrency):
    """k of every sample: the exclusive count of hits inside its row block (Renderer.cs:1655-1666)."""
    conc = concurrency if concurrency > 0 else 4
    block_height = (num_rows - 1 + conc) // conc
    block = (np.arange(hit.size) // row_samples) // block_height
    idx = np.zeros(hit.size, dtype=np.int64)
    for b in np.unique(block):
        m = block == b
        idx[m] = np.cumsum(hit[m]) - hit[m]
    return idx


def sample_colors(scene, f, target=TRACE_ROOT_TREE):
    """ARGB of every camera sample (scan order) of the path-traced frame `f`."""
    W, H, n = f.width, f.height, f.sub_pixel_res
    a = min(max(0, f.start_row), H - 1)
    b = min(max(0, f.end_row), H - 1)
    starts, dirs = camera_samples(f)
    first = scene.trace(target, starts, dirs)
    hit = first["hit"].astype(bool)
    col = np.full(hit.size, (f.background_argb | 0xFF000000) & 0xFFFFFFFF, dtype=np.uint32)
    hi = np.nonzero(hit)[0]
    if hi.size == 0:
        return col
    idx = hit_indices(hit.astype(np.int64), W * n * n, b - a + 1, f.concurrency)
    u = orc.Random(f.random_seed).NextDoubles(3 * (int(idx[hi].max()) + 1)).reshape(-1, 3)
    nrm, pos = first["normal"][hi], first["pos"][hi]
    own = first["color"][hi]
    if f.flags & orc.F_SHADING:
        own = orc.shade_points(f, pos, nrm, own)
    d = u[idx[hi]] * 2 - 1
    dn = (d[:, 0] * nrm[:, 0] + d[:, 1] * nrm[:, 1]) + d[:, 2] * nrm[:, 2]
    d = np.where((dn < 0)[:, None], -d, d)
    inv = 1.0 / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    d = d * inv[:, None]
    second = scene.trace(target, pos + nrm * 0.001, d)
    hit2 = second["hit"].astype(bool)
    c2 = second["color"]
    if f.flags & orc.F_SHADING:
        c2 = orc.shade_points(f, second["pos"], second["normal"], c2)
    incoming = np.where(hit2[:, None], _unpack(c2), 0.0)
    frac = (nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1]) + nrm[:, 2] * d[:, 2]
    out = incoming * frac[:, None] + _unpack(own)
    big = (out > 1.0).any(axis=1)
    il = 1.0 / np.sqrt((out[:, 0] * out[:, 0] + out[:, 1] * out[:, 1]) + out[:, 2] * out[:, 2])
    out = np.where(big[:, None], out * il[:, None], out)
    by = (out * 255.0).astype(np.int64) & 255
    col[hi] = (0xFF000000 | (by[:, 0] << 16) | (by[:, 1] << 8) | by[:, 2]).astype(np.uint32)
    return col


def render(scene, f, target=TRACE_ROOT_TREE):
    """The rows start_row..end_row of the path-traced frame as ARGB [rows, width] (alpha 0xFF)."""
    W, n = f.width, f.sub_pixel_res
    col = sample_colors(scene, f, target)
    if n == 1:
        return col.reshape(-1, W)
    c = col.reshape(-1, n * n).astype(np.int64)
    r = ((c >> 16) & 255).sum(1) // (n * n)
    g = ((c >> 8) & 255).sum(1) // (n * n)
    bl = (c & 255).sum(1) // (n * n)
    return (0xFF000000 | (r << 16) | (g << 8) | bl).astype(np.uint32).reshape(-1, W)


# ---- the reference's two scenes (RendererTests.cs:247-281) ----
TRIANGLE_GOLDENS = [("pathTracing_noShading", {}),
                    ("pathTracing_noShading_2xAA", dict(sub_pixel_res=2)),
                    ("pathTracing_noShading_4xAA", dict(sub_pixel_res=4)),
                    ("pathTracing_noShading_8xAA", dict(sub_pixel_res=8)),
                    ("pathTracing_noShading_focalBlurx2", dict(focal_blur=True, sub_pixel_res=2, focal_depth=1.0)),
                    ("pathTracing_noShading_focalBlurx4", dict(focal_blur=True, sub_pixel_res=4, focal_depth=1.0)),
                    ("pathTracing_noShading_focalBlurx8", dict(focal_blur=True, sub_pixel_res=8, focal_depth=1.0))]
SPHERE_GOLDENS = [("pathTracing_noShading_6_geometry", dict(depth=3.0)),
                  ("pathTracing_noShading_focalBlurx4_7_geometry", dict(depth=3.0, focal_blur=True, sub_pixel_res=4, focal_depth=2.5)),
                  ("pathTracing_noShading_focalBlurx8_8_geometry", dict(depth=3.0, focal_blur=True, sub_pixel_res=8, focal_depth=2.5))]
_A = 0xFF000000
PRIMITIVES = [(0, _A | 0xFFFFFF, [0.0, -10000.0, 0.0, 9999.5]), (0, _A | 0xFF0000, [-0.5, 0.0, -0.5, 0.5]), (0, _A | 0x00FF00, [0.5, 0.0, 0.5, 0.5]),
              (0, _A | 0x0000FF, [0.5, 0.0, -0.5, 0.5]), (0, _A | 0xFFFF00, [-0.5, 0.0, 0.5, 0.5])]
