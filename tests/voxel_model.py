"""CPU model of the reference's voxel-grid rendering (rayTraceVoxels: Renderer.cs:1568-1588, TriMeshToVoxelGrid.cs, VoxelGrid.cs:125-177,
LineWalker3D.cs:17-35) in numpy, composed only of what exists already: the oracle's 3DS loader (through helpers), orc.shade_points
(ShadingMethod's colour step) and pathtrace_model.camera_samples (the camera rays).  FP64, operations in the order written.

Grid (64^3, cell (x,y,z) spans [k/64 - 0.5, (k+1)/64 - 0.5] per axis): triangle t is in a cell when on every axis max_vertex >= k/64 - 0.5
and min_vertex <= (k+1)/64 - 0.5; colour = sum of byte / 255.0 per channel over the cell's triangles in ascending index, / count, truncation
of c * 255.0, alpha 255 (0 = empty); normal = unit plane normal of the cell's lowest-index triangle.
Ray: end = start + dir * 10; clip to the box (-1,-1,-1)..(1,1,1) (ContainsPoint with +-1e-10); p = (p * 0.5 + 0.5) * 63.999; fixed steps of
0.1 along the longest axis with pos accumulated by repeated addition; the first cell (truncation of pos) with a non-zero colour is the hit
{colour, normal, pos = 0, rayFrac = 0}.
"""
import numpy as np

from helpers import orc
from pathtrace_model import camera_samples

F_VOXELS = 1 << 7                            # SR_F_VOXELS (include/softray.h)
TARGET_VOXELS = 0x200                        # SR_TARGET_VOXELS
G = 64
_PLANES = np.arange(G + 1, dtype=np.float64) / G - 0.5


def triangle_normals(v9):
    """Plane.Normal of Triangle(v1, v2, v3) (Triangle.cs:29-57, Plane.cs:25-27): unit((v2 - v1) x (v3 - v1)), multiply by 1 / length."""
    v9 = np.asarray(v9, dtype=np.float64).reshape(-1, 3, 3)
    e1, e2 = v9[:, 1] - v9[:, 0], v9[:, 2] - v9[:, 0]
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=-1)
    zero = (np.abs(n) < 1e-10).all(axis=1)
    n[zero] = (1.0, 0.0, 0.0)
    inv = 1.0 / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return n * inv[:, None]


def voxelise(v9, argb):
    """(colors uint32 [64,64,64], normals [64,64,64,3], stats) of TriMeshToVoxelGrid.Convert(triangles, 64)."""
    v9 = np.asarray(v9, dtype=np.float64).reshape(-1, 3, 3)
    argb = np.asarray(argb, dtype=np.uint32)
    n = v9.shape[0]
    mn, mx = v9.min(axis=1), v9.max(axis=1)
    lo = np.zeros((n, 3), dtype=np.int64)
    cnt = np.zeros((n, 3), dtype=np.int64)
    for a in range(3):
        inside = (mx[:, a, None] >= _PLANES[None, :G]) & (mn[:, a, None] <= _PLANES[None, 1:])     # [n, 64]: exact comparisons, no epsilon
        lo[:, a] = inside.argmax(axis=1)
        cnt[:, a] = inside.sum(axis=1)                                                              # (a contiguous run of cells)
    per_tri = cnt[:, 0] * cnt[:, 1] * cnt[:, 2]
    total = int(per_tri.sum())
    tri = np.repeat(np.arange(n), per_tri)
    j = np.arange(total) - np.repeat(np.cumsum(per_tri) - per_tri, per_tri)
    nyz = (cnt[:, 1] * cnt[:, 2])[tri]
    x = j // np.maximum(nyz, 1)
    r = j - x * nyz
    y = r // np.maximum(cnt[tri, 2], 1)
    z = r - y * cnt[tri, 2]
    cell = ((lo[tri, 0] + x) * G + (lo[tri, 1] + y)) * G + (lo[tri, 2] + z)
    order = np.argsort(cell, kind="stable")                         # every cell's triangles in ascending index
    cell, tri = cell[order], tri[order]
    counts = np.bincount(cell, minlength=G ** 3)
    first = np.cumsum(counts) - counts
    rank = np.arange(total) - first[cell]
    chan = np.stack([((argb >> 16) & 255) / 255.0, ((argb >> 8) & 255) / 255.0, (argb & 255) / 255.0], axis=-1)     # Color(uint)
    acc = np.zeros((G ** 3, 3))
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.searchsorted(rank[by_rank], np.arange(int(counts.max()) + 1 if total else 1))
    for k in range(len(bounds) - 1):                                 # the k-th triangle of every cell that has one: sequential sums
        sel = by_rank[bounds[k]:bounds[k + 1]]
        acc[cell[sel]] = acc[cell[sel]] + chan[tri[sel]]
    filled = counts > 0
    colors = np.zeros(G ** 3, dtype=np.uint32)
    avg = acc[filled] / counts[filled, None].astype(np.float64)
    by = (avg * 255.0).astype(np.int64) & 255
    colors[filled] = (0xFF000000 | (by[:, 0] << 16) | (by[:, 1] << 8) | by[:, 2]).astype(np.uint32)
    normals = np.zeros((G ** 3, 3))
    tn = triangle_normals(v9)
    normals[filled] = tn[tri[first[filled]]]
    stats = dict(triangles=n, filled=int(filled.sum()), pairs=total, max_per_cell=int(counts.max()) if total else 0)
    return colors.reshape(G, G, G), normals.reshape(G, G, G, 3), stats


_LO, _HI = -1.0 - 1e-10, 1.0 + 1e-10


def _inside(p):
    return ((_LO < p) & (p < _HI)).all(axis=1)


def _box_segment(a, b):
    """AxisAlignedBox.IntersectLineSegment: the nearest crossing of a -> b with one of the six planes that lies on the box."""
    closest = np.full(a.shape[0], np.inf)
    cpos = np.zeros_like(a)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(6):                                           # -x, -y, -z at min; +x, +y, +z at max; originDist 1.0 each
            ax, sg = i % 3, (-1.0 if i < 3 else 1.0)
            sd, ed = sg * a[:, ax], sg * b[:, ax]
            f = (1.0 - sd) / (ed - sd)
            ok = (0.0 <= f) & (f <= 1.0)
            p = a + (b - a) * f[:, None]
            ok &= (f < closest)
            ok[ok] = _inside(p[ok])
            closest = np.where(ok, f, closest)
            cpos[ok] = p[ok]
    return np.isfinite(closest), cpos


def _clip(start, end):
    """AxisAlignedBox.ClipLineSegment(ref start, ref end) -> (overlaps, start, end)."""
    start, end = start.copy(), end.copy()
    si, ei = _inside(start), _inside(end)
    keep = si & ei
    todo = ~keep
    hit, ip = _box_segment(start, end)
    keep |= todo & hit
    m = todo & hit & si
    end[m] = ip[m]
    m = todo & hit & ~si
    original = start.copy()
    start[m] = ip[m]
    m2 = m & ~ei
    if m2.any():
        hit2, ip2 = _box_segment(end[m2], original[m2])
        idx = np.nonzero(m2)[0][hit2]
        end[idx] = ip2[hit2]
    return keep, start, end


def walk(colors, normals, starts, dirs, return_steps=False):
    """VoxelGrid.IntersectRay for a batch: dict(hit uint8, color uint32, normal [n,3]) (+ steps walked)."""
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    n = starts.shape[0]
    flat = colors.reshape(-1)
    nflat = normals.reshape(-1, 3)
    out_hit = np.zeros(n, dtype=np.uint8)
    out_cell = np.zeros(n, dtype=np.int64)
    steps_taken = np.zeros(n, dtype=np.int64)
    ok, s, e = _clip(starts, starts + dirs * 10)
    scale = float(G) - 0.001
    s = (s * 0.5 + 0.5) * scale
    e = (e * 0.5 + 0.5) * scale
    delta = e - s
    ok &= ~(np.abs(delta) < 1e-10).all(axis=1)
    idx = np.nonzero(ok)[0]
    pos, delta = s[idx], delta[idx]
    max_dim = np.maximum(np.maximum(np.abs(delta[:, 0]), np.abs(delta[:, 1])), np.abs(delta[:, 2]))
    steps = np.maximum(1, (max_dim / 0.1).astype(np.int64))
    delta = delta * (0.1 / max_dim)[:, None]
    k = 0
    while idx.size:
        c = pos.astype(np.int64)                                     # (int) truncation
        assert c.min() >= 0 and c.max() < G, "the walk left the grid"
        cell = (c[:, 0] * G + c[:, 1]) * G + c[:, 2]
        filled = flat[cell] != 0
        out_hit[idx[filled]] = 1
        out_cell[idx[filled]] = cell[filled]
        steps_taken[idx] = k + 1
        k += 1
        go = ~filled & (k < steps)
        idx, pos, delta, steps = idx[go], pos[go] + delta[go], delta[go], steps[go]      # pos += delta, accumulated
    h = out_hit.astype(bool)
    res = dict(hit=out_hit, color=np.where(h, flat[out_cell], 0).astype(np.uint32), normal=np.where(h[:, None], nflat[out_cell], 0.0))
    if return_steps:
        res["steps"] = steps_taken
    return res


def sample_colors(grid, f):
    """ARGB of every camera sample (scan order) of the voxel frame `f`; grid = (colors, normals)."""
    starts, dirs = camera_samples(f)
    r = walk(grid[0], grid[1], starts, dirs)
    hit = r["hit"].astype(bool)
    col = np.full(hit.size, (f.background_argb | 0xFF000000) & 0xFFFFFFFF, dtype=np.uint32)
    own = r["color"][hit]
    if f.flags & orc.F_SHADING and own.size:
        own = orc.shade_points(f, np.zeros((own.size, 3)), r["normal"][hit], own)      # pos stays (0, 0, 0)
    col[hit] = own
    return col


def render(grid, f):
    """The rows start_row..end_row of the voxel frame as ARGB [rows, width] (alpha 0xFF)."""
    W, n = f.width, f.sub_pixel_res
    col = sample_colors(grid, f)
    if n == 1:
        return col.reshape(-1, W)
    c = col.reshape(-1, n * n).astype(np.int64)
    r = ((c >> 16) & 255).sum(1) // (n * n)
    g = ((c >> 8) & 255).sum(1) // (n * n)
    bl = (c & 255).sum(1) // (n * n)
    return (0xFF000000 | (r << 16) | (g << 8) | bl).astype(np.uint32).reshape(-1, W)


# ---- the reference's two tests (RendererTests.cs:285-306) ----
GOLDENS = [("voxels_shading", "obj.3ds", dict(depth=4.0, shading=True)),
           ("voxels_noShading", "obj2.3DS", dict(depth=3.0, yaw_deg=170.0, pitch_deg=0.0, roll_deg=0.0, shading=False))]
