"""tests/voxel_model.py with the grid size as a parameter: the CPU model of the reference's voxel-grid rendering for VoxelGrid(n, ...) /
TriMeshToVoxelGrid.Convert(tris, n, grid) with n in 1..256 (sr_set_voxel_res).  voxelise, walk, sample_colors and render are voxel_model's,
operation for operation; what depends on the size is
  * the planes of an axis, plane(k) = (double)k / (double)n - 0.5 (TriMeshToVoxelGrid.cs:28-29): a division and then a subtraction, both of
    which round when n is no power of two;
  * the cell index (x * n + y) * n + z;
  * the walk's scale (double)n - 0.001 (VoxelGrid.cs:125-177).
tests/test_voxel_res_model.py pins it to voxel_model at n = 64 (and so to the reference's goldens) and to the reference's own unit tests at 32.
"""
import numpy as np

from helpers import orc
from pathtrace_model import camera_samples
from voxel_model import F_VOXELS, TARGET_VOXELS, _box_segment, _clip, _inside, triangle_normals  # noqa: F401  (the size-independent parts)


def planes_of(n):
    """plane(k), k = 0..n, of an axis of an n-cell grid, as FP64 computes k / n - 0.5."""
    return np.arange(n + 1, dtype=np.float64) / np.float64(n) - 0.5


def voxelise(v9, argb, n=64):
    """(colors uint32 [n,n,n], normals [n,n,n,3], stats) of TriMeshToVoxelGrid.Convert(triangles, n)."""
    G = int(n)
    planes = planes_of(G)
    v9 = np.asarray(v9, dtype=np.float64).reshape(-1, 3, 3)
    argb = np.asarray(argb, dtype=np.uint32)
    nt = v9.shape[0]
    mn, mx = v9.min(axis=1), v9.max(axis=1)
    lo = np.zeros((nt, 3), dtype=np.int64)
    cnt = np.zeros((nt, 3), dtype=np.int64)
    for a in range(3):
        inside = (mx[:, a, None] >= planes[None, :G]) & (mn[:, a, None] <= planes[None, 1:])     # [triangles, n]: exact comparisons, no epsilon
        lo[:, a] = inside.argmax(axis=1)
        cnt[:, a] = inside.sum(axis=1)                                                              # (a contiguous run of cells)
    per_tri = cnt[:, 0] * cnt[:, 1] * cnt[:, 2]
    total = int(per_tri.sum())
    tri = np.repeat(np.arange(nt), per_tri)
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
    stats = dict(triangles=nt, filled=int(filled.sum()), pairs=total, max_per_cell=int(counts.max()) if total else 0)
    return colors.reshape(G, G, G), normals.reshape(G, G, G, 3), stats


def walk(colors, normals, starts, dirs, return_steps=False):
    G = colors.shape[0]
    """VoxelGrid.IntersectRay for a batch on the grid colors [n,n,n] (the scale is (double)n - 0.001): dict(hit uint8, color uint32, normal [n,3]) (+ steps walked)."""
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    nr = starts.shape[0]
    flat = colors.reshape(-1)
    nflat = normals.reshape(-1, 3)
    out_hit = np.zeros(nr, dtype=np.uint8)
    out_cell = np.zeros(nr, dtype=np.int64)
    steps_taken = np.zeros(nr, dtype=np.int64)
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


# ---- scenes and constants that tests/test_voxel_res_model.py and tests/test_gpu_voxel_res.py share ----
KAT_TRIANGLE = np.array([[-0.5, -0.5, 0.001, 0.5, 0.5, 0.001, -0.5, 0.5, 0.001]])     # TriangleTests.cs:368-393: fills 32 * 32 cells at n = 32
KAT_COLOR = np.array([0xFF40C080], dtype=np.uint32)


def boundary_triangles(n, count=240, seed=2024):
    """Small triangles whose vertex coordinates lie exactly on the planes k / n - 0.5 as FP64 computes them, or one ulp to either side
    (nextafter), mixed with arbitrary coordinates: whether `max >= plane(k)` / `min <= plane(k + 1)` holds then hangs on the last bit, which
    is where a voxeliser that scales and floors without the exact correction goes wrong.  (v9 [count, 3, 3], argb)."""
    rng = np.random.default_rng(seed + n)
    planes = planes_of(n)
    base = rng.integers(0, max(1, n - 1), (count, 1, 3))
    k = np.minimum(base + rng.integers(0, 3, (count, 3, 3)), n)                       # a triangle spans at most three planes per axis
    v = planes[k]
    kind = rng.integers(0, 4, (count, 3, 3))                                          # 0 on the plane, 1 one ulp above, 2 one ulp below, 3 anywhere in the cell
    v = np.where(kind == 1, np.nextafter(v, np.inf), v)
    v = np.where(kind == 2, np.nextafter(v, -np.inf), v)
    v = np.where(kind == 3, v + rng.uniform(0.0, 1.0, v.shape) / n, v)
    v[:8] = planes[np.array([0, n, 0, n, n, 0, 0, 0])][:, None, None]                 # degenerate triangles on the grid's own corners and faces
    v[4:8, :, 1] = np.nextafter(v[4:8, :, 1], [[np.inf], [-np.inf], [np.inf], [-np.inf]])
    argb = (rng.integers(0, 1 << 24, count).astype(np.uint32) | np.uint32(0xFF000000))
    return np.ascontiguousarray(v), argb
