"""CPU model of the reference's triangle-index light field (rayTraceLightField with LightFieldStoresTriangles = true: LightFieldTriMethod.cs:82-231,
LightField4D.cs:175-206, 253-273, 304-344, SpatialSubdivision.cs:235-243, 428-452, 629-676, Triangle.cs:83-104, Renderer.cs:1590-1611), composed
of what the oracle exports -- pathtrace_model.camera_samples, Scene.trace (nearest hit with tri_index and counters), shade_points,
lightfield_model.sample_cells / sphere_points -- plus two restatements that tests/test_lightfield_tri_model.py pins:

  (a) tri_records / tri_hit: Triangle's constructor and Triangle.IntersectRay in FP64 in the reference's operand order, vectorised;
  (b) build_tree: RecursivePlaneSplit -> the leaves in creation order and, per triangle, Triangle.HandleToLeafNode = the leaf that
      ProcessLeafNode assigned last (nodes are built normal side first, so the leaf with the highest node index whose list holds the triangle).

The table: 4 N^4 entries, 0 = empty, 1 = the cell's canonical ray hit nothing, e >= 2 = triangle e - 2.  The canonical ray is traced through the
MODEL ALONE (no extra geometry), a NaN ray (N = 1) stores 1.  Per camera sample (start, dir in model space, unmodified):
  cell      lightfield_model.sample_cells; a line that misses the sphere: no intersection
  e == 1    no intersection
  stage 1   Triangle.IntersectRay on triangle e - 2 alone; a hit is the result
  stage 2   the handle leaf's triangles in the leaf's order, nearest hit with strict < whose position lies strictly inside the leaf's box widened by 1e-10
  stage 3   the full trace of the model (Scene.trace target 1 = the reference tree, 3 = the global nearest hit of the own BVH's semantics)
The colour is shade_points' with F_SHADING, else the triangle's; a miss is the background.
"""
import numpy as np

import lightfield_model as lfm
import pathtrace_model as ptm
from helpers import orc

TRACE_TREE, TRACE_NEAREST = 1, 3             # Scene.trace targets WITHOUT the extra geometry: the reference tree / the global nearest hit
NOTHING = 1
EPS = 1e-10


# ---- (a) Triangle.cs:29-57 and :83-104 (Plane.IntersectRay inside), every product and sum in the reference's order ----
def tri_records(v9):
    """The precomputed fields of every triangle, [n, 15]: unit normal, originDist, vertex1, edge2Perp, edge1 . edge2Perp, edge1Perp, edge2 . edge1Perp."""
    v = np.asarray(v9, dtype=np.float64).reshape(-1, 9)
    e1 = v[:, 3:6] - v[:, 0:3]
    e2 = v[:, 6:9] - v[:, 0:3]
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    zero = (-EPS < nx) & (nx < EPS) & (-EPS < ny) & (ny < EPS) & (-EPS < nz) & (nz < EPS)
    nx, ny, nz = np.where(zero, 1.0, nx), np.where(zero, 0.0, ny), np.where(zero, 0.0, nz)
    inv = 1.0 / np.sqrt(nx * nx + ny * ny + nz * nz)
    ux, uy, uz = nx * inv, ny * inv, nz * inv
    r = np.zeros((v.shape[0], 15))
    r[:, 0], r[:, 1], r[:, 2] = ux, uy, uz
    r[:, 3] = v[:, 0] * ux + v[:, 1] * uy + v[:, 2] * uz
    r[:, 4:7] = v[:, 0:3]
    p1 = np.stack([e1[:, 1] * nz - e1[:, 2] * ny, e1[:, 2] * nx - e1[:, 0] * nz, e1[:, 0] * ny - e1[:, 1] * nx], axis=1)     # edge1 x n
    p2 = np.stack([e2[:, 1] * nz - e2[:, 2] * ny, e2[:, 2] * nx - e2[:, 0] * nz, e2[:, 0] * ny - e2[:, 1] * nx], axis=1)     # edge2 x n
    r[:, 7:10] = p2
    r[:, 10] = e1[:, 0] * p2[:, 0] + e1[:, 1] * p2[:, 1] + e1[:, 2] * p2[:, 2]
    r[:, 11:14] = p1
    r[:, 14] = e2[:, 0] * p1[:, 0] + e2[:, 1] * p1[:, 1] + e2[:, 2] * p1[:, 2]
    return r


def tri_hit(rec, s, d):
    """Triangle.IntersectRay of ray i (s[i], d[i]) with record rec[i] (or one record for all): (hit bool [n], rayFrac [n], pos [n, 3])."""
    s = np.asarray(s, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    p = np.broadcast_to(np.asarray(rec, dtype=np.float64).reshape(-1, 15), (s.shape[0], 15))
    with np.errstate(all="ignore"):
        start_dist = s[:, 0] * p[:, 0] + s[:, 1] * p[:, 1] + s[:, 2] * p[:, 2]
        dir_dist = d[:, 0] * p[:, 0] + d[:, 1] * p[:, 1] + d[:, 2] * p[:, 2]
        rf = p[:, 3] - start_dist
        ok = ~(dir_dist >= 0.0) & (rf <= 0.0)
        rf = rf / dir_dist
        pos = s + d * rf[:, None]
        w = pos - p[:, 4:7]
        sv = (w[:, 0] * p[:, 7] + w[:, 1] * p[:, 8] + w[:, 2] * p[:, 9]) / p[:, 10]
        tv = (w[:, 0] * p[:, 11] + w[:, 1] * p[:, 12] + w[:, 2] * p[:, 13]) / p[:, 14]
        ok &= ~((sv < 0.0) | (sv > 1.0))
        ok &= (sv >= 0.0) & (tv >= 0.0) & (sv + tv <= 1.0)
    return ok, np.where(ok, rf, 0.0), np.where(ok[:, None], pos, 0.0)


# ---- (b) SpatialSubdivision.cs:39-230: the tree's leaves and the triangles' handles ----
class Tree:
    def __init__(self):
        self.num_nodes = self.num_leaves = self.depth = 0
        self.leaf_node = []          # node index of leaf k (creation order)
        self.leaf_lo, self.leaf_hi = [], []     # the containment test's box: min - 1e-10, max + 1e-10
        self.leaf_members = []       # int32 arrays, the leaf's order
        self.handle = None           # per triangle: index k of its handle leaf

    def stats(self):
        return (self.depth, self.num_nodes, self.num_leaves, self.num_nodes - self.num_leaves)


def build_tree(v9, bmin, bmax, max_depth=15, max_per_leaf=25):
    v = np.asarray(v9, dtype=np.float64).reshape(-1, 3, 3)
    t = Tree()
    t.handle = np.full(v.shape[0], -1, dtype=np.int64)

    def leaf(idx, geom, mn, mx):
        k = len(t.leaf_node)
        t.leaf_node.append(idx)
        t.leaf_lo.append(mn - EPS)
        t.leaf_hi.append(mx + EPS)
        t.leaf_members.append(geom.astype(np.int32))
        t.handle[geom] = k           # ProcessLeafNode: the last leaf to list a triangle keeps its handle
        t.num_leaves += 1

    def split(geom, mn, mx, depth):
        idx = t.num_nodes
        t.num_nodes += 1
        t.depth = max(t.depth, depth)
        if depth >= max_depth or geom.size <= max_per_leaf:
            return leaf(idx, geom, mn, mx)
        ext = np.abs(mx - mn)
        if ext[0] > ext[1]:
            axis = 0 if ext[0] > ext[2] else 2
        else:
            axis = 1 if ext[1] > ext[2] else 2
        c = (mn + mx) * 0.5
        side = v[geom][:, :, axis] >= c[axis]                # Point.IntersectPlane: normal side where the coordinate >= the plane's distance
        ns, bs = geom[side.any(axis=1)], geom[(~side).any(axis=1)]
        if ns.size == geom.size or bs.size == geom.size:     # rejected split
            return leaf(idx, geom, mn, mx)
        norm_min, back_max = mn.copy(), mx.copy()
        norm_min[axis] = back_max[axis] = c[axis]
        if ns.size:
            split(ns, norm_min, mx, depth + 1)               # normal side first
        if bs.size:
            split(bs, mn, back_max, depth + 1)

    split(np.arange(v.shape[0], dtype=np.int64), np.asarray(bmin, dtype=np.float64).copy(), np.asarray(bmax, dtype=np.float64).copy(), 1)
    return t


def handle_leaf(tree, tri):
    """(box [6] = lo, hi; members in order) of triangle tri's handle leaf."""
    k = int(tree.handle[tri])
    return np.concatenate([tree.leaf_lo[k], tree.leaf_hi[k]]), tree.leaf_members[k]


# ---- the method ----
class LightFieldTriModel:
    """One Renderer's LightFieldTriMethod at resolution n over (oracle scene with its tree built, v9, argb, model tree); the table lives as long as the object."""

    def __init__(self, scene, v9, argb, tree, n=64):
        self.scene, self.tree, self.n = scene, tree, n
        self.rec = tri_records(v9)
        self.argb = np.asarray(argb, dtype=np.uint32)
        self.points = lfm.sphere_points(n)
        self.table = {}
        self.filled = np.zeros(0, dtype=np.int64)
        self.coord_margin = self.term_margin = float("inf")
        self.stats = [0] * 24
        self.stage3_hits = self.stage3_misses = 0

    def reset(self):
        self.table = {}

    def dense(self):
        out = np.zeros(lfm.cache_entries(self.n), dtype=np.uint32)
        if self.table:
            out[np.fromiter(self.table.keys(), dtype=np.int64)] = np.fromiter(self.table.values(), dtype=np.uint32)
        return out

    def fill(self, index, target):
        """Entries of the cells `index` (all empty); returns (canonical rays traced, their tests, node visits, leaf visits)."""
        u, v, s, t = lfm.decode(index, self.n)
        start = self.points[u, v]
        dirs = self.points[s, t] - start
        real = ~np.isnan(start.sum(axis=1) + dirs.sum(axis=1))
        e = np.full(index.size, NOTHING, dtype=np.int64)
        walk = [int(real.sum()), 0, 0, 0]
        if real.any():
            res = self.scene.trace(target, np.ascontiguousarray(start[real]), np.ascontiguousarray(dirs[real]), counters=True)
            e[real] = np.where(res["hit"].astype(bool), res["tri_index"].astype(np.int64) + 2, NOTHING)
            walk[1:] = [int(x) for x in res["counters"].sum(axis=0)]
        for i, x in zip(index.tolist(), e.tolist()):
            self.table[i] = x
        return walk

    def bake(self, target, first=0, count=None):
        """Every empty entry of the range; returns the number written."""
        total = lfm.cache_entries(self.n)
        count = total - first if count is None else count
        index = np.array([i for i in range(first, first + count) if i not in self.table], dtype=np.int64)
        walk = self.fill(index, target) if index.size else [0, 0, 0, 0]
        self.stats = [0] * 24
        self.stats[4:8] = walk
        return index.size

    def sample_colors(self, f, target=TRACE_TREE):
        starts, dirs = ptm.camera_samples(f)
        idx, self.coord_margin, self.term_margin = lfm.sample_cells(starts, dirs, self.n)
        bg = (f.background_argb | 0xFF000000) & 0xFFFFFFFF
        nsamp = idx.size
        st = [0] * 24
        st[0] = nsamp
        inside = idx >= 0
        cells = np.unique(idx[inside])
        self.filled = np.array([c for c in cells.tolist() if c not in self.table], dtype=np.int64)
        if self.filled.size:
            st[4:8] = self.fill(self.filled, target)
        e = np.full(nsamp, NOTHING, dtype=np.int64)
        if cells.size:
            values = np.array([self.table[int(c)] for c in cells], dtype=np.int64)
            e[inside] = values[np.searchsorted(cells, idx[inside])]
        hit = np.zeros(nsamp, dtype=bool)
        pos = np.zeros((nsamp, 3))
        tri = np.full(nsamp, -1, dtype=np.int64)
        cand = np.nonzero(e >= 2)[0]
        st[20] = nsamp - cand.size
        # stage 1
        t0 = e[cand] - 2
        ok, _, p = tri_hit(self.rec[t0], starts[cand], dirs[cand])
        st[1] += cand.size
        hit[cand[ok]], pos[cand[ok]], tri[cand[ok]] = True, p[ok], t0[ok]
        st[21] = int(ok.sum())
        # stage 2: per handle leaf, the members in order
        rest, rest_tri = cand[~ok], t0[~ok]
        leaves = self.tree.handle[rest_tri]
        done2 = np.zeros(rest.size, dtype=bool)
        for k in np.unique(leaves):
            sel = np.nonzero(leaves == k)[0]
            rays = rest[sel]
            lo, hi = self.tree.leaf_lo[k], self.tree.leaf_hi[k]
            best = np.full(sel.size, np.inf)
            btri = np.full(sel.size, -1, dtype=np.int64)
            bpos = np.zeros((sel.size, 3))
            members = self.tree.leaf_members[k]
            for m in members.tolist():
                h, rf, p = tri_hit(self.rec[m], starts[rays], dirs[rays])
                better = h & (rf < best)
                better &= ((lo < p) & (p < hi)).all(axis=1)
                best[better], btri[better], bpos[better] = rf[better], m, p[better]
            st[1] += sel.size * members.size
            st[2] += sel.size
            st[3] += sel.size
            got = btri >= 0
            done2[sel[got]] = True
            hit[rays[got]], pos[rays[got]], tri[rays[got]] = True, bpos[got], btri[got]
        st[22] = int(done2.sum())
        # stage 3
        last = rest[~done2]
        st[23] = last.size
        self.stage3_hits = self.stage3_misses = 0
        nrm3 = col3 = None
        if last.size:
            res = self.scene.trace(target, np.ascontiguousarray(starts[last]), np.ascontiguousarray(dirs[last]), counters=True)
            h3 = res["hit"].astype(bool)
            hit[last], pos[last], tri[last] = h3, res["pos"], res["tri_index"]
            cnt = res["counters"].sum(axis=0)
            st[1] += int(cnt[0]); st[2] += int(cnt[1]); st[3] += int(cnt[2])
            self.stage3_hits, self.stage3_misses = int(h3.sum()), int((~h3).sum())
        col = np.full(nsamp, bg, dtype=np.uint32)
        k = np.nonzero(hit)[0]
        if k.size:
            own = self.argb[tri[k]]
            if f.flags & orc.F_SHADING:
                own = orc.shade_points(f, pos[k], self.rec[tri[k], 0:3], own)
            col[k] = own
        self.stats = st
        return col

    def render(self, f, target=TRACE_TREE):
        """The rows start_row..end_row of the frame as ARGB [rows, width] (alpha 0xFF after the resolve of sub-pixel samples)."""
        W, n = f.width, f.sub_pixel_res
        col = self.sample_colors(f, target)
        if n == 1:
            return col.reshape(-1, W)
        c = col.reshape(-1, n * n).astype(np.int64)
        r = ((c >> 16) & 255).sum(1) // (n * n)
        g = ((c >> 8) & 255).sum(1) // (n * n)
        bl = (c & 255).sum(1) // (n * n)
        return (0xFF000000 | (r << 16) | (g << 8) | bl).astype(np.uint32).reshape(-1, W)


# ---- the frames tests/test_gpu_lightfield_tri.py renders: entries of lightfield_model.GPU_FRAMES (coarse tables make the later stages work) ----
GPU_FRAMES_TRI = ["contention", "small_blur", "view0_n8", "view1_n8", "view2_n8", "far_n16", "far_primitives", "view0_n64", "unit_cube"]


def model_data(model):
    """(v9, argb, bmin, bmax) of a model name of lightfield_model.GPU_FRAMES."""
    from helpers import load_obj3ds, unit_cube_scene
    return unit_cube_scene(2000) if model == "unit_cube_2000" else load_obj3ds(model)


def oracle_scene(model):
    """(oracle scene with its tree at the default 15 / 25 and NO extra geometry, v9, argb, model tree)."""
    v9, argb, bmin, bmax = model_data(model)
    s = orc.Scene()
    s.set_triangles(v9, argb, bmin, bmax)
    assert s.build_tree() == 0
    return s, v9, argb, build_tree(v9, bmin, bmax)
