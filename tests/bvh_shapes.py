"""Adversarial geometry for the library's own BVH, and a plain model of the device build.

Generators (deterministic, numpy only) of the shapes a BVH builder and its walks usually get wrong -- trees as deep as the traversal
stacks allow, a four-wide tree as deep as its binary one, triangles with equal Morton keys, exact duplicates, an axis on which every box
centre coincides -- and `lbvh_model`, a restatement of the device LBVH's keys, radix tree and leaf collapse (sr_lbvh.hip: k_lbvh_keys,
k_lbvh_tree, k_lbvh_mark) that never calls into the library; with it `lbvh_nodes` (the same tree with its fp32 boxes), `sah_nodes` (the
host's binned-SAH builder) and `wide_depth_model` (the collapse into the four-wide tree).  Every generator returns (v9 [n, 3, 3],
argb [n], bmin [3], bmax [3]) with a distinct colour per triangle.
"""
import math

import numpy as np

UNIT_MIN, UNIT_MAX = np.array([-0.5] * 3), np.array([0.5] * 3)
MORTON_CELLS = 2097151.0                      # 2^21 - 1: the scale of k_lbvh_keys
CHAIN_MAX = (0.75, 0.5, 0.5)                  # the chain's first triangle reaches x = 0.7: its root box is [-0.5, 0.75] x [-0.5, 0.5]^2
CHAIN_Y = -0.4                                # the shrinking chain lies in the plane z = 0 around this y; it converges to (0, CHAIN_Y, 0)
STAIRCASE_MAX = 61                            # keys 2^j - 1, j <= 60: every coordinate stays below the middle of the box


def colours(n, first=0):
    """n distinct opaque colours (an odd multiplier is a bijection of the 24-bit values)."""
    i = np.arange(first + 1, first + n + 1, dtype=np.uint64)
    return (np.uint32(0xFF000000) | ((i * np.uint64(2654435761)) & np.uint64(0xFFFFFF)).astype(np.uint32)).astype(np.uint32)


def soup(n, centre, extent, seed):
    """n random triangles inside the cube of edge `extent` about `centre` (each at most a quarter of it long)."""
    r = np.random.RandomState(seed)
    c = np.asarray(centre, dtype=np.float64)
    v1 = c + (r.random_sample((n, 3)) - 0.5) * extent * 0.75
    v2 = v1 + (r.random_sample((n, 3)) - 0.5) * extent * 0.25
    v3 = v1 + (r.random_sample((n, 3)) - 0.5) * extent * 0.25
    return np.stack([v1, v2, v3], axis=1)


def _pack(parts, bmax=UNIT_MAX):
    v9 = np.ascontiguousarray(np.concatenate(parts, axis=0), dtype=np.float64)
    return v9, colours(v9.shape[0]), UNIT_MIN.copy(), np.array(bmax, dtype=np.float64)


def shrinking_chain(n, ratio=2.0, extra=None, extra_first=False):
    """Triangle k is (c - h, y - 0.05, 0), (c + h, y - 0.05, 0), (c, y + 0.05, 0) with c = 0.45 ratio^-k, h = 0.25 ratio^-k: every
    triangle is as far from the next as it is wide, so no split separates more than one of them from the rest and the tree is a path.
    `extra` ([m, 3, 3], e.g. soup(...)) is appended (or put first): visible triangles, so that frames are not empty."""
    k = np.arange(n, dtype=np.float64)
    c, h = 0.45 * ratio ** -k, 0.25 * ratio ** -k
    z = np.zeros(n)
    lo, hi = np.full(n, CHAIN_Y - 0.05), np.full(n, CHAIN_Y + 0.05)
    chain = np.stack([np.stack([c - h, lo, z], axis=1), np.stack([c + h, lo, z], axis=1), np.stack([c, hi, z], axis=1)], axis=1)
    if extra is None:
        return _pack([chain], CHAIN_MAX)
    return _pack([extra, chain] if extra_first else [chain, extra], CHAIN_MAX)


def staircase_centres(m):
    """Box centres whose Morton keys are 2^j - 1, j = 0 .. m - 1, in the unit box: the radix tree over them is a single path."""
    if not 1 <= m <= STAIRCASE_MAX:
        raise ValueError("morton_staircase: 1 <= m <= %d" % STAIRCASE_MAX)
    q = np.zeros((m, 3))
    for j in range(m):
        for a in range(3):
            cnt = max(0, -((-(j - (2 - a))) // 3))                      # ceil((j - (2 - a)) / 3): bits of axis a below bit j
            q[j, a] = (2.0 ** cnt - 0.5) / MORTON_CELLS
    return q


def morton_staircase(m, extra=None):
    """Triangle j has its box centre in the cell with Morton key 2^j - 1 (staircase_centres).  Its half extents are 0.9 of the
    centre's distance from the box's lower faces, at most 0.04: it stays inside the box, and the high steps are large enough to see."""
    q = staircase_centres(m)
    ext = UNIT_MAX - UNIT_MIN
    c = UNIT_MIN + q * ext
    r = np.minimum(0.9 * q * ext, 0.04)
    v1 = np.stack([c[:, 0] - r[:, 0], c[:, 1] - r[:, 1], c[:, 2] - r[:, 2]], axis=1)
    v2 = np.stack([c[:, 0] + r[:, 0], c[:, 1] - r[:, 1], c[:, 2] + r[:, 2]], axis=1)
    v3 = np.stack([c[:, 0], c[:, 1] + r[:, 1], c[:, 2] - r[:, 2]], axis=1)
    stairs = np.stack([v1, v2, v3], axis=1)
    return _pack([stairs] if extra is None else [stairs, extra])


def corner_cluster(n):
    """n tiny triangles inside the Morton cell 0 of the unit box (key 0, like step 0 of the staircase): they keep the lowest nodes of
    the staircase's path above the leaf size, which is how the path reaches the depth limit with at most 61 distinct steps."""
    cell = 1.0 / MORTON_CELLS
    i = np.arange(n, dtype=np.float64)
    c = UNIT_MIN + np.stack([0.3 + 0.4 * i / max(1, n), 0.5 + 0.0 * i, 0.7 - 0.4 * i / max(1, n)], axis=1) * cell
    r = 0.2 * cell
    v1 = c + np.array([-r, -r, -r]); v2 = c + np.array([r, -r, r]); v3 = c + np.array([0.0, r, -r])
    return np.stack([v1, v2, v3], axis=1)


CLUSTER_CELL = 2 ** 20 - 1                   # the cell 0111..1 on every axis: the cluster staircase converges to the box's middle


def cluster_point():
    """The point the cluster staircase converges to: the middle of the Morton cell (CLUSTER_CELL,) * 3 of the unit box."""
    return UNIT_MIN + (np.full(3, CLUSTER_CELL) + 0.5) / MORTON_CELLS


def cluster_staircase(m, r0=0.34, ratio=0.85, per=3, extra=None):
    """A staircase whose every step is a cluster of `per` oversized triangles, for a device build with one triangle per leaf whose
    FOUR-WIDE tree is about as deep as the binary one.  Step i = 0 .. m - 1 lies in the sibling of the cell of cluster_point() at key
    bit 61 - i (the one key bit flipped, every lower bit of that axis set towards the point: the cell nearest to it), step m in the
    point's own cell; the triangles of a step share their box centre (equal keys) and have box half extents r0 ratio^i 0.9^k.  The radix
    tree is a path with one step hanging off every node; the step's box is larger than that of everything below it, and so is its
    two-triangle half, so the collapse (wide_depth_model) spends both expansions of a wide node on the step and the path goes on one
    wide level per binary level.  The steps of the second and third key bit of an axis lie a quarter and an eighth of the box from the
    point, so r0 = 0.34 is what keeps step 2 inside the box, and a few of the highest steps do cost a second binary level.  The
    triangles' normals alternate between (-4, 2, 4) and (4, 2, -4) from step to step: the triangles are one-sided, so a ray through
    the point with a direction of positive product with both hits none of them and walks every level."""
    centres, radii, signs = [], [], []
    for i in range(m + 1):
        cell = [CLUSTER_CELL] * 3
        if i < m:
            a, t = (i + 1) % 3, (i + 1) // 3                            # key bit 61 - i is bit 20 - t of axis a
            cell[a] = 2 ** 20 if t == 0 else CLUSTER_CELL - 2 ** (20 - t)
        for k in range(per):
            centres.append(UNIT_MIN + (np.array(cell) + 0.5) / MORTON_CELLS)
            radii.append(r0 * ratio ** i * 0.9 ** k)
            signs.append([1, 1 - 2 * (i & 1), 1])
    c, r, s = np.array(centres), np.array(radii)[:, None], np.array(signs, dtype=np.float64)
    stairs = np.stack([c - r * s, c + r * s * np.array([1.0, -1.0, 1.0]), c + r * s * np.array([0.0, 1.0, -1.0])], axis=1)
    return _pack([stairs] if extra is None else [stairs, extra])


SAME_CENTRE = np.array([0.125, -0.0625, 0.03125])


def same_centre(n):
    """n concentric triangles of different sizes and tilts whose boxes all have exactly the centre SAME_CENTRE: every coordinate is a
    dyadic number, so centre - r and centre + r are exact and 0.5 (lo + hi) gives the centre back bit for bit."""
    if n > 4097:
        raise ValueError("same_centre: n <= 4097")
    i = np.arange(n)
    rx = (i + 1) * 2.0 ** (int(math.log2(4097 // n)) - 14)            # a power of two apart, the largest between 0.125 and 0.25
    ry = (1 + (i * 7) % 1021) * 2.0 ** -13
    rz = (1 + (i * 5) % 509) * 2.0 ** -12
    u = ((i * 5) % 9 - 4) / 4.0                                        # where on the x extent the third vertex sits
    t = np.stack([np.array([-1.0, 1.0, 0.5]), np.array([1.0, -1.0, -0.25]), np.array([0.0, -1.0, 1.0])])[i % 3]   # z of the vertices: both ends of the extent taken
    cx, cy, cz = SAME_CENTRE
    v1 = np.stack([cx - rx, cy - ry, cz + t[:, 0] * rz], axis=1)
    v2 = np.stack([cx + rx, cy - ry, cz + t[:, 1] * rz], axis=1)
    v3 = np.stack([cx + u * rx, cy + ry, cz + t[:, 2] * rz], axis=1)
    return _pack([np.stack([v1, v2, v3], axis=1)])


def exact_duplicates(base, copies, seed=7):
    """Every triangle of a soup of `base` appears `copies` times with identical vertices and different colours, at shuffled positions."""
    tris = soup(base, (0.0, 0.0, 0.0), 0.8, seed)
    v9 = np.repeat(tris, copies, axis=0)
    v9 = v9[np.random.RandomState(seed + 1).permutation(v9.shape[0])]
    return _pack([v9])


def duplicate_groups(v9):
    """For every triangle the lowest index of a triangle with the same nine coordinates."""
    flat9 = np.ascontiguousarray(v9, dtype=np.float64).reshape(-1, 9)
    _, first, inverse = np.unique(flat9, axis=0, return_index=True, return_inverse=True)
    return first[np.asarray(inverse).reshape(-1)].astype(np.int32)


def flat(n, thick=False, seed=11):
    """thick=False: every triangle lies in the plane z = 0 of a root box whose z extent is 0 (ext == 0 in k_lbvh_keys, `ext > 0` false
    in the host builder).  thick=True: the box is the unit box and the triangles tilt out of the plane by +-rz about z = 0, so all box
    centres are equal on z and on z only."""
    r = np.random.RandomState(seed)
    v1 = (r.random_sample((n, 3)) - 0.5) * 0.7
    v2 = v1 + (r.random_sample((n, 3)) - 0.5) * 0.25
    v3 = v1 + (r.random_sample((n, 3)) - 0.5) * 0.25
    v9 = np.stack([v1, v2, v3], axis=1)
    if thick:
        rz = (1 + np.arange(n) % 37) * 2.0 ** -9                       # up to 0.072, exact
        v9[:, 0, 2], v9[:, 1, 2], v9[:, 2, 2] = -rz, rz, rz * 0.5
        return _pack([v9])
    v9[:, :, 2] = 0.0
    v9, argb, bmin, bmax = _pack([v9])
    bmin[2] = bmax[2] = 0.0
    return v9, argb, bmin, bmax


# ---- the device build, restated ----
def _spread21(x):
    x = x & np.uint64(0x1fffff)
    for shift, mask in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(shift))) & np.uint64(mask)
    return x


def morton_keys(v9, bmin, bmax):
    """63-bit keys of the box centres (k_lbvh_keys): per axis (0.5 (lo + hi) - min) / ext (0 where ext == 0), clamped to [0, 1], times
    2^21 - 1, truncated; x takes the highest bit of every triple."""
    v = np.asarray(v9, dtype=np.float64).reshape(-1, 3, 3)
    bmin = np.asarray(bmin, dtype=np.float64); bmax = np.asarray(bmax, dtype=np.float64)
    lo, hi = v.min(axis=1), v.max(axis=1)
    keys = np.zeros(v.shape[0], dtype=np.uint64)
    for a in range(3):
        ext = bmax[a] - bmin[a]
        q = (0.5 * (lo[:, a] + hi[:, a]) - bmin[a]) / ext if ext > 0 else np.zeros(v.shape[0])
        q = np.minimum(np.maximum(q, 0.0), 1.0)
        keys |= _spread21((q * MORTON_CELLS).astype(np.uint64)) << np.uint64(2 - a)
    return keys


def lbvh_model(v9, bmin, bmax, leaf_max=4):
    """(depth, inner nodes, sorted order) of the device-built BVH as sr_bvh_stats reports them.

    Keys as morton_keys, stable sort, binary radix tree: a range splits where the highest differing bit of its first and last key
    changes; a range of equal keys splits by the highest differing bit of the sorted POSITIONS (k_lbvh_tree's delta: 64 + clz(i ^ j)),
    which is the radix tree over (key, position).  A node is kept iff its range holds more than leaf_max triangles (k_lbvh_mark); depth
    = the deepest kept node counted from the root (root = 1) plus 1 for the leaf level (build_bvh_device)."""
    keys = morton_keys(v9, bmin, bmax)
    order = np.argsort(keys, kind="stable")
    aug = [(int(k) << 32) | i for i, k in enumerate(keys[order])]
    depth = nodes = 0
    todo = [(0, len(aug) - 1, 1)]
    while todo:
        first, last, level = todo.pop()
        if last - first + 1 <= leaf_max:
            continue
        nodes += 1
        depth = max(depth, level)
        bit = (aug[first] ^ aug[last]).bit_length() - 1
        lo, hi = first, last                                            # the first entry with that bit set: aug[lo] has it clear, aug[hi] set
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if (aug[mid] >> bit) & 1:
                hi = mid
            else:
                lo = mid
        todo.append((first, lo, level + 1))
        todo.append((hi, last, level + 1))
    return depth + 1, nodes, order.astype(np.int64)


def _f32_down(x):
    f = np.asarray(x, dtype=np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def _f32_up(x):
    f = np.asarray(x, dtype=np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def node_boxes32(lo, hi, bmin, bmax):
    """The builders' fp32 boxes of FP64 extents lo, hi [n, 3]: relative to the root centre, padded by 2^-16 of the root's largest
    extent, rounded outward (sr_host.cpp store(), sr_lbvh.hip tri_box)."""
    bmin = np.asarray(bmin, dtype=np.float64); bmax = np.asarray(bmax, dtype=np.float64)
    ext = float(np.max(bmax - bmin))
    pad = math.ldexp(ext if ext > 0 else 1.0, -16)
    centre = (bmin + bmax) * 0.5
    return _f32_down(lo - centre - pad), _f32_up(hi - centre + pad)


def lbvh_nodes(v9, bmin, bmax, leaf_max=4):
    """The device-built binary tree as wide_depth_model takes it: node i = ((lo, hi, child), (lo, hi, child)) with the children's fp32
    boxes (unions of the triangles' boxes, k_lbvh_boxes) and child = the index of an inner node, -1 for a leaf; node 0 is the root.
    Topology as lbvh_model.  A scene that fits one leaf has a root with that leaf alone."""
    v = np.asarray(v9, dtype=np.float64).reshape(-1, 3, 3)
    keys = morton_keys(v, bmin, bmax)
    order = np.argsort(keys, kind="stable")
    aug = [(int(k) << 32) | i for i, k in enumerate(keys[order])]
    tlo, thi = node_boxes32(v.min(axis=1)[order], v.max(axis=1)[order], bmin, bmax)
    nodes = []

    def build(first, last):
        box = (tlo[first:last + 1].min(axis=0), thi[first:last + 1].max(axis=0))
        if last - first + 1 <= leaf_max:
            return box + (-1,)
        idx = len(nodes)
        nodes.append(None)
        bit = (aug[first] ^ aug[last]).bit_length() - 1
        lo, hi = first, last
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if (aug[mid] >> bit) & 1:
                hi = mid
            else:
                lo = mid
        nodes[idx] = (build(first, lo), build(hi, last))
        return box + (idx,)

    top = build(0, len(aug) - 1)
    return nodes if nodes else [(top,)]


SAH_BINS = 16


def sah_nodes(v9, bmin, bmax, leaf_max=4):
    """The host-built binary tree (sr_host.cpp BvhBuilder::build), in lbvh_nodes' form, with its depth: (nodes, depth).  The widest
    axis of the centroids' box (the first on a tie), 16 bins over it, the split of least sum of half area x count (the first on a
    tie), a stable partition; where no bin boundary separates the range, the halves by index of the order by (centre, index)."""
    v = np.asarray(v9, dtype=np.float64).reshape(-1, 3, 3)
    plo, phi = v.min(axis=1), v.max(axis=1)
    pc = 0.5 * (plo + phi)
    nodes = []
    deepest = [0]

    def half_area(lo, hi):
        d = hi - lo
        return d[0] * d[1] + d[1] * d[2] + d[2] * d[0]

    def build(ids, depth):
        deepest[0] = max(deepest[0], depth)
        lo, hi = plo[ids].min(axis=0), phi[ids].max(axis=0)
        flo, fhi = node_boxes32(lo, hi, bmin, bmax)
        if len(ids) <= leaf_max:
            return (flo, fhi, -1)
        c = pc[ids]
        clo, chi = c.min(axis=0), c.max(axis=0)
        axis, ext = 0, chi[0] - clo[0]
        for a in (1, 2):
            if chi[a] - clo[a] > ext:
                axis, ext = a, chi[a] - clo[a]
        left = right = None
        if ext > 0:
            k1 = SAH_BINS * (1.0 - 1e-9) / ext
            bins = np.clip(((c[:, axis] - clo[axis]) * k1).astype(np.int64), 0, SAH_BINS - 1)
            best, bestk = None, -1
            for k in range(SAH_BINS - 1):
                l, r = ids[bins <= k], ids[bins > k]
                if len(l) == 0 or len(r) == 0:
                    continue
                cost = half_area(plo[l].min(axis=0), phi[l].max(axis=0)) * len(l) + half_area(plo[r].min(axis=0), phi[r].max(axis=0)) * len(r)
                if best is None or cost < best:
                    best, bestk = cost, k
            if bestk >= 0:
                left, right = ids[bins <= bestk], ids[bins > bestk]
        if left is None:
            by = sorted(ids.tolist(), key=lambda i: (pc[i, axis], i))
            mid = len(by) // 2
            left, right = np.array(by[:mid]), np.array(by[mid:])
        idx = len(nodes)
        nodes.append(None)
        l = build(left, depth + 1)
        r = build(right, depth + 1)
        nodes[idx] = (l, r)
        return (flo, fhi, idx)

    top = build(np.arange(v.shape[0]), 1)
    return (nodes if nodes else [(top,)]), deepest[0]


def wide_depth_model(nodes, fp32=False):
    """Depth of the four-wide tree collapsed from a binary one (collapse_bvh4 in sr_host.cpp, k_collapse_level in sr_lbvh.hip), as
    sr_wide_tree_stats()[0] reports it.  A wide node takes a binary node's two children and, while it has fewer than four, replaces
    the inner child of largest box area dx dy + dy dz + dz dx (the first of equals) by that child's two children; every inner child
    left is a wide node one level down.  The host takes the areas of the fp32 boxes in FP64, the device (fp32=True) in fp32."""
    t = np.float32 if fp32 else np.float64

    def area(child):
        d = child[1].astype(t) - child[0].astype(t)
        return d[0] * d[1] + d[1] * d[2] + d[2] * d[0]

    depth = 0
    todo = [(0, 1)]
    while todo:
        src, level = todo.pop()
        depth = max(depth, level)
        ch = list(nodes[src])
        while len(ch) < 4:
            best, best_area = -1, -1.0
            for i, c in enumerate(ch):
                if c[2] >= 0 and area(c) > best_area:
                    best, best_area = i, area(c)
            if best < 0:
                break
            ch[best:best + 1] = list(nodes[ch[best][2]])
        todo.extend((c[2], level + 1) for c in ch if c[2] >= 0)
    return depth


def levels_crossed_model(nodes, bmin, bmax, start, direction):
    """The deepest level (root = 1) of an inner node of `nodes` (lbvh_nodes / sah_nodes) whose box the line start + t direction
    crosses, its ancestors' boxes with it: a ray that hits nothing visits at least that many nodes, on whichever form of the tree."""
    centre = (np.asarray(bmin, dtype=np.float64) + np.asarray(bmax, dtype=np.float64)) * 0.5
    s = np.asarray(start, dtype=np.float64) - centre
    d = np.asarray(direction, dtype=np.float64)

    def crosses(child):
        t0, t1 = -np.inf, np.inf
        for a in range(3):
            lo, hi = float(child[0][a]), float(child[1][a])
            if d[a] == 0.0:
                if not lo <= s[a] <= hi:
                    return False
                continue
            ta, tb = (lo - s[a]) / d[a], (hi - s[a]) / d[a]
            t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
        return t0 <= t1

    deepest = 0
    todo = [(0, 1)]
    while todo:
        i, level = todo.pop()
        deepest = max(deepest, level)
        todo.extend((c[2], level + 1) for c in nodes[i] if c[2] >= 0 and crosses(c))
    return deepest


def balanced_position_depth(n, leaf_max):
    """Depth lbvh_model gives n equal keys: the radix tree over the positions 0 .. n - 1, cut where a range fits a leaf."""
    def kept_levels(first, last):
        if last - first + 1 <= leaf_max:
            return 0
        bit = (first ^ last).bit_length() - 1
        split = (last >> bit) << bit                                    # the first position with that bit set
        return 1 + max(kept_levels(first, split - 1), kept_levels(split, last))
    return kept_levels(0, n - 1) + 1


# ---- ray batches ----
def rays_at_triangles(v9, indices, per_triangle=5):
    """Rays aimed at triangles: from a point above them on the plane x = 0 side of the box (outside it), at the centroid and at points
    a fraction of the triangle's own size away from it.  They start at x = 0, so that the x coordinate along the ray is a product, not
    a sum: it keeps its relative precision down to the smallest triangle of the shrinking chain."""
    v = np.asarray(v9, dtype=np.float64).reshape(-1, 3, 3)[np.asarray(indices)]
    w = np.array([[1, 1, 1], [2, 1, 1], [1, 2, 1], [1, 1, 2], [4, 3, 1], [1, 4, 3], [3, 1, 4]], dtype=np.float64)[:per_triangle]
    w /= w.sum(axis=1, keepdims=True)
    targets = np.einsum("pk,nkc->npc", w, v).reshape(-1, 3)           # barycentric combinations: strictly inside
    starts = np.tile(np.array([0.0, 0.3, 2.0]), (targets.shape[0], 1))
    return starts, targets - starts


def rays_through_point(p, count=64):
    """`count` rays through the point p from outside the unit box, directions on a spiral over the sphere."""
    k = np.arange(count) + 0.5
    zc = 1.0 - 2.0 * k / count
    rad = np.sqrt(1.0 - zc * zc)
    phi = k * math.pi * (3.0 - math.sqrt(5.0))
    d = np.stack([rad * np.cos(phi), rad * np.sin(phi), zc], axis=1)
    starts = np.asarray(p, dtype=np.float64) - 3.0 * d
    return starts, 6.0 * d


def rays_missing_by_less_than_the_pad(v9, indices, ext=1.0):
    """Rays parallel to z through a triangle's box at half the builders' box pad (2^-16 x extent) above and below its y range, at the
    x of its centre: inside the padded box, outside the triangle -- and outside every other triangle of a shrinking chain, whose
    triangles share that y range."""
    v = np.asarray(v9, dtype=np.float64).reshape(-1, 3, 3)[np.asarray(indices)]
    pad = ext * 2.0 ** -17
    lo, hi = v.min(axis=1), v.max(axis=1)
    x = 0.5 * (lo[:, 0] + hi[:, 0])
    a = np.stack([x, hi[:, 1] + pad, np.full(len(x), 2.0)], axis=1)
    b = np.stack([x, lo[:, 1] - pad, np.full(len(x), 2.0)], axis=1)
    starts = np.concatenate([a, b])
    return starts, np.tile(np.array([0.0, 0.0, -4.0]), (starts.shape[0], 1))
