"""CPU model of sr_ao_points: AmbientOcclusionMethod.IntersectRay applied to n caller-given intersections IN INPUT ORDER by one
RenderContext whose Random has made 300 * first_generator draws.  Built from the frame model's parts (tests/ao_model.py: clamp_pos,
cells, probe_bytes, modulate), so tests/test_ao_points_model.py can pin it to AoModel -- the model the AO frames are held to.

Per point: pc = pos clamped to [-0.5, 0.5] (a NaN component: 0.5 -- the reference would throw), cell = cells(pc); a GENERATOR fires 100
probes from pc + normal * 0.001; generator g of the call (input order) has k = first_generator + g, i.e. draws 300 k .. 300 k + 299.
Cached: point i generates iff cache[cell] == 0 at the start of the call and no point j < i has its cell; the byte goes into the cache and
every point's amount is its cell's byte.  Uncached: every point generates, its amount is its own byte.
A probe origin that is not finite (it can only come from the normal): a NaN component -- nothing is traced, all 100 escape, byte 255; an
infinite component -- the oracle is asked as for any origin, through its root geometry (its triangles never answer such a ray, its extra
primitives can).  Both stay generators: they take their k and fill their cell.
"""
import numpy as np

import ao_model as aom

TRACE_ROOT_TREE, TRACE_NEAREST = aom.TRACE_ROOT_TREE, aom.TRACE_NEAREST


def clamp_pos(pos):
    pos = np.asarray(pos, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(pos), 0.5, aom.clamp_pos(pos))


class NearestWithExtras:
    """The root geometry of a SR_MODE_BVH frame for a probe: the extra primitives plus the global nearest triangle hit.  The oracle's
    TRACE_NEAREST has no extra geometry, so the primitives are asked through `extras_only` -- a scene that holds them and a model no probe
    can meet.  A probe only asks "is there a hit with rayFrac <= 2.0", so the nearer of the two answers is all it needs."""

    def __init__(self, scene, extras_only):
        self.scene, self.extras_only = scene, extras_only

    def trace(self, target, starts, dirs):
        a = self.scene.trace(TRACE_NEAREST, starts, dirs)
        b = self.extras_only.trace(TRACE_ROOT_TREE, starts, dirs)
        ha, hb = a["hit"].astype(bool), b["hit"].astype(bool)
        fa = np.where(ha, a["ray_frac"], np.inf)
        fb = np.where(hb, b["ray_frac"], np.inf)
        return dict(hit=(ha | hb).astype(np.uint8), ray_frac=np.minimum(fa, fb))


def ao_points(scene, target, pos, nrm, seed, cache, uncached=False, first_generator=0, color=None, inf_scene=None):
    """(amount uint8 [n], out uint32 [n], generators).  `cache`: uint8 [128^3], read and written in place unless `uncached`.  `scene` answers
    trace(target, starts, dirs) for the finite origins, `inf_scene` (default: scene) trace(TRACE_ROOT_TREE, ...) for the infinite ones."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, dtype=np.float64).reshape(-1, 3)
    n = pos.shape[0]
    pc = clamp_pos(pos)
    cell = aom.cells(pc)
    if uncached:
        is_gen = np.ones(n, dtype=bool)
    else:
        is_gen = np.zeros(n, dtype=bool)
        taken = set()
        for i in range(n):                                                  # first come, first served in input order
            c = int(cell[i])
            if cache[c] == 0 and c not in taken:
                taken.add(c)
                is_gen[i] = True
    gi = np.flatnonzero(is_gen)
    k = first_generator + np.arange(gi.size, dtype=np.int64)               # k = first_generator + running index
    with np.errstate(invalid="ignore", over="ignore"):
        origin = pc[gi] + nrm[gi] * aom.PROBE_OFFSET
    has_nan = np.isnan(origin).any(axis=1)
    has_inf = np.isinf(origin).any(axis=1) & ~has_nan
    finite = ~has_nan & ~has_inf
    b = np.zeros(gi.size, dtype=np.uint8)
    b[has_nan] = int(100 / 100.0 * 254 + 1)
    with np.errstate(invalid="ignore", over="ignore"):
        if finite.any():
            b[finite] = aom.probe_bytes(scene, target, pc[gi][finite], nrm[gi][finite], k[finite], seed)
        if has_inf.any():
            b[has_inf] = aom.probe_bytes(inf_scene if inf_scene is not None else scene, TRACE_ROOT_TREE, pc[gi][has_inf], nrm[gi][has_inf], k[has_inf], seed)
    if uncached:
        amount = b
    else:
        cache[cell[gi]] = b
        amount = cache[cell].copy()
        assert n == 0 or amount.min() > 0
    col = np.full(n, 0xFFFFFFFF, dtype=np.uint32) if color is None else np.asarray(color, dtype=np.uint32)
    return amount.astype(np.uint8), aom.modulate(col, amount), int(gi.size)
