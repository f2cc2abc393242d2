"""CPU model of the reference's ambient occlusion (AmbientOcclusionMethod.cs:65-99, AmbientOcclusion.cs:101-230, Renderer.cs:1631-1638,
1693), composed only of what the oracle already exports: pathtrace_model.camera_samples, Scene.trace (one ray -> nearest hit with
ray_frac, pos, normal, color), Random (System.Random), shade_points (ShadingMethod's colour step) and Scene.render (frames with dynamic
shadows).

For every camera sample that hits the root geometry, after the inner chain has produced its colour (base, shading, dynamic shadow):
  pos    = the hit point clamped per axis to [-0.5, 0.5]
  cell   = (int)((x + 0.5) * 127) * 128 * 128 + (int)((y + 0.5) * 127) * 128 + (int)((z + 0.5) * 127)
  byte   = cache[cell] when it is not 0 (cache on), otherwise generated: 100 probes from pos + n * 0.001 with directions
           (2 u0 - 1, 2 u1 - 1, 2 u2 - 1) (NOT normalised, negated when d . n < 0); a probe escapes when it hits nothing or its nearest
           hit has ray_frac > 2.0; byte = (byte)(escapes / 100.0 * 254 + 1)
  colour = ModulatePackedColor(colour, byte)
Every row block restarts Random(random_seed); generator number k of a block (scan order: row, column, subX, subY) uses draws
300 k .. 300 k + 299.  Who generates an empty cell: the hit sample with the smallest order key of the static shadow cache's order (row r
of every block, blocks ascending, before row r + 1; columns ascending; sub-samples in loop order) -- with concurrency = 1 that is the
scan order, i.e. the reference's own frame.  The model keeps the 128^3 cache between calls, as a Renderer does.
"""
import os

import numpy as np

import pathtrace_model as ptm
from helpers import orc

F_AMBIENT_OCCLUSION = 1 << 13                # SR_F_AMBIENT_OCCLUSION (include/softray.h)
F_AO_UNCACHED = 1 << 14                      # SR_F_AO_UNCACHED
RES = 128                                    # staticShadowRes, passed as the cache resolution (Renderer.cs:1635)
PROBES = 100                                 # ambientOcclusionQuality
PROBE_OFFSET = 0.001
PROBE_DIST = 2.0
TRACE_ROOT_TREE, TRACE_NEAREST = ptm.TRACE_ROOT_TREE, ptm.TRACE_NEAREST


def modulate(color, amount):
    """Color.ModulatePackedColor (Color.cs:124-133): per channel (c * amount) >> 8, alpha 255."""
    c = np.asarray(color).astype(np.int64)
    a = np.asarray(amount).astype(np.int64)
    r = (((c >> 16) & 255) * a >> 8) & 255
    g = (((c >> 8) & 255) * a >> 8) & 255
    b = ((c & 255) * a >> 8) & 255
    return ((255 << 24) + (r << 16) + (g << 8) + b).astype(np.uint32)


def clamp_pos(pos):
    return np.minimum(np.maximum(-0.5, pos), 0.5)


def cells(pos_clamped):
    k = ((pos_clamped + 0.5) * (RES - 1)).astype(np.int64)
    return k[:, 0] * RES * RES + k[:, 1] * RES + k[:, 2]


def order_keys(sample, width, n2, num_rows, concurrency):
    """static_key of scan positions `sample`: ((row-in-block * blocks + block) * width + col) * n2 + sub-sample."""
    conc = concurrency if concurrency > 0 else 4
    block_height = (num_rows - 1 + conc) // conc
    nblocks = (num_rows - 1 + block_height) // block_height
    sample = np.asarray(sample, dtype=np.int64)
    si, pix = sample % n2, sample // n2
    col, row = pix % width, pix // width
    return (((row % block_height) * nblocks + row // block_height) * width + col) * n2 + si


def probe_bytes(scene, target, pos_clamped, normal, k, seed):
    """The byte of every generator: its 100 probes in one batch."""
    if k.size == 0:
        return np.zeros(0, dtype=np.uint8)
    u = orc.Random(seed).NextDoubles(3 * PROBES * (int(k.max()) + 1)).reshape(-1, PROBES, 3)
    d = u[k] * 2 - 1                                                   # [g, 100, 3]
    n = normal[:, None, :]
    dn = (d[..., 0] * n[..., 0] + d[..., 1] * n[..., 1]) + d[..., 2] * n[..., 2]
    d = np.where((dn < 0)[..., None], -d, d)
    start = pos_clamped + normal * PROBE_OFFSET
    starts = np.broadcast_to(start[:, None, :], d.shape)
    res = scene.trace(target, starts.reshape(-1, 3), d.reshape(-1, 3))
    escaped = (res["hit"] == 0) | (res["ray_frac"] > PROBE_DIST)
    count = escaped.reshape(-1, PROBES).sum(axis=1)
    return np.array([int(c / 100.0 * 254 + 1) & 255 for c in count], dtype=np.uint8)


class AoModel:
    """One Renderer's AmbientOcclusionMethod: the cache lives as long as the object."""

    def __init__(self):
        self.cache = np.zeros(RES ** 3, dtype=np.uint8)
        self.generators = 0            # of the last frame
        self.generator_samples = None  # scan positions of the last frame's generators, ascending
        self.generator_k = None        # ... and their k

    def reset(self):
        self.cache[:] = 0

    def cache3(self):
        return self.cache.reshape(RES, RES, RES)

    def sample_colors(self, scene, f, target=TRACE_ROOT_TREE):
        W, H, n = f.width, f.height, f.sub_pixel_res
        n2 = n * n
        a = min(max(0, f.start_row), H - 1)
        b = min(max(0, f.end_row), H - 1)
        num_rows = b - a + 1
        starts, dirs = ptm.camera_samples(f)
        first = scene.trace(target, starts, dirs)
        hit = first["hit"].astype(bool)
        col = np.full(hit.size, (f.background_argb | 0xFF000000) & 0xFFFFFFFF, dtype=np.uint32)
        hi = np.nonzero(hit)[0]
        self.generators, self.generator_samples, self.generator_k = 0, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        if hi.size == 0:
            return col
        nrm, pos = first["normal"][hi], first["pos"][hi]
        if f.flags & orc.F_SHADOWS:
            # the colour the inner chain leaves: the same frame without the AO bits (one sample per pixel)
            assert n == 1, "shadows with sub-pixel samples are not modelled"
            g = type(f).from_buffer_copy(bytes(f))
            g.flags = f.flags & ~(F_AMBIENT_OCCLUSION | F_AO_UNCACHED)
            inner, _ = scene.render(g, threads=min(16, os.cpu_count() or 1))
            own = inner.reshape(H, W)[a:b + 1].reshape(-1)[hi]
        else:
            own = first["color"][hi]
            if f.flags & orc.F_SHADING:
                own = orc.shade_points(f, pos, nrm, own)
        pc = clamp_pos(pos)
        cell = cells(pc)
        uncached = bool(f.flags & F_AO_UNCACHED)
        if uncached:
            is_gen = np.ones(hi.size, dtype=bool)
        else:
            # first come, first served in the deterministic order; the picks depend on which cells are empty, not on probe results
            is_gen = np.zeros(hi.size, dtype=bool)
            taken = set()
            for j in np.argsort(order_keys(hi, W, n2, num_rows, f.concurrency), kind="stable"):
                c = int(cell[j])
                if self.cache[c] == 0 and c not in taken:
                    taken.add(c)
                    is_gen[j] = True
        flags = np.zeros(hit.size, dtype=np.int64)
        flags[hi[is_gen]] = 1
        k_all = ptm.hit_indices(flags, W * n2, num_rows, f.concurrency)
        k = k_all[hi[is_gen]]
        bytes_ = probe_bytes(scene, target, pc[is_gen], nrm[is_gen], k, f.random_seed)
        self.generators = int(is_gen.sum())
        self.generator_samples, self.generator_k = hi[is_gen], k
        if uncached:
            amount = bytes_
        else:
            self.cache[cell[is_gen]] = bytes_
            amount = self.cache[cell]
            assert amount.min() > 0
        col[hi] = modulate(own, amount)
        return col

    def render(self, scene, f, target=TRACE_ROOT_TREE):
        """The rows start_row..end_row of the frame as ARGB [rows, width] (alpha 0xFF)."""
        W, n = f.width, f.sub_pixel_res
        col = self.sample_colors(scene, f, target)
        if n == 1:
            return col.reshape(-1, W)
        c = col.reshape(-1, n * n).astype(np.int64)
        r = ((c >> 16) & 255).sum(1) // (n * n)
        g = ((c >> 8) & 255).sum(1) // (n * n)
        bl = (c & 255).sum(1) // (n * n)
        return (0xFF000000 | (r << 16) | (g << 8) | bl).astype(np.uint32).reshape(-1, W)


def ao_frame(f, uncached=False):
    """`f` with the ambient-occlusion bits OR-ed in."""
    f.flags |= F_AMBIENT_OCCLUSION | (F_AO_UNCACHED if uncached else 0)
    return f
