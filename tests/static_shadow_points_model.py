"""CPU model of sr_static_shadow_points: ShadowMethod.IntersectRay's static branch (ShadowMethod.cs:106-112, Texture3DCache.Sample) applied to
n caller-given surface points IN INPUT ORDER, composed of what the other models already have -- shadow_points_model.escapes (the escape count
of sr_shadow_points, its rule for probe ends that are not finite included), ao_model.modulate -- plus the cell formula and first-wins:

  cell      (int)((p + 0.5) * 127) per axis, clamped to 0 .. 127 (a point outside the unit cube: the edge cell, where the reference asserts;
            a NaN coordinate: index 0), [x][y][z] order
  generate  point i generates iff cache[cell] == 0 when the call starts and no point j < i of the call has its cell
  byte      (byte)(escapes / (double)S * 254 + 1), 0 replaced by 1 (ShadowMethod.cs:80, Texture3DCache.cs:124-126), stored in the cache
  outputs   amount[i] = cache[cell_i], out[i] = ModulatePackedColor(color[i], amount[i])

tests/test_static_shadow_points_model.py pins it to both static goldens of the reference.
"""
import numpy as np

import ao_model
import lightfield_shadow_model as lsm
import shadow_points_model as spm

RES = 128
CELLS = RES ** 3
WHITE = 0xFFFFFFFF


def cells(pos):
    """Cache index of every point: int64 [n]."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (pos + 0.5) * (RES - 1)
    v = np.where(np.isnan(v), 0.0, v)                                       # a NaN coordinate takes index 0
    k = np.clip(np.trunc(np.clip(v, -1.0, float(RES))), 0, RES - 1).astype(np.int64)   # (int) truncates towards zero; the asserts, clamped
    return (k[:, 0] * RES + k[:, 1]) * RES + k[:, 2]


def cache_bytes(esc, samples):
    b = (np.asarray(esc).astype(np.float64) / float(samples) * 254 + 1).astype(np.int64) & 255
    return np.where(b == 0, 1, b).astype(np.uint8)


def generators_of(cell, cache):
    """bool [n]: the first point, in input order, of every cell that is empty in `cache`."""
    first = np.zeros(cell.size, dtype=bool)
    _, idx = np.unique(cell, return_index=True)                             # the first occurrence of every cell
    first[idx] = True
    return first & (cache[cell] == 0)


def static_shadow_points(scene, f, pos, nrm, target, cache, color=None):
    """(amount uint8 [n], out uint32 [n], generators).  `cache`: uint8 [128^3], read and written in place.  `scene` answers
    trace(target, starts, dirs) as shadow_points_model.escapes asks it."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, dtype=np.float64).reshape(-1, 3)
    n = pos.shape[0]
    cell = cells(pos)
    gi = np.flatnonzero(generators_of(cell, cache))
    if gi.size:
        esc = spm.escapes(scene, f, pos[gi], nrm[gi], target)
        cache[cell[gi]] = cache_bytes(esc, lsm.shadow_samples_of(f))
    amount = cache[cell].copy()
    assert n == 0 or amount.min() > 0
    col = np.full(n, WHITE, dtype=np.uint32) if color is None else np.asarray(color, dtype=np.uint32)
    return amount.astype(np.uint8), ao_model.modulate(col, amount.astype(np.int64)), int(gi.size)


def golden_order(width, height, concurrency=4):
    """The pixels of a width x height frame (one sample per pixel) in the order a static frame fills the cache: row r of every row block, blocks
    ascending, before row r + 1; columns ascending (sr_pipeline.hip static_key)."""
    block_height = (height - 1 + concurrency) // concurrency
    blocks = (height - 1 + block_height) // block_height
    row = np.repeat(np.arange(height), width)
    col = np.tile(np.arange(width), height)
    key = ((row % block_height) * blocks + row // block_height) * width + col
    return np.argsort(key, kind="stable")
