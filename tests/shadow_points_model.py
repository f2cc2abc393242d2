"""CPU model of sr_shadow_points: ShadowMethod's step (ShadowMethod.cs:103-119, 144-179) for surface points the caller gives, composed only
of what the oracle already exports and the light-field-with-shadows model already uses (Scene.trace, light_model, light_offsets, modulate):

  end   = pos + normal * 0.001                  the normal as given: not normalised, no facing test
  point light:        src = L_model + off[i],  ray (src, end - src)
  directional light:  ray (end + dir * 1000.0 + off[i], dir)
  a ray is blocked iff it hits with ray_frac <= 1.0;  escapes = S - blocked;  out = ModulatePackedColor(color, (byte)(escapes / S * 255))

It is lightfield_shadow_model.shadow_bytes with the escape count kept, plus the ingest rule for points whose probe end is not finite
(include/softray.h): a NaN component of `end` -- all S samples escape, nothing is traced; an infinite component -- what the oracle answers
for those rays (its triangles never answer them, its extra primitives can: tests/test_shadow_points_model.py pins both).
"""
import numpy as np

import ao_model
import lightfield_shadow_model as lsm
from helpers import orc

PROBE_OFFSET = lsm.PROBE_OFFSET
WHITE = 0xFFFFFFFF


def probe_ends(pos, nrm):
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        return pos + nrm * PROBE_OFFSET


def sample_rays(f, end):
    """(starts, dirs) [n, S, 3] of the S sample rays towards every probe end."""
    off = lsm.light_offsets(f)
    samples = off.shape[0]
    lpos, ldir = lsm.light_model(f)
    with np.errstate(invalid="ignore", over="ignore"):
        if f.flags & orc.F_POINT_LIGHT:
            src = np.broadcast_to((lpos[None, :] + off)[None, :, :], (end.shape[0], samples, 3))
            dirs = end[:, None, :] - src
        else:
            dirs = np.broadcast_to(ldir[None, None, :], (end.shape[0], samples, 3))
            src = (end + ldir[None, :] * 1000.0)[:, None, :] + off[None, :, :]
    return np.ascontiguousarray(src), np.ascontiguousarray(dirs)


def escapes(scene, f, pos, nrm, target, chunk=20000):
    """rayEscapeCount of every point: int64 [n] in 0..S."""
    end = probe_ends(pos, nrm)
    samples = lsm.shadow_samples_of(f)
    out = np.full(end.shape[0], samples, dtype=np.int64)
    traced = np.flatnonzero(~np.isnan(end).any(axis=1))                 # a NaN component: never traced, all escape
    for a in range(0, traced.size, chunk):
        idx = traced[a:a + chunk]
        src, dirs = sample_rays(f, end[idx])
        res = scene.trace(target, src.reshape(-1, 3), dirs.reshape(-1, 3))
        blocked = res["hit"].astype(bool) & (res["ray_frac"] <= 1.0)
        out[idx] = samples - blocked.reshape(-1, samples).sum(axis=1)
    return out


def light_bytes(esc, samples):
    return (esc.astype(np.float64) / float(samples) * 255).astype(np.int64) & 255


def shadowed(scene, f, pos, nrm, color, target):
    """out of sr_shadow_points: uint32 [n]; color None = every point 0xFFFFFFFF."""
    esc = escapes(scene, f, pos, nrm, target)
    if color is None:
        color = np.full(esc.size, WHITE, dtype=np.uint32)
    return ao_model.modulate(np.asarray(color, dtype=np.uint32), light_bytes(esc, lsm.shadow_samples_of(f)))


def bad_points():
    """Probe ends with a NaN or an infinite component, from the position, the normal or both; (pos, nrm, has_nan)."""
    p0, n0 = np.array([0.1, 0.2, -0.1]), np.array([0.0, 1.0, 0.0])
    pos, nrm = [], []
    for b in (np.nan, np.inf, -np.inf):
        for k in range(3):
            p, n = p0.copy(), n0.copy()
            p[k] = b
            pos.append(p); nrm.append(n0)
            n[k] = b
            pos.append(p0); nrm.append(n)
            p2, n2 = p0.copy(), n0.copy()
            p2[k] = b; n2[(k + 1) % 3] = -b
            pos.append(p2); nrm.append(n2)
        pos.append(np.full(3, b)); nrm.append(np.full(3, b))
        pos.append(np.full(3, b)); nrm.append(np.full(3, -b))                 # inf + (-inf) * 0.001: NaN
    pos.append(np.array([1.7976e308, 0.0, 0.0])); nrm.append(np.array([1.79e308, 0.0, 0.0]))  # finite inputs, the probe end overflows to +inf
    pos, nrm = np.array(pos), np.array(nrm)
    return pos, nrm, np.isnan(probe_ends(pos, nrm)).any(axis=1)
