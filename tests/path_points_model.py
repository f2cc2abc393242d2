"""CPU model of sr_path_points: PathTracingMethod.IntersectRay's step (PathTracingMethod.cs:51-76) applied to n caller-given intersections
IN INPUT ORDER by one RenderContext whose Random(frame.random_seed) has made 3 * first_sample draws.  Composed of the oracle's exports
(Scene.trace, Random, shade_points), as tests/pathtrace_model.py is -- tests/test_path_points_model.py pins it to that model's samples.

Point i uses draws 3 (first_sample + i) .. + 2 (every point is a hit):
  u        = InternalSample * (1.0 / 2147483647.0)
  d        = (2 u0 - 1, 2 u1 - 1, 2 u2 - 1), negated when d . n < 0.0, multiplied by 1 / length                     -> dirs
  incoming = colour of the nearest hit of the ray (pos + n * 0.001, d), shaded when the frame has F_SHADING; 0 on a miss
  out      = incoming / 255.0 * (n . d) + color / 255.0 per channel, all three scaled by 1 / sqrt(r^2 + g^2 + b^2) when one exceeds 1.0,
             bytes by truncation (NaN: 0), alpha 0xFF
A second-ray origin that is not finite: a NaN component -- nothing is traced, no hit; an infinite component -- the oracle is asked as for
any origin, through `inf_scene`'s root geometry (its triangles never answer such a ray, its extra primitives can).  The colour step runs
on whatever IEEE gives.
"""
import numpy as np

from helpers import orc
from pathtrace_model import TRACE_NEAREST, TRACE_ROOT_TREE, _unpack

OFFSET = 0.001                                # raySurfaceOffset
WHITE = 0xFFFFFFFF


class NearestWithExtras:
    """The root geometry of a SR_MODE_BVH frame for a second ray: the extra primitives from the ray's origin first, then the global
    nearest triangle hit where it is strictly nearer.  The oracle's TRACE_NEAREST has no extra geometry, so the primitives are asked
    through `extras_only` -- a scene that holds them and a model no ray of the tests can meet."""

    def __init__(self, scene, extras_only):
        self.scene, self.extras_only = scene, extras_only

    def trace(self, target, starts, dirs):
        a = self.scene.trace(TRACE_NEAREST, starts, dirs)
        b = self.extras_only.trace(TRACE_ROOT_TREE, starts, dirs)
        ha, hb = a["hit"].astype(bool), b["hit"].astype(bool)
        fa = np.where(ha, a["ray_frac"], np.inf)
        fb = np.where(hb, b["ray_frac"], np.inf)
        tri = ha & (~hb | (fa < fb))
        res = dict(hit=(ha | hb).astype(np.uint8), ray_frac=np.where(tri, fa, fb))
        for k in ("pos", "normal"):
            res[k] = np.where(tri[:, None], a[k], b[k])
        res["color"] = np.where(tri, a["color"], b["color"])
        return res


def directions(ints, nrm):
    """dirs [n, 3] from the 3 n InternalSample() values `ints` and the normals."""
    nrm = np.asarray(nrm, dtype=np.float64).reshape(-1, 3)
    u = np.asarray(ints, dtype=np.int64).astype(np.float64).reshape(-1, 3) * (1.0 / 2147483647.0)
    d = u * 2 - 1
    with np.errstate(invalid="ignore", over="ignore"):
        dn = (d[:, 0] * nrm[:, 0] + d[:, 1] * nrm[:, 1]) + d[:, 2] * nrm[:, 2]
    d = np.where((dn < 0.0)[:, None], -d, d)
    inv = 1.0 / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return d * inv[:, None]


def draws(seed, first_sample, n):
    """InternalSample() number 3 first_sample .. 3 (first_sample + n) - 1 of Random(seed), one after the other."""
    return orc.Random(seed).NextInts(3 * (int(first_sample) + int(n)))[3 * int(first_sample):]


def colour_step(incoming, frac, own):
    """out uint32 [n] from the incoming and own packed colours and frac = n . d."""
    with np.errstate(invalid="ignore", over="ignore"):
        out = _unpack(incoming) * frac[:, None] + _unpack(own)
        big = (out > 1.0).any(axis=1)
        il = 1.0 / np.sqrt((out[:, 0] * out[:, 0] + out[:, 1] * out[:, 1]) + out[:, 2] * out[:, 2])
        out = np.where(big[:, None], out * il[:, None], out) * 255.0
        ok = (out > -2147483649.0) & (out < 2147483648.0)                          # C# unchecked (byte)(double); NaN / huge: 0
        by = np.where(ok, out, 0.0).astype(np.int64) & 255
    return (0xFF000000 | (by[:, 0] << 16) | (by[:, 1] << 8) | by[:, 2]).astype(np.uint32), big


def path_points(scene, target, frame, pos, nrm, color, first_sample=0, inf_scene=None, ints=None, info=None):
    """(out uint32 [n], incoming uint32 [n], dirs float64 [n, 3]).  `scene` answers trace(target, starts, dirs) for the finite origins,
    `inf_scene` (default: scene) trace(TRACE_ROOT_TREE, ...) for the infinite ones.  color None: every point 0xFFFFFFFF.  `ints`: the
    call's 3 n draws when the caller has them already.  `info` (a dict) receives hit [n] and normalised [n]."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, dtype=np.float64).reshape(-1, 3)
    n = pos.shape[0]
    own = np.full(n, WHITE, dtype=np.uint32) if color is None else np.asarray(color, dtype=np.uint32)
    d = directions(draws(frame.random_seed, first_sample, n) if ints is None else ints, nrm)
    with np.errstate(invalid="ignore", over="ignore"):
        origin = pos + nrm * OFFSET
    has_nan = np.isnan(origin).any(axis=1)
    has_inf = np.isinf(origin).any(axis=1) & ~has_nan
    finite = ~has_nan & ~has_inf
    hit = np.zeros(n, dtype=bool)
    c2 = np.zeros(n, dtype=np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for sel, sc, tg in ((finite, scene, target), (has_inf, inf_scene if inf_scene is not None else scene, TRACE_ROOT_TREE)):
            if not sel.any():
                continue
            second = sc.trace(tg, origin[sel], d[sel])
            col = second["color"]
            if frame.flags & orc.F_SHADING:
                col = orc.shade_points(frame, second["pos"], second["normal"], col)
            hit[sel] = second["hit"].astype(bool)
            c2[sel] = col
        incoming = np.where(hit, c2, 0).astype(np.uint32)
        frac = (nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1]) + nrm[:, 2] * d[:, 2]
    out, big = colour_step(incoming, frac, own)
    if info is not None:
        info["hit"], info["normalised"] = hit, big
    return out, incoming, d
