"""What frame-sequence tests share: one GpuScene and one oracle scene holding the same geometry (Pair), the frame of a pose and a
model-space light, the two frame sizes and the three lights of tests/test_gpu_sequences.py."""
import os

import numpy as np

import softray_amd as sa
from helpers import make_frame, orc

NCPU = min(16, os.cpu_count() or 8)
SMALL = dict(res=(96, 72), samples=33, hook=None)
PERSISTENT = dict(res=(512, 384), samples=5, hook=831)        # the shaft walk's grid shrunk to one workgroup per CU (as big_case_of)
L_OUT = (0.9, 1.1, -0.8)                                      # model-space lights: outside the box on all axes / inside / outside on x only
L_IN = (0.1, -0.2, 0.15)
L_X = (-0.95, 0.2, -0.1)


def model_origin_and_light(f):
    """prepare_frame's camera origin and light position in model space, with its arithmetic (sr_api.cpp)."""
    it = [f.inv_transform[i] for i in range(12)]
    lp = [f.light_pos_view[i] for i in range(3)]
    origin = tuple(0.0 * it[4 * r] + 0.0 * it[4 * r + 1] + (-f.position_z) * it[4 * r + 2] for r in range(3))
    light = tuple(lp[0] * it[4 * r] + lp[1] * it[4 * r + 1] + lp[2] * it[4 * r + 2] + it[4 * r + 3] for r in range(3))
    return origin, light


def set_model_light(f, m):
    t = [f.transform[i] for i in range(12)]
    for r in range(3):
        f.light_pos_view[r] = t[4 * r] * m[0] + t[4 * r + 1] * m[1] + t[4 * r + 2] * m[2] + t[4 * r + 3]


class Pair:
    """One GpuScene and one oracle Scene holding the same geometry; render() compares a frame on both.  The oracle's results are kept
    per (geometry, frame, offset table) so that a frame that repeats costs one render (not for static-shadow frames: renderer state)."""

    def __init__(self, v9, argb, lo, hi, hook=None, devices=None, modes=(sa.MODE_BVH, sa.MODE_REF_TREE)):
        self.g = sa.GpuScene(devices=devices) if devices else sa.GpuScene(0)
        self.o = orc.Scene()
        self.modes = modes
        if hook:
            self.g.debug_set(sa._lib.DBG_KERNEL_SWITCH, hook)
        self.cache = {}
        self.load(v9, argb, lo, hi)

    def load(self, v9, argb, lo, hi):
        for s in (self.g, self.o):
            s.set_triangles(v9, argb, lo, hi)
        self.g.build(self.modes)
        assert self.o.build_tree() == 0
        self.geometry = (len(v9), float(np.asarray(v9).sum()), ())

    def extra(self, prims):
        self.g.set_extra(prims)
        self.o.set_extra(prims)
        self.geometry = self.geometry[:2] + (repr(prims),)

    def want(self, f, table):
        key = None
        if not (f.flags & orc.F_STATIC_SHADOWS):
            g = orc.Frame.from_buffer_copy(bytes(f))
            g.area_light_offsets = None
            key = (self.geometry, bytes(g), None if table is None else table.tobytes())
            if key in self.cache:
                return self.cache[key]
        w, _ = self.o.render(f, threads=NCPU)
        w = w.copy()
        if key is not None:
            self.cache[key] = w
        return w

    def render(self, f, mode=sa.MODE_BVH, table=None, label=""):
        if table is not None:
            f.area_light_offsets = table.ctypes.data
        want = self.want(f, table)
        sf = sa.Frame.from_buffer_copy(bytes(f))
        sf.trace_mode = mode
        got, _ = self.g.render(sf, stats=False)
        got = got.copy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: %d of %d pixels differ from the oracle (first %s)" % (label, bad.size, want.size, bad[:5])
        return got, self.g.debug_counters()


def frame(size, pose=(135.0, -22.0, 0.0), light=L_OUT, depth=1.5, **kw):
    w, h = kw.pop("res", size["res"])
    kw.setdefault("shadows", True)
    kw.setdefault("shadow_samples", size["samples"])
    f = make_frame(w, h, yaw_deg=pose[0], pitch_deg=pose[1], roll_deg=pose[2], depth=depth, **kw)
    set_model_light(f, light)
    return f
