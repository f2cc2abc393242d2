#!/usr/bin/env python3
"""Model-generated fixtures for the path-traced frames that are too slow to model inside a test.

Runs the CPU model of path tracing (tests/pathtrace_model.py: the oracle's Scene.trace with the global-nearest-hit semantics of
the library's own BVH, its System.Random and its shade_points) over whole frames of the 20 000-triangle unit-cube scene and
writes, per 16-row strip, the CRC-32 (zlib) of the strip's pixels (uint32 ARGB, row-major, little-endian) to
tests/golden/pathtrace/<name>.json.  tests/test_gpu_pathtrace.py renders the same frames through the C ABI in SR_MODE_BVH and
compares every strip.  Scene.trace is single-threaded; the rays are spread over worker processes (every ray is independent, the
hit index is computed afterwards from all of them), so the result does not depend on --procs.

This is test infrastructure (it imports oracle/); nothing under softray_amd/ uses it.  It needs no GPU.

    python scripts/make_pathtrace_fixtures.py cube20k_640x480
    python scripts/make_pathtrace_fixtures.py cube20k_640x480_2xAA
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pathtrace_model as ptm  # noqa: E402
from helpers import make_frame, orc, unit_cube_scene  # noqa: E402

STRIP = 16
OUT_DIR = os.path.join(ROOT, "tests", "golden", "pathtrace")

# name -> triangles of unit_cube_scene, frame size, make_frame keywords (shading on, the RendererTests pose at depth 1.5)
CONFIGS = {
    "cube20k_640x480": dict(n=20000, width=640, height=480, frame=dict(depth=1.5)),
    "cube20k_640x480_2xAA": dict(n=20000, width=640, height=480, frame=dict(depth=1.5, sub_pixel_res=2)),
}


def frame_of(cfg):
    f = make_frame(cfg["width"], cfg["height"], **cfg["frame"])
    f.flags |= ptm.F_PATH_TRACING
    return f


_scene = None


def _trace_chunk(args):
    target, starts, dirs = args
    return _scene.trace(target, starts, dirs)


class ParallelScene:
    """Scene.trace over a pool of forked workers that share the built scene."""

    def __init__(self, pool, procs):
        self.pool, self.procs = pool, procs

    def trace(self, target, starts, dirs):
        n = len(starts)
        cuts = np.linspace(0, n, self.procs * 8 + 1).astype(np.int64)
        parts = self.pool.map(_trace_chunk, [(target, starts[a:b], dirs[a:b]) for a, b in zip(cuts[:-1], cuts[1:]) if b > a])
        return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def main():
    global _scene
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=sorted(CONFIGS))
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    _scene = orc.Scene()
    _scene.set_triangles(*unit_cube_scene(cfg["n"]))
    assert _scene.build_tree() == 0
    f = frame_of(cfg)
    with mp.get_context("fork").Pool(args.procs) as pool:
        px = ptm.render(ParallelScene(pool, args.procs), f, ptm.TRACE_NEAREST)
    px = np.ascontiguousarray(px, dtype="<u4")
    strips = {str(s): zlib.crc32(px[STRIP * s:STRIP * s + STRIP].tobytes()) & 0xFFFFFFFF for s in range((cfg["height"] + STRIP - 1) // STRIP)}
    doc = dict(what="CRC-32 (zlib) of each 16-row strip of the path-traced frame the CPU model renders: uint32 ARGB pixels, row-major, little-endian",
               config=args.config, width=cfg["width"], height=cfg["height"], strip_rows=STRIP, strips=strips,
               scene=dict(generator="unit_cube_scene", triangles=cfg["n"], seed=12345),
               frame=dict(cfg["frame"], shading=True, pose="RendererTests yaw 135 pitch -22", random_seed=int(f.random_seed), concurrency="default (4)",
                          semantics="global nearest hit (Scene.trace target 3)"),
               background_pixels=int(np.count_nonzero(px == ((f.background_argb | 0xFF000000) & 0xFFFFFFFF))),
               command="python scripts/make_pathtrace_fixtures.py " + args.config)
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, args.config + ".json"), "w") as out:
        json.dump(doc, out, indent=1, sort_keys=True)
        out.write("\n")
    print(args.config, "written:", len(strips), "strips,", doc["background_pixels"], "background pixels")


if __name__ == "__main__":
    main()
