"""The colour light field with dynamic soft shadows (sr_set_light_field_shadows) measured on the GPU, on the unit-cube scene of the benchmark
(SR_MODE_BVH, N = 64: 4 x 64^4 = 67 M canonical rays, 100 area-light samples per hit point):

    python scripts/gpu_lightfield_shadows.py [--out profiles/lightfield_shadows/shadows.json]

Two child processes, each with a time limit of its own, `reps` timed repetitions each after a warm-up; the variants of a step alternate inside
every repetition, so that drift of the shared machine hits them alike:
  bake    the whole table on an empty light field without shadows, with shadows (the packet shaft walk over 64 consecutive queue entries,
          production) and with shadows under SR_DBG_PER_LANE_SHAFT 1 (private per-lane shaft walks in the first round).  Recorded: the call's
          time, the HIP event times per kernel, the entries written, the hit cells (entries that are not the background) and whether the two
          shadowed variants left the same table.
  frames  at res x res: the plain shadowed frame without the light field (the project's headline path), the light-field frame on the shadowed
          baked table (look-ups only) and the cold lazy-fill frame on an empty table, with the per-lane shaft walks the fill takes
          (production) and with the packet shaft walk (SR_DBG_KERNEL_SWITCH 36).
A failing or overrunning child ends the script: nothing more is started on the GPU after it.  Reads neither the reference nor anything the
oracle built.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=4096)
ap.add_argument("--triangles", type=int, default=1_000_000)
ap.add_argument("--lf-res", type=int, default=64, help="N of the light field's 4 N^4 entries")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["bake", "frames"], help="(internal) run one step in this process")
args = ap.parse_args()


def stats(xs):
    import numpy as np
    t = np.array(xs, dtype=np.float64)
    return {"median": round(float(np.median(t)), 3), "min": round(float(t.min()), 3), "max": round(float(t.max()), 3), "n": int(t.size)}


def make_scene():
    import softray_amd as sa
    g = sa.GpuScene(0)
    g.set_triangles(*sa.unit_cube_scene(args.triangles))
    g.build((sa.MODE_BVH,))
    g.debug_set(sa._lib.DBG_KERNEL_TIMING, 1)
    g.light_field_res = args.lf_res
    g.light_field_shadows = True
    return g


def frame(res, light_field, shadows, shading=True):
    import numpy as np
    import softray_amd as sa
    f = sa.Frame()
    f.width = f.height = res
    f.start_row, f.end_row = 0, res - 1
    f.sub_pixel_res = 1
    f.background_argb = 0xff00ff
    f.flags = (sa.F_SHADING if shading else 0) | sa.F_POINT_LIGHT | sa.F_SPECULAR | (sa.F_LIGHT_FIELD if light_field else 0) | (sa.F_SHADOWS if shadows else 0)
    f.trace_mode = sa.MODE_BVH
    f.random_seed = 1234567890
    t, it = sa.instance_matrices([0.0, 0.0, 1.5], 135.0 / 180.0 * np.pi, -22.0 / 180.0 * np.pi, 0.0)
    for i in range(12):
        f.transform[i] = t[i]
        f.inv_transform[i] = it[i]
    f.position_z = 1.5
    f.fov_depth = sa.default_fov_depth()
    f.focal_depth, f.focal_blur_strength = 2.0, 10.0
    f.ambient, f.shininess = 0.1, 100.0
    d = np.array([-1.0, -1.0, 1.0]) * (1.0 / np.sqrt(3.0))
    p = np.array([0.0, 0.0, 1.5]) - d * 2
    for i in range(3):
        f.light_dir_view[i] = d[i]
        f.light_pos_view[i] = p[i]
    return f


BACKGROUND = 0xFFFF00FF


FILL_PACKET_SHAFT = 36                       # SR_DBG_KERNEL_SWITCH: the lazy fill's shadow stage with the packet shaft walk


def with_hook(g, hook, fn):
    """hook: None, "per_lane_shaft" (SR_DBG_PER_LANE_SHAFT 1) or "fill_packet_shaft" (SR_DBG_KERNEL_SWITCH 36)."""
    import softray_amd as sa
    key, value = {None: (None, 0), "per_lane_shaft": (sa._lib.DBG_PER_LANE_SHAFT, 1), "fill_packet_shaft": (sa._lib.DBG_KERNEL_SWITCH, FILL_PACKET_SHAFT)}[hook]
    if key is not None:
        g.debug_set(key, value)
    try:
        return fn()
    finally:
        if key is not None:
            g.debug_set(key, -1)


def timed_bake(g, f, hook):
    """One whole-table bake on an empty light field: (call ms, event ms per kernel, entries written)."""
    def run():
        g.reset_light_field()
        g.reset_kernel_times()
        t0 = time.perf_counter()
        filled = g.bake_light_field(f)                                # blocks
        return (time.perf_counter() - t0) * 1e3, filled
    ms, filled = with_hook(g, hook, run)
    return ms, {k: (round(v[0], 3), v[1]) for k, v in g.kernel_times().items()}, filled


def digest(g):
    """(sum, xor, hit cells) over the table's entries."""
    import numpy as np
    table = g.get_light_field()
    return int(table.astype(np.uint64).sum()), int(np.bitwise_xor.reduce(table)), int(np.count_nonzero(table != BACKGROUND))


def step_bake():
    g = make_scene()
    total = 4 * args.lf_res ** 4
    variants = {"plain": (False, None), "shadows": (True, None), "shadows_per_lane_shaft": (True, "per_lane_shaft")}
    digests = {}
    for name, (shadows, hook) in variants.items():                    # warm-up of every kernel, and the tables' digests
        _, _, filled = timed_bake(g, frame(16, True, shadows), hook)
        assert filled == total, (filled, total)
        digests[name] = digest(g)
    call, kernels = {n: [] for n in variants}, {}
    for _ in range(args.reps):
        for name, (shadows, hook) in variants.items():
            ms, kt, filled = timed_bake(g, frame(16, True, shadows), hook)
            assert filled == total
            call[name].append(ms); kernels[name] = kt
    doc = {"triangles": args.triangles, "light_field_res": args.lf_res, "entries": total, "hit_cells": digests["shadows"][2],
           "same_table_both_shaft_walks": digests["shadows"] == digests["shadows_per_lane_shaft"],
           "shadows_change_the_table": digests["shadows"][:2] != digests["plain"][:2], "variants": {}}
    for name in variants:
        doc["variants"][name] = {"call_ms": stats(call[name]), "kernels_last_rep_ms_and_launches": kernels[name]}
    return doc


def timed_frame(g, f, surface, stream, hook=None):
    import torch

    def run():
        g.reset_kernel_times()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.render_device(f, surface.data_ptr(), stream)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    ms = with_hook(g, hook, run)
    return ms, {k: round(v[0], 3) for k, v in g.kernel_times().items()}


def step_frames():
    import torch
    g = make_scene()
    res = args.res
    surface = torch.zeros(res * res, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    fl, fp = frame(res, True, True), frame(res, False, True)
    timed_frame(g, fp, surface, stream)                               # warm-up of every kernel
    timed_frame(g, fl, surface, stream)
    g.reset_light_field()
    timed_frame(g, fl, surface, stream, "fill_packet_shaft")
    g.reset_light_field()
    g.bake_light_field(fl)
    times = {k: [] for k in ("plain_shadowed", "lightfield_on_baked_table", "lightfield_cold_lazy", "lightfield_cold_lazy_packet_shaft")}
    kernels = {}
    for _ in range(args.reps):
        ms, kernels["plain_shadowed"] = timed_frame(g, fp, surface, stream)
        times["plain_shadowed"].append(ms)
        ms, kernels["lightfield_on_baked_table"] = timed_frame(g, fl, surface, stream)
        times["lightfield_on_baked_table"].append(ms)
    for _ in range(args.reps):
        g.reset_light_field()
        ms, kernels["lightfield_cold_lazy"] = timed_frame(g, fl, surface, stream)
        times["lightfield_cold_lazy"].append(ms)
        g.reset_light_field()
        ms, kernels["lightfield_cold_lazy_packet_shaft"] = timed_frame(g, fl, surface, stream, "fill_packet_shaft")
        times["lightfield_cold_lazy_packet_shaft"].append(ms)
    return {"res": res, "triangles": args.triangles, "light_field_res": args.lf_res, "frame_ms": {k: stats(v) for k, v in times.items()},
            "kernels_last_rep_ms": kernels}


if args.step:
    print("RESULT " + json.dumps({"bake": step_bake, "frames": step_frames}[args.step]()))
    sys.exit(0)


def child(step, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--triangles", str(args.triangles), "--res", str(args.res),
           "--lf-res", str(args.lf_res), "--reps", str(args.reps)]
    print("step: %s, time limit %.0f s" % (step, limit), flush=True)
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)          # TimeoutExpired ends the script: nothing is started after it
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("step %s failed with exit status %d: stopping here" % (step, r.returncode))
    doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    doc["step_wall_s"] = round(time.perf_counter() - t0, 1)
    print(json.dumps(doc), flush=True)
    return doc


doc = {"bake": child("bake", 420.0)}
doc["frames"] = child("frames", 300.0)
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
