"""The triangle-index light field (sr_set_light_field_triangles) measured on the GPU, on the unit-cube scene of the benchmark (N = 64):

    python scripts/gpu_lightfield_tri.py [--out profiles/lightfield_tri/frames.json]

One child process per step, each with a time limit of its own; `reps` timed repetitions after a warm-up, the variants alternating inside every
repetition, so that drift of the shared machine hits them alike.  At res x res, one sample per pixel, reference tree at max_depth / 25:
  bvh       SR_MODE_BVH, reference tree at the default depth 15: the bake of the triangle table; on the baked table the plain frame, the
            nearest-lookup colour light-field frame (its own baked table), the triangle frame (production: all three stages in k_lft_hit) and the same with
            stage 3 as a compact list for k_lft_trace (SR_DBG_KERNEL_SWITCH 43), with the stage census and the HIP event times per kernel; then the cold lazy-fill
            frames of both light fields on empty tables
  bvh_deep  the same scene with the reference tree rebuilt at --deep-depth (the table is kept: sr_build does not drop it): the triangle frames again --
            stage 2 searches one leaf of that tree, so its cost is the leaf's size
  tree      SR_MODE_REF_TREE (the literal method), fewer repetitions: its full traces walk the reference tree, so only the first 2^22 entries are
            baked (one sixteenth of the table; labelled so) and the warm frames run on the table a cold frame filled lazily
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--deep-depth", type=int, default=24, help="max_depth of the reference tree in the bvh_deep step")
ap.add_argument("--steps", default="bvh,bvh_deep,tree")
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["bvh", "bvh_deep", "tree"], help="(internal) run the step in this process")
args = ap.parse_args()

SPLIT = 43                                   # SR_DBG_KERNEL_SWITCH: stage 3 in k_lft_trace instead of inside k_lft_hit


def stats(xs):
    import numpy as np
    t = np.array(xs, dtype=np.float64)
    return {"median": round(float(np.median(t)), 3), "min": round(float(t.min()), 3), "max": round(float(t.max()), 3), "n": int(t.size)}


def frame(res, light_field, mode):
    import numpy as np
    import softray_amd as sa
    f = sa.Frame()
    f.width = f.height = res
    f.start_row, f.end_row = 0, res - 1
    f.sub_pixel_res = 1
    f.background_argb = 0xff00ff
    f.flags = sa.F_SHADING | sa.F_POINT_LIGHT | sa.F_SPECULAR | (sa.F_LIGHT_FIELD if light_field else 0)
    f.trace_mode = mode
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


def run_step(step):
    import numpy as np
    import softray_amd as sa
    import torch
    mode = sa.MODE_REF_TREE if step == "tree" else sa.MODE_BVH
    depth = args.deep_depth if step == "bvh_deep" else 0
    reps = max(1, args.reps // 2) if step == "tree" else args.reps
    g = sa.GpuScene(0)
    g.set_triangles(*sa.unit_cube_scene(args.triangles))
    t0 = time.perf_counter()
    g.build((sa.MODE_REF_TREE,), depth, 0)
    tree_build_s = time.perf_counter() - t0
    if mode == sa.MODE_BVH:
        g.build((sa.MODE_BVH,))
    g.debug_set(sa._lib.DBG_KERNEL_TIMING, 1)
    g.light_field_res = args.lf_res
    res = args.res
    surface = torch.zeros(res * res, dtype=torch.int32, device="cuda:0")
    counters = torch.zeros(24, dtype=torch.int64, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    fl, fp = frame(res, True, mode), frame(res, False, mode)

    def timed(f, tris, hook=None, with_stats=False):
        g.light_field_triangles = tris
        if hook is not None:
            g.debug_set(sa._lib.DBG_KERNEL_SWITCH, hook)
        try:
            g.reset_kernel_times()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.render_device(f, surface.data_ptr(), stream, counters.data_ptr() if with_stats else None)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
        finally:
            if hook is not None:
                g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
        return ms, {k: round(v[0], 3) for k, v in g.kernel_times().items()}

    def digest():
        px = surface.cpu().numpy().view(np.uint32)
        return (int(px.astype(np.uint64).sum()), int(np.bitwise_xor.reduce(px)))

    doc = {"step": step, "res": res, "triangles": args.triangles, "light_field_res": args.lf_res, "tree_stats": g.tree_stats(),
           "tree_build_host_s": round(tree_build_s, 2), "reps": reps}
    warm = {"plain": (fp, False, None), "triangles": (fl, True, None), "triangles_split": (fl, True, SPLIT)}
    cold = {"triangles": (fl, True, None)}
    if step == "bvh":
        warm["colours_nearest"] = (fl, False, None)
        cold["colours_nearest"] = (fl, False, None)
    if step == "bvh_deep":
        del warm["plain"]
        cold = {}
    # ---- warm-up of every kernel and scratch buffer on empty tables; the cells a cold frame fills ----
    filled = {}
    for name, (f, tris, hook) in cold.items():
        g.reset_light_field()
        timed(f, tris, hook)
        filled[name] = int(np.count_nonzero(g.get_light_field_tris() if tris else g.get_light_field()))
    # ---- the bakes ----
    bake_ms, bake_kernels = [], {}
    bake_count = (1 << 22) if step == "tree" else None      # (None: the whole table)
    for _ in range(1 if step == "tree" else 3):
        g.reset_light_field()
        g.light_field_triangles = True
        g.reset_kernel_times()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        total = g.bake_light_field(fl, 0, bake_count)
        bake_ms.append((time.perf_counter() - t0) * 1e3)
        bake_kernels = {k: round(v[0], 3) for k, v in g.kernel_times().items()}
    doc["bake_triangle_table_ms"] = stats(bake_ms)
    doc["bake_kernels_last_rep_ms"] = bake_kernels
    doc["entries_baked"] = total
    if step == "tree":                                      # the warm frames' table: what a cold frame fills
        g.reset_light_field()
        timed(fl, True)
    table = g.get_light_field_tris()
    doc["entries_naming_a_triangle"] = int(np.count_nonzero(table >= 2))
    del table
    if "colours_nearest" in warm:
        g.light_field_triangles = False
        g.bake_light_field(fl)
    # ---- warm frames: look-ups only ----
    digests, census = {}, {}
    for name, (f, tris, hook) in warm.items():
        timed(f, tris, hook, with_stats=True)
        digests[name] = digest()
        c = [int(x) for x in counters.cpu().numpy()]
        census[name] = {"samples": c[0], "triangle_tests": c[1], "nodes": c[2], "leaves": c[3], "cells_filled": c[4],
                        "no_candidate": c[20], "stage1": c[21], "stage2": c[22], "stage3": c[23]}
    times, kernels = {k: [] for k in warm}, {}
    for _ in range(reps):
        for name, (f, tris, hook) in warm.items():
            ms, kernels[name] = timed(f, tris, hook)
            times[name].append(ms)
    doc["split_and_production_draw_the_same_frame"] = digests["triangles"] == digests["triangles_split"]
    doc["split_and_production_count_the_same"] = census["triangles"] == census["triangles_split"]
    if "plain" in digests:
        px_plain_sum = digests["plain"]
        doc["triangle_frame_equals_plain_frame"] = digests["triangles"] == px_plain_sum
    doc["warm_census"] = {"triangles": census["triangles"]}
    doc["warm_frame_ms"] = {k: stats(v) for k, v in times.items()}
    doc["warm_kernels_last_rep_ms"] = kernels
    # ---- cold frames: empty tables ----
    ctimes, ckernels = {k: [] for k in cold}, {}
    for _ in range(reps):
        for name, (f, tris, hook) in cold.items():
            g.reset_light_field()
            torch.cuda.synchronize()
            ms, ckernels[name] = timed(f, tris, hook)
            ctimes[name].append(ms)
    if cold:
        doc["cold_frame_ms"] = {k: stats(v) for k, v in ctimes.items()}
        doc["cold_kernels_last_rep_ms"] = ckernels
        doc["cold_cells_filled"] = filled
    g.light_field_triangles = False
    return doc


if args.step:
    print("RESULT " + json.dumps(run_step(args.step)))
    sys.exit(0)


def child(step, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--triangles", str(args.triangles), "--res", str(args.res),
           "--lf-res", str(args.lf_res), "--reps", str(args.reps), "--deep-depth", str(args.deep_depth)]
    print("step: %s, time limit %.0f s" % (step, limit), flush=True)
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)          # TimeoutExpired ends the script: nothing is started after it
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("step %s failed with exit status %d: stopping here" % (step, r.returncode))
    doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    doc["step_wall_s"] = round(time.perf_counter() - t0, 1)
    return doc


LIMITS = {"bvh": 300.0, "bvh_deep": 300.0, "tree": 420.0}
doc = {}
for step in args.steps.split(","):
    doc[step] = child(step, LIMITS[step])
    print(json.dumps({step: doc[step]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
