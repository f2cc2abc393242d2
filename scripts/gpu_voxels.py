"""Voxel-grid rendering (SR_F_VOXELS) measured on the GPU: the voxeliser on the unit-cube scene and the 4096^2 voxel frame (shading on,
one sample per pixel and 2x2 sub-pixel samples) next to the plain SR_MODE_BVH frame of the same scene from the same run.

    python scripts/gpu_voxels.py [--voxel-res N] [--out profiles/voxel_res/res<N>.json]

--voxel-res N (default 64; `--res` is the frame's edge) sets the grid size with sr_set_voxel_res.  Above 64 the second schedule of the walk
is SR_DBG_KERNEL_SWITCH 42 (one level, the row-major occupancy bits in global memory) instead of 41 (the colour table).
--only voxelise|frames runs one of the steps on --triangles, --no-plain leaves the SR_MODE_BVH frames (and their sr_build) out, and
--root DIR imports softray_amd from another checkout: the parent commit's build next to this one for an A/B at 64.

Every step is a child process of its own with a time limit of its own, and a step that fails or runs out of time ends the script (nothing
more is started on the GPU after it):
  1. voxelise 200 k triangles                   limit 300 s (a fixed allowance: torch import, scene generation, the first HIP calls)
  2. voxelise --triangles (1 M) triangles       limit 120 s + 20 x the wall time step 1 measured for ONE build of 200 k: the pairs grow
                                                5-fold, so a voxeliser that is linear in the pairs stays four times inside it; the only
                                                condition on this step is that it completes inside that limit
  3. the frames                                 limit 600 s
Voxelisation: `reps` builds, each after sr_set_triangles has dropped the grid; per build the wall time of sr_build_voxels (it ends in a
device synchronise and includes the first build's upload of the triangles) and the library's own HIP event pair around the voxeliser
(count, scan, the read-back of the pair count, emit, sort, per-cell sums).  Frames: device frames (sr_render_device into a torch tensor),
variants alternating, HIP events around each frame, warm-up first, median and spread over the repetitions.  The walk is measured twice:
on its default schedule (occupancy bits in LDS; two levels above 64) and on the second one (SR_DBG_KERNEL_SWITCH 41: the colour table in global
memory at every step; above 64, 42: the row-major occupancy bits in global memory).
Reads neither the reference nor anything the oracle built: the scene comes from the library's seeded generator.
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
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--voxel-res", type=int, default=64, help="N of the N^3 grid (sr_set_voxel_res)")
ap.add_argument("--only", default=None, choices=["voxelise", "frames"], help="run only this step (on --triangles)")
ap.add_argument("--no-plain", action="store_true", help="no SR_MODE_BVH frames next to the voxel frames")
ap.add_argument("--root", default=None, help="import softray_amd from this checkout instead of the script's own")
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["voxelise", "frames"], help="(internal) run one step in this process")
args = ap.parse_args()
if args.root:
    sys.path.insert(0, os.path.abspath(args.root))
HOOK = 42 if args.voxel_res > 64 else 41
HOOK_NAME = "flat_mask" if args.voxel_res > 64 else "global_table"


def set_res(g):
    if args.voxel_res != 64:                                          # (64 is the default: a library without sr_set_voxel_res runs the script too)
        g.voxel_res = args.voxel_res


def pair_count(v9, n):
    """(cell, triangle) pairs of the grid: per axis the cells with max >= plane(k) and min <= plane(k + 1), planes as FP64 computes k / n - 0.5."""
    import numpy as np
    planes = np.arange(n + 1, dtype=np.float64) / np.float64(n) - 0.5
    v = np.asarray(v9, dtype=np.float64).reshape(-1, 3, 3)
    total = np.ones(v.shape[0], dtype=np.int64)
    for a in range(3):
        hi = np.minimum(np.searchsorted(planes, v[:, :, a].max(axis=1), side="right") - 1, n - 1)
        lo = np.searchsorted(planes[1:], v[:, :, a].min(axis=1), side="left")
        total *= np.maximum(0, hi - lo + 1)
    return int(total.sum())


def stats(xs):
    import numpy as np
    t = np.array(xs, dtype=np.float64)
    return {"median": round(float(np.median(t)), 3), "min": round(float(t.min()), 3), "max": round(float(t.max()), 3), "n": int(t.size)}


def step_voxelise():
    import numpy as np
    import softray_amd as sa
    v9, argb, bmin, bmax = sa.unit_cube_scene(args.triangles)
    g = sa.GpuScene(0)
    set_res(g)
    g.debug_set(sa._lib.DBG_KERNEL_TIMING, 1)
    wall, dev = [], []
    for i in range(args.reps + 1):                                    # the first build also uploads the triangles and loads the code objects: warm-up
        g.set_triangles(v9, argb, bmin, bmax)
        g.reset_kernel_times()
        t0 = time.perf_counter()
        g.build_voxels()                                              # ends in a device synchronise
        t1 = time.perf_counter()
        if i:
            wall.append((t1 - t0) * 1e3)
            dev.append(g.kernel_times()["voxelise"][0])
        else:
            first = (t1 - t0) * 1e3
    colors, _ = g.get_voxels()
    return {"triangles": args.triangles, "voxel_res": args.voxel_res, "pairs": pair_count(v9, args.voxel_res), "filled_cells": int(np.count_nonzero(colors)),
            "first_build_wall_ms": round(first, 3),
            "build_wall_ms": stats(wall), "voxeliser_events_ms": stats(dev)}


def step_frames():
    import numpy as np
    import torch
    import softray_amd as sa
    res = args.res
    g = sa.GpuScene(0)
    g.set_triangles(*sa.unit_cube_scene(args.triangles))
    set_res(g)
    if not args.no_plain:
        g.build((sa.MODE_BVH,))
    g.build_voxels()
    table = sa.GpuScene(0)                                            # the same grid on the walk's second schedule (hook 41 / 42)
    table.set_triangles(*sa.unit_cube_scene(args.triangles))
    set_res(table)
    table.build_voxels()
    table.debug_set(sa._lib.DBG_KERNEL_SWITCH, HOOK)

    def frame(voxels, sub):
        f = sa.Frame()
        f.width = f.height = res
        f.start_row, f.end_row = 0, res - 1
        f.sub_pixel_res = sub
        f.background_argb = 0xff00ff
        f.flags = sa.F_SHADING | sa.F_POINT_LIGHT | sa.F_SPECULAR | (sa.F_VOXELS if voxels else 0)
        f.trace_mode = sa.MODE_BVH
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

    variants = [("voxels_1spp", g, frame(True, 1)), ("voxels_2x2", g, frame(True, 2)),
                ("voxels_1spp_" + HOOK_NAME, table, frame(True, 1)), ("voxels_2x2_" + HOOK_NAME, table, frame(True, 2))]
    if not args.no_plain:
        variants += [("plain_bvh_1spp", g, frame(False, 1)), ("plain_bvh_2x2", g, frame(False, 2))]
    surface = torch.zeros(res * res, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    images = {}
    for _ in range(3):                                                # warm-up: code objects, scratch, per-origin records
        for n, s, f in variants:
            s.render_device(f, surface.data_ptr(), stream)
            torch.cuda.synchronize()
            images[n] = surface.cpu().numpy().copy()
    same = bool(np.array_equal(images["voxels_1spp"], images["voxels_1spp_" + HOOK_NAME]) and
                np.array_equal(images["voxels_2x2"], images["voxels_2x2_" + HOOK_NAME]))
    shown = float(np.count_nonzero(images["voxels_1spp"].view(np.uint32) != 0xffff00ff)) / images["voxels_1spp"].size
    times = {n: [] for n, _, _ in variants}
    for _ in range(args.reps):
        for n, s, f in variants:                                      # alternating: drift hits all alike
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            s.render_device(f, surface.data_ptr(), stream)
            b.record()
            b.synchronize()
            times[n].append(a.elapsed_time(b))
    import zlib
    return {"res": res, "triangles": args.triangles, "voxel_res": args.voxel_res, "second_schedule_hook": HOOK,
            "frames_ms": {n: stats(times[n]) for n, _, _ in variants},
            "frame_crc": {n: zlib.crc32(images[n].tobytes()) & 0xFFFFFFFF for n in ("voxels_1spp", "voxels_2x2")},
            "both_schedules_frames_identical": same, "voxel_frame_non_background_share": round(shown, 4)}


if args.step:
    print("RESULT " + json.dumps(step_voxelise() if args.step == "voxelise" else step_frames()))
    sys.exit(0)


def child(step, triangles, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--triangles", str(triangles), "--res", str(args.res), "--reps", str(args.reps),
           "--voxel-res", str(args.voxel_res)] + (["--no-plain"] if args.no_plain else []) + (["--root", args.root] if args.root else [])
    print("step: %s, %d triangles, time limit %.0f s" % (step, triangles, limit), flush=True)
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)          # TimeoutExpired ends the script: nothing is started after it
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("step %s failed with exit status %d: stopping here" % (step, r.returncode))
    doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    doc["step_wall_s"] = round(time.perf_counter() - t0, 1)
    doc["step_time_limit_s"] = round(limit, 1)
    print(json.dumps(doc), flush=True)
    return doc


doc = {}
if args.only == "voxelise":
    doc["voxelise_%d" % args.triangles] = child("voxelise", args.triangles, 300.0)
elif args.only == "frames":
    doc["frames"] = child("frames", args.triangles, 600.0)
else:
    doc["voxelise_200k"] = child("voxelise", 200_000, 300.0)
    limit = 120.0 + 20.0 * doc["voxelise_200k"]["build_wall_ms"]["median"] / 1e3
    doc["voxelise_%d" % args.triangles] = child("voxelise", args.triangles, limit)
    doc["frames"] = child("frames", args.triangles, 600.0)
print(json.dumps(doc))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
