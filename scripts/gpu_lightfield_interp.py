"""Quad-linear interpolation of the colour light field (sr_set_light_field_interpolation) measured on the GPU, on the unit-cube scene of the
benchmark (SR_MODE_BVH, N = 64):

    python scripts/gpu_lightfield_interp.py [--out profiles/lightfield_interp/frames.json]

One child process with a time limit of its own, `reps` timed repetitions after a warm-up; the variants alternate inside every repetition, so
that drift of the shared machine hits them alike.  At res x res, one sample per pixel:
  warm    on the baked table (look-ups only): the plain frame without the light field, the nearest-lookup light-field frame, the interpolated
          frame with the lookup handing base cell and fractions to the apply kernel (production) and with the apply kernel computing them
          again (SR_DBG_KERNEL_SWITCH 39).  Recorded: the frame's time and the HIP event times per kernel, and whether both variants drew the same frame.
  cold    on an empty table (lazy fill): the nearest-lookup frame and the interpolated frame, with the number of cells each filled.
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
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["frames"], help="(internal) run the step in this process")
args = ap.parse_args()

RECOMPUTE = 39                               # SR_DBG_KERNEL_SWITCH: k_lfi_apply computes base cell and fractions again


def stats(xs):
    import numpy as np
    t = np.array(xs, dtype=np.float64)
    return {"median": round(float(np.median(t)), 3), "min": round(float(t.min()), 3), "max": round(float(t.max()), 3), "n": int(t.size)}


def frame(res, light_field):
    import numpy as np
    import softray_amd as sa
    f = sa.Frame()
    f.width = f.height = res
    f.start_row, f.end_row = 0, res - 1
    f.sub_pixel_res = 1
    f.background_argb = 0xff00ff
    f.flags = sa.F_SHADING | sa.F_POINT_LIGHT | sa.F_SPECULAR | (sa.F_LIGHT_FIELD if light_field else 0)
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


def step_frames():
    import numpy as np
    import softray_amd as sa
    import torch
    g = sa.GpuScene(0)
    g.set_triangles(*sa.unit_cube_scene(args.triangles))
    g.build((sa.MODE_BVH,))
    g.debug_set(sa._lib.DBG_KERNEL_TIMING, 1)
    g.light_field_res = args.lf_res
    res = args.res
    surface = torch.zeros(res * res, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    fl, fp = frame(res, True), frame(res, False)

    def timed(f, interpolate, hook=None):
        g.light_field_interpolation = interpolate
        if hook is not None:
            g.debug_set(sa._lib.DBG_KERNEL_SWITCH, hook)
        try:
            g.reset_kernel_times()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.render_device(f, surface.data_ptr(), stream)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
        finally:
            if hook is not None:
                g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
        return ms, {k: round(v[0], 3) for k, v in g.kernel_times().items()}

    warm = {"plain": (fp, False, None), "lightfield_nearest": (fl, False, None), "lightfield_interpolated": (fl, True, None),
            "lightfield_interpolated_recompute": (fl, True, RECOMPUTE)}
    cold = {"lightfield_nearest": (fl, False, None), "lightfield_interpolated": (fl, True, None)}
    filled = {}
    for name, (f, interp, hook) in cold.items():                       # warm-up of every kernel and every scratch buffer; the cells a cold frame fills
        g.reset_light_field()
        timed(f, interp, hook)
        filled[name] = int(np.count_nonzero(g.get_light_field()))
    g.reset_light_field()
    g.light_field_interpolation = False
    total = g.bake_light_field(fl)
    digests = {}
    for name, (f, interp, hook) in warm.items():
        timed(f, interp, hook)
        px = surface.cpu().numpy().view(np.uint32)
        digests[name] = (int(px.astype(np.uint64).sum()), int(np.bitwise_xor.reduce(px)))
    times, kernels = {k: [] for k in warm}, {}
    for _ in range(args.reps):
        for name, (f, interp, hook) in warm.items():
            ms, kernels[name] = timed(f, interp, hook)
            times[name].append(ms)
    ctimes, ckernels = {k: [] for k in cold}, {}
    for _ in range(args.reps):
        for name, (f, interp, hook) in cold.items():
            g.reset_light_field()
            torch.cuda.synchronize()
            ms, ckernels[name] = timed(f, interp, hook)
            ctimes[name].append(ms)
    g.light_field_interpolation = False
    return {"res": res, "triangles": args.triangles, "light_field_res": args.lf_res, "entries_baked": total,
            "both_hand_over_variants_draw_the_same_frame": digests["lightfield_interpolated"] == digests["lightfield_interpolated_recompute"],
            "interpolated_frame_differs_from_nearest": digests["lightfield_interpolated"] != digests["lightfield_nearest"],
            "warm_frame_ms": {k: stats(v) for k, v in times.items()}, "warm_kernels_last_rep_ms": kernels,
            "cold_frame_ms": {k: stats(v) for k, v in ctimes.items()}, "cold_kernels_last_rep_ms": ckernels, "cold_cells_filled": filled}


if args.step:
    print("RESULT " + json.dumps(step_frames()))
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
    return doc


doc = {"frames": child("frames", 300.0)}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
