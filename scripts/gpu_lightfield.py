"""The colour light field (SR_F_LIGHT_FIELD) measured on the GPU, on the unit-cube scene of the benchmark (SR_MODE_BVH, shading on, N = 64):

    python scripts/gpu_lightfield.py [--out profiles/lightfield/frames.json]

One child process with a time limit of its own renders, `reps` times each after a warm-up:
  cold    the light-field frame on an empty cache (sr_reset_light_field before every timed frame: the 256 MiB table is zeroed, the frame's
          cells are claimed and their canonical rays traced)
  warm    the same frame again (every cell is there: lookup and apply only)
  plain   the frame of the same commit without the bit, for scale
and records the cells a cold frame fills, the three kernels' own times from the library's HIP event pairs, and canonical rays per second
(cells / k_lf_fill's time).  A failing or overrunning child ends the script: nothing more is started on the GPU after it.
`--step frame` (internal, also what a profiler is pointed at: `rocprofv3 --kernel-trace --stats -- python scripts/gpu_lightfield.py --step frame`)
renders one warm-up, one cold and one warm frame.
Frames are timed with the host clock around sr_render_device into a torch tensor + synchronise.  Reads neither the reference nor anything
the oracle built.
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
ap.add_argument("--step", default=None, choices=["frames", "frame"], help="(internal) run one step in this process")
args = ap.parse_args()
KERNELS = ("k_lf_lookup", "k_lf_fill", "k_lf_apply")


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
    return g


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


def timed(g, f, surface, stream):
    """One device frame, host clock from the call to the end of everything it enqueued; the three kernels' event times of that frame."""
    import torch
    g.reset_kernel_times()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.render_device(f, surface.data_ptr(), stream)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    kt = g.kernel_times()
    return ms, [kt.get(k, (0.0, 0))[0] for k in KERNELS]


def cells_of(g, f):
    """Cells a cold frame fills = its secondary rays (blocking call with statistics)."""
    g.reset_light_field()
    g.render(f)
    return int(g.ray_stats()[4])


def step_frames():
    import numpy as np
    import torch
    g = make_scene()
    res = args.res
    surface = torch.zeros(res * res, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    fl, fp = frame(res, True), frame(res, False)
    cells = cells_of(g, fl)                                           # warm-up of every kernel and of the scratch, and the count
    timed(g, fp, surface, stream)
    cold, warm, plain = [], [], []
    kc, kw = [], []
    for _ in range(args.reps):
        g.reset_light_field()
        ms, k = timed(g, fl, surface, stream)
        cold.append(ms); kc.append(k)
        ms, k = timed(g, fl, surface, stream)
        warm.append(ms); kw.append(k)
        plain.append(timed(g, fp, surface, stream)[0])
    kc, kw = np.array(kc), np.array(kw)
    fill_ms = float(np.median(kc[:, 1]))
    doc = {"res": res, "triangles": args.triangles, "light_field_res": args.lf_res, "samples": res * res, "cells_filled_cold": cells,
           "cold_frame_ms": stats(cold), "warm_frame_ms": stats(warm), "plain_frame_ms": stats(plain),
           "canonical_rays_per_s": round(cells / (fill_ms * 1e-3), 0) if fill_ms > 0 else 0}
    for i, k in enumerate(KERNELS):
        doc[k + "_cold_ms"] = stats(kc[:, i])
        doc[k + "_warm_ms"] = stats(kw[:, i])
    return doc


def step_frame():
    import torch
    g = make_scene()
    res = args.res
    surface = torch.zeros(res * res, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    fl = frame(res, True)
    cells = cells_of(g, fl)
    g.reset_light_field()
    cold, kc = timed(g, fl, surface, stream)
    warm, kw = timed(g, fl, surface, stream)
    return {"res": res, "triangles": args.triangles, "light_field_res": args.lf_res, "cells_filled_cold": cells, "cold_frame_ms": round(cold, 3),
            "warm_frame_ms": round(warm, 3), "kernels_cold_ms": dict(zip(KERNELS, [round(x, 3) for x in kc])),
            "kernels_warm_ms": dict(zip(KERNELS, [round(x, 3) for x in kw]))}


if args.step:
    print("RESULT " + json.dumps({"frames": step_frames, "frame": step_frame}[args.step]()))
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


doc = {"frames": child("frames", 600.0)}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
