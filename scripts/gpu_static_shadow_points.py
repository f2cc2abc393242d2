"""sr_static_shadow_points_device measured on the GPU, on the unit-cube scene of the benchmark (SR_MODE_BVH, the benchmark's pose and light, 100
area-light samples): the points are the hit points of the res x res frame in scan order, taken with sr_render_hits_device.

    python scripts/gpu_static_shadow_points.py [--out profiles/static_shadow_points/points.json]

One child process with a time limit of its own, one session.  After a warm-up of everything, `reps` repetitions in which the variants
alternate, so that drift of the shared machine hits them alike; every call is timed with a HIP event pair on its stream:
  call_cold / call_cold_coherent   sr_reset_shadow_cache, then the call (sorted passes / SR_POINTS_COHERENT): every cell is generated
  call_warm / call_warm_coherent   the call again: every cell is there, nothing is generated
  frame_static_cold / _warm        the static frame of the same pose from an empty / a filled cache (sr_render_device)
  frame_plain                      the frame without shadows: static frame minus plain frame is the frame's own static-shadow cost, the
                                   yardstick for the calls
A last repetition runs with SR_DBG_KERNEL_TIMING for the per-kernel event times of a cold and a warm call.  The cache the cold call leaves is
compared with the cold coherent call's, and the warm outputs with the cold ones.  Reads neither the reference nor anything the oracle built.
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
ap.add_argument("--samples", type=int, default=100)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["measure"], help="(internal) run the measurement in this process")
args = ap.parse_args()

def stats(xs):
    import numpy as np
    t = np.array(xs, dtype=np.float64)
    return {"median": round(float(np.median(t)), 3), "min": round(float(t.min()), 3), "max": round(float(t.max()), 3), "n": int(t.size)}


def frame(res, shadows):
    import numpy as np
    import softray_amd as sa
    f = sa.Frame()
    f.width = f.height = res
    f.start_row, f.end_row = 0, res - 1
    f.sub_pixel_res = 1
    f.background_argb = 0xff00ff
    f.flags = sa.F_SHADING | sa.F_POINT_LIGHT | sa.F_SPECULAR | (sa.F_SHADOWS if shadows else 0) | sa._lib.F_PRIMARY_STATS_ONLY
    f.trace_mode = sa.MODE_BVH
    f.random_seed = 1234567890
    f.shadow_samples = args.samples
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


def measure():
    import numpy as np
    import torch
    import softray_amd as sa
    dev = torch.device("cuda", 0)
    g = sa.GpuScene(0)
    g.set_triangles(*sa.unit_cube_scene(args.triangles))
    g.build((sa.MODE_BVH,))
    res = args.res
    fs, fp = frame(res, True), frame(res, False)
    # the frame's own primary hits, on the device (sr_render_hits_device: the library's ray set-up and its packet walk)
    n_rays = sa.GpuScene.sample_count(fs)
    hit = torch.zeros(n_rays, dtype=torch.uint8, device=dev)
    pos, nrm = torch.zeros((n_rays, 3), dtype=torch.float64, device=dev), torch.zeros((n_rays, 3), dtype=torch.float64, device=dev)
    col = torch.zeros(n_rays, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g.render_hits_device(fs, d_hit=hit.data_ptr(), d_pos=pos.data_ptr(), d_normal=nrm.data_ptr(), d_color=col.data_ptr(),
                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    keep = hit.bool()
    scan = (pos[keep].contiguous(), nrm[keep].contiguous(), col[keep].contiguous())
    n = scan[0].shape[0]
    del pos, nrm, col, hit
    out = torch.zeros(n, dtype=torch.int32, device=dev)
    amount = torch.zeros(n, dtype=torch.uint8, device=dev)
    gen = torch.zeros(1, dtype=torch.int64, device=dev)
    surface = torch.zeros(res * res, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    fst = frame(res, True)
    fst.flags |= sa._lib.F_STATIC_SHADOWS

    def call(cold, coherent):
        if cold:
            g.reset_shadow_cache()
        p, m, c = scan
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.static_shadow_points_device(fs, n, p.data_ptr(), m.data_ptr(), c.data_ptr(), out.data_ptr(), amount.data_ptr(), coherent=coherent, stream=stream,
                                      d_generators_ptr=gen.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def render(f, cold=False):
        if cold:
            g.reset_shadow_cache()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.render_device(f, surface.data_ptr(), stream)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    VARIANTS = {"call_cold": lambda: call(True, False), "call_warm": lambda: call(False, False), "call_cold_coherent": lambda: call(True, True),
                "call_warm_coherent": lambda: call(False, True), "frame_static_cold": lambda: render(fst, True), "frame_static_warm": lambda: render(fst),
                "frame_plain": lambda: render(fp)}
    # warm-up of every variant, and the checks: both cold calls leave one cache and one output, the warm calls generate nothing and repeat the output
    checks = {}
    call(True, False)
    generators = int(gen.cpu()[0])
    ref_out, ref_amount, ref_cache = out.clone(), amount.clone(), g.get_shadow_cache().copy()
    call(False, False)
    checks["warm_generates_nothing"] = int(gen.cpu()[0]) == 0
    checks["warm_output_equals_cold"] = bool(torch.equal(out, ref_out) and torch.equal(amount, ref_amount))
    call(True, True)
    checks["coherent_equals_sorted"] = bool(torch.equal(out, ref_out) and torch.equal(amount, ref_amount)) and bool(np.array_equal(g.get_shadow_cache(), ref_cache))
    call(False, True)
    render(fst, True); render(fst); render(fp)
    frame_cells = int(np.count_nonzero(g.get_shadow_cache()))
    times = {k: [] for k in VARIANTS}
    for _ in range(args.reps):
        for name, fn in VARIANTS.items():
            times[name].append(fn())
    g.debug_set(sa._lib.DBG_KERNEL_TIMING, 1)
    kernels = {}
    for name in ("call_cold", "call_warm", "call_cold_coherent", "call_warm_coherent"):
        g.reset_kernel_times()
        VARIANTS[name]()
        kernels[name] = {k: round(v[0], 3) for k, v in g.kernel_times().items()}
    g.debug_set(sa._lib.DBG_KERNEL_TIMING, -1)
    doc = {"res": res, "triangles": args.triangles, "samples": args.samples, "points": n, "generators_cold": generators, "cells_a_static_frame_fills": frame_cells,
           "checks": checks, "call_ms": {k: stats(v) for k, v in times.items()}, "kernels_one_rep_ms": kernels}
    doc["frame_static_shadow_cost_cold_ms"] = stats([a - b for a, b in zip(times["frame_static_cold"], times["frame_plain"])])
    doc["frame_static_shadow_cost_warm_ms"] = stats([a - b for a, b in zip(times["frame_static_warm"], times["frame_plain"])])
    doc["points_per_s"] = {k: round(n / (doc["call_ms"][k]["median"] * 1e-3)) for k in VARIANTS if k.startswith("call_")}
    return doc


if args.step:
    print("RESULT " + json.dumps(measure()))
    sys.exit(0)

cmd = [sys.executable, os.path.abspath(__file__), "--step", "measure", "--triangles", str(args.triangles), "--res", str(args.res), "--samples", str(args.samples),
       "--reps", str(args.reps)]
t0 = time.perf_counter()
r = subprocess.run(cmd, capture_output=True, text=True, timeout=420.0)              # TimeoutExpired ends the script: nothing is started after it
if r.returncode != 0:
    sys.stderr.write(r.stdout + r.stderr)
    raise SystemExit("the measurement failed with exit status %d" % r.returncode)
doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
doc["wall_s"] = round(time.perf_counter() - t0, 1)
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
