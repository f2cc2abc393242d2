"""sr_shadow_points_device measured on the GPU, on the unit-cube scene of the benchmark (SR_MODE_BVH, the benchmark's pose and light, 100
area-light samples): the points are the hit points of the res x res frame, taken with sr_render_hits_device.

    python scripts/gpu_shadow_points.py [--out profiles/shadow_points/points.json]

One child process with a time limit of its own.  After a warm-up of every variant, `reps` repetitions in which the variants alternate, so
that drift of the shared machine hits them alike; every call is timed with a HIP event pair on its stream:
  a  the points in scan order with SR_POINTS_COHERENT          b  in scan order, with the sort
  c  randomly permuted, with the sort                          d  permuted, SR_DBG_KERNEL_SWITCH 37 (no sort)
  e  permuted, with the sort, SR_DBG_KERNEL_SWITCH 38 (the first shaft round with private per-lane walks)
and, beside them in the same repetitions, the shadowed frame and the unshadowed frame of the same pose (sr_render_device): their difference
is the frame's own shadow stage over the same points, the yardstick for (a).  A last repetition runs with SR_DBG_KERNEL_TIMING for the event
times of the ingest kernel and of the ordering step.  Every variant's output is compared with (a)'s.  Reads neither the reference nor
anything the oracle built.
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

VARIANTS = {"a_scan_coherent": (False, True, None), "b_scan_sorted": (False, False, None), "c_permuted_sorted": (True, False, None),
            "d_permuted_no_sort": (True, False, 37), "e_permuted_sorted_per_lane_walks": (True, False, 38)}       # (permuted, coherent, switch)


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
    perm = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    permuted = tuple(x[perm].contiguous() for x in scan)
    out = torch.zeros(n, dtype=torch.int32, device=dev)
    surface = torch.zeros(res * res, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(name):
        permute, coherent, switch = VARIANTS[name]
        p, m, c = permuted if permute else scan
        if switch:
            g.debug_set(sa._lib.DBG_KERNEL_SWITCH, switch)
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.shadow_points_device(fs, n, p.data_ptr(), m.data_ptr(), c.data_ptr(), out.data_ptr(), coherent=coherent, stream=stream)
            e1.record()
            torch.cuda.synchronize()
        finally:
            if switch:
                g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
        return e0.elapsed_time(e1)

    def render(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.render_device(f, surface.data_ptr(), stream)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # warm-up of every variant, and the outputs: all equal to (a)'s
    same = {}
    call("a_scan_coherent")
    ref = out.clone()
    for name, (permute, _, _) in VARIANTS.items():
        call(name)
        same[name] = bool(torch.equal(out, ref[perm] if permute else ref))
    render(fs); render(fp)
    times = {k: [] for k in list(VARIANTS) + ["frame_shadowed", "frame_unshadowed"]}
    for _ in range(args.reps):
        for name in VARIANTS:
            times[name].append(call(name))
        times["frame_shadowed"].append(render(fs))
        times["frame_unshadowed"].append(render(fp))
    g.debug_set(sa._lib.DBG_KERNEL_TIMING, 1)
    kernels = {}
    for name in VARIANTS:
        g.reset_kernel_times()
        call(name)
        kernels[name] = {k: round(v[0], 3) for k, v in g.kernel_times().items()}
    g.debug_set(sa._lib.DBG_KERNEL_TIMING, -1)
    doc = {"res": res, "triangles": args.triangles, "samples": args.samples, "points": n, "outputs_equal_a": same,
           "call_ms": {k: stats(v) for k, v in times.items()}, "kernels_one_rep_ms": kernels}
    diff = [s - p for s, p in zip(times["frame_shadowed"], times["frame_unshadowed"])]
    doc["frame_shadow_stage_ms"] = stats(diff)
    doc["points_per_s"] = {k: round(n / (doc["call_ms"][k]["median"] * 1e-3)) for k in VARIANTS}
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
