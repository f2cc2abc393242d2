"""Ambient occlusion (SR_F_AMBIENT_OCCLUSION) measured on the GPU, on the unit-cube scene of the benchmark (SR_MODE_BVH, shading on):

    python scripts/gpu_ao.py [--out profiles/ao/frames.json]

Every step is a child process of its own with a time limit of its own, and a step that fails or runs out of time ends the script (nothing
more is started on the GPU after it):
  1. cached      --res^2 (4096^2): the first frame (cold cache, with its generator count, its table size and the probe kernel's own time
                 from the library's HIP event pair) and the second frame (warm: no probes, no table), `reps` times each -- the cache is
                 reset before every cold frame                                                             limit 600 s
  2. uncached    --uncached-res^2 (1024^2): every hit sample generates; frame time, generators, table size   limit 600 s
  3. plain       the same frames without the AO bits, from the same run, for scale                          (inside steps 1 and 2)
  4. shadows     the 100-sample soft-shadow frame as two half-frame pipelines (default) and as one (SR_F_NO_SPLIT), and the shadowed AO
                 frame on a warm cache: what an AO frame pays for running as one pipeline                   (inside step 1)
  5. A/B         the probe kernel with nearest-hit walks (SR_DBG_KERNEL_SWITCH 34) instead of the any-hit walks  (inside steps 1 and 2)
`table_bytes_upper_bound` is 1200 bytes x ALL generators: what one row block would need; the table holds the fullest block's share.
`--step probe` (internal, also what a profiler is pointed at: `rocprofv3 --kernel-trace --stats -- python scripts/gpu_ao.py --step probe`)
renders one warm-up and one cold cached frame and prints the probe kernel's event time, probes per second and the lane occupancy of the
(generator, probe) layout: probes / (64 x the waves that carry at least one).
AO frames wait for the device once (the host sizes the draw table), so every frame -- the plain ones alike -- is timed with the host clock
around sr_render_device into a torch tensor + synchronise.  The default of 8 row blocks keeps the uncached 1024^2 frame's table (1200
bytes per generator of the fullest block) under the 256 MiB limit.  Reads neither the reference nor anything the oracle built.
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
ap.add_argument("--uncached-res", type=int, default=1024)
ap.add_argument("--triangles", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--concurrency", type=int, default=8, help="rayTraceConcurrency: the row blocks (the table holds the fullest block's generators)")
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["cached", "uncached", "probe"], help="(internal) run one step in this process")
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
    return g


def sa_lib():
    import softray_amd as sa
    return sa._lib


def frame(res, ao, uncached=False):
    import numpy as np
    import softray_amd as sa
    f = sa.Frame()
    f.width = f.height = res
    f.start_row, f.end_row = 0, res - 1
    f.sub_pixel_res = 1
    f.background_argb = 0xff00ff
    f.flags = sa.F_SHADING | sa.F_POINT_LIGHT | sa.F_SPECULAR | (sa.F_AMBIENT_OCCLUSION if ao else 0) | (sa.F_AO_UNCACHED if ao and uncached else 0)
    f.trace_mode = sa.MODE_BVH
    f.random_seed = 1234567890
    f.concurrency = args.concurrency
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
    """One device frame, host clock from the call to the end of everything it enqueued; the probe kernel's event time of that frame."""
    import torch
    g.reset_kernel_times()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.render_device(f, surface.data_ptr(), stream)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, g.kernel_times().get("k_ao_probe", (0.0, 0))[0]


def generators_of(g, f):
    """Generators of a frame = secondary rays / 100 (blocking call with statistics; run on a scene state equal to the timed one)."""
    g.render(f)
    return int(g.ray_stats()[4]) // 100


def lane_occupancy(generators):
    probes = generators * 100
    return round(probes / (64.0 * ((probes + 63) // 64)), 6) if probes else 0.0


def step_cached():
    import numpy as np
    import torch
    g = make_scene()
    res = args.res
    surface = torch.zeros(res * res, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    fa, fp = frame(res, True), frame(res, False)
    g.reset_ao_cache()
    gens = generators_of(g, fa)                                       # warm-up of every kernel and of the scratch, and the count
    filled = int(np.count_nonzero(g.get_ao_cache()))
    cold, warm, plain, probe = [], [], [], []
    for _ in range(args.reps):
        g.reset_ao_cache()
        ms, pk = timed(g, fa, surface, stream)
        cold.append(ms); probe.append(pk)
        warm.append(timed(g, fa, surface, stream)[0])
        plain.append(timed(g, fp, surface, stream)[0])
    # what a shadowed AO frame pays for running as ONE pipeline: the shadowed frame without AO as two half-frame pipelines (the default) and
    # with SR_F_NO_SPLIT, and the shadowed AO frame on a warm cache
    import softray_amd as sa
    fs, fsn, fsa = frame(res, False), frame(res, False), frame(res, True)
    fs.flags |= sa.F_SHADOWS
    fsn.flags |= sa.F_SHADOWS | sa._lib.F_NO_SPLIT
    fsa.flags |= sa.F_SHADOWS
    g.reset_ao_cache()
    for f in (fs, fsn, fsa):
        timed(g, f, surface, stream)                                  # warm-up (and the cache for fsa)
    sh_split, sh_one, sh_ao = [], [], []
    for _ in range(args.reps):
        sh_split.append(timed(g, fs, surface, stream)[0])
        sh_one.append(timed(g, fsn, surface, stream)[0])
        sh_ao.append(timed(g, fsa, surface, stream)[0])
    # A/B of the probe walk (same bytes): SR_DBG_KERNEL_SWITCH 34 = nearest-hit walks instead of any-hit walks with the limit 2.0
    nearest = []
    g.debug_set(sa_lib().DBG_KERNEL_SWITCH, 34)
    for _ in range(args.reps):
        g.reset_ao_cache()
        nearest.append(timed(g, fa, surface, stream)[1])
    g.debug_set(sa_lib().DBG_KERNEL_SWITCH, -1)
    return {"res": res, "triangles": args.triangles, "concurrency": args.concurrency, "generators_cold": gens, "cells_filled": filled,
            "k_ao_probe_nearest_hit_ms": stats(nearest),
            "shadowed_frame_two_pipelines_ms": stats(sh_split), "shadowed_frame_no_split_ms": stats(sh_one), "shadowed_ao_warm_frame_ms": stats(sh_ao),
            "table_bytes_upper_bound": gens * 1200, "cold_frame_ms": stats(cold), "warm_frame_ms": stats(warm), "plain_frame_ms": stats(plain),
            "k_ao_probe_ms": stats(probe), "probes_per_s": round(gens * 100 / (float(np.median(probe)) * 1e-3), 0) if gens else 0,
            "lane_occupancy": lane_occupancy(gens)}


def step_uncached():
    import numpy as np
    import torch
    g = make_scene()
    res = args.uncached_res
    surface = torch.zeros(res * res, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    fa, fp = frame(res, True, True), frame(res, False)
    gens = generators_of(g, fa)
    ao, plain, probe = [], [], []
    for _ in range(args.reps):
        ms, pk = timed(g, fa, surface, stream)
        ao.append(ms); probe.append(pk)
        plain.append(timed(g, fp, surface, stream)[0])
    nearest = []
    g.debug_set(sa_lib().DBG_KERNEL_SWITCH, 34)
    for _ in range(args.reps):
        nearest.append(timed(g, fa, surface, stream)[1])
    g.debug_set(sa_lib().DBG_KERNEL_SWITCH, -1)
    return {"res": res, "triangles": args.triangles, "concurrency": args.concurrency, "generators": gens, "table_bytes_upper_bound": gens * 1200,
            "k_ao_probe_nearest_hit_ms": stats(nearest),
            "uncached_frame_ms": stats(ao), "plain_frame_ms": stats(plain), "k_ao_probe_ms": stats(probe),
            "probes_per_s": round(gens * 100 / (float(np.median(probe)) * 1e-3), 0) if gens else 0, "lane_occupancy": lane_occupancy(gens)}


def step_probe():
    import torch
    g = make_scene()
    res = args.res
    surface = torch.zeros(res * res, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    fa = frame(res, True)
    gens = generators_of(g, fa)
    g.reset_ao_cache()
    ms, pk = timed(g, fa, surface, stream)
    return {"res": res, "triangles": args.triangles, "generators": gens, "cold_frame_ms": round(ms, 3), "k_ao_probe_ms": round(pk, 3),
            "probes_per_s": round(gens * 100 / (pk * 1e-3), 0) if pk else 0, "lane_occupancy": lane_occupancy(gens)}


if args.step:
    print("RESULT " + json.dumps({"cached": step_cached, "uncached": step_uncached, "probe": step_probe}[args.step]()))
    sys.exit(0)


def child(step, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--triangles", str(args.triangles), "--res", str(args.res),
           "--uncached-res", str(args.uncached_res), "--reps", str(args.reps), "--concurrency", str(args.concurrency)]
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


doc = {"cached": child("cached", 600.0)}
doc["uncached"] = child("uncached", 600.0)
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
