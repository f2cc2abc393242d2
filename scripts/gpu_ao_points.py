"""sr_ao_points_device measured on the GPU, on the unit-cube scene of the benchmark (SR_MODE_BVH, the benchmark's pose), by the method of
scripts/gpu_ao.py:

    python scripts/gpu_ao_points.py [--out profiles/ao_points/points.json]

Every step is a child process of its own with a time limit of its own, and a step that fails or runs out of time ends the script (nothing
more is started on the GPU after it):
  1. uncached    the hit points of the --uncached-res^2 (1024^2) frame, in scan order: sr_ao_points_device uncached with the table made on
                 the device, the same with the table made on the host (SR_DBG_KERNEL_SWITCH 44), the uncached AO frame at --concurrency
                 row blocks for scale, and the table kernels' (k_aop_base + k_aop_states + k_draws: "k_draws") and the probe kernel's own
                 times from the library's HIP event pairs                                                  limit 600 s
  2. cached      the hit points of the --res^2 (4096^2) frame: the call on a cold cache and on a warm one, the AO frame cold and warm for
                 scale                                                                                     limit 600 s
  3. jump        host time of the jump-ahead: sr_net_random_jump over 300 x 2^17 and over 300 x 2^40 draws   (inside step 1)
The outputs of the device table and of the host table are compared (they must be equal) before anything is timed.
A call never waits for the host, so it is timed with the host clock from the call to the end of a device synchronise; the AO frames
alike.  Reads neither the reference nor anything the oracle built.
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
ap.add_argument("--concurrency", type=int, default=8, help="rayTraceConcurrency of the AO frames the calls are compared with")
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["cached", "uncached"], help="(internal) run one step in this process")
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


class Points:
    """The hit points of a frame on the device, in scan order, with the call's outputs."""

    def __init__(self, g, f):
        import softray_amd as sa
        import torch
        n = sa.GpuScene.sample_count(f)
        hit = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        pos = torch.empty((n, 3), dtype=torch.float64, device="cuda:0")
        nrm = torch.empty((n, 3), dtype=torch.float64, device="cuda:0")
        g.render_hits_device(f, d_hit=hit.data_ptr(), d_pos=pos.data_ptr(), d_normal=nrm.data_ptr())
        idx = torch.nonzero(hit, as_tuple=False).reshape(-1)
        self.n = int(idx.numel())
        self.pos, self.nrm = pos[idx].contiguous(), nrm[idx].contiguous()
        self.amount = torch.zeros(self.n, dtype=torch.uint8, device="cuda:0")
        self.gen = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()

    def call(self, g, f, stream):
        """One call: (host-clock ms to the end of what it enqueued, k_draws ms, k_aop_probe ms)."""
        import torch
        g.reset_kernel_times()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.ao_points_device(f, self.n, self.pos.data_ptr(), self.nrm.data_ptr(), 0, 0, self.amount.data_ptr(), stream=stream, d_generators_ptr=self.gen.data_ptr())
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        kt = g.kernel_times()
        return ms, kt.get("k_draws", (0.0, 0))[0], kt.get("k_aop_probe", (0.0, 0))[0]


def timed_frame(g, f, surface, stream):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.render_device(f, surface.data_ptr(), stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def step_uncached():
    import numpy as np
    import softray_amd as sa
    import torch
    g = make_scene()
    res = args.uncached_res
    stream = torch.cuda.current_stream().cuda_stream
    fu = frame(res, True, True)
    pts = Points(g, fu)
    pts.call(g, fu, stream)                                            # warm-up of every kernel, the scratch and the table
    dev_bytes = pts.amount.clone()
    gens = int(pts.gen.item())
    g.debug_set(sa._lib.DBG_KERNEL_SWITCH, 44)
    pts.call(g, fu, stream)
    equal = bool(torch.equal(dev_bytes, pts.amount))
    g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
    if not equal:
        raise SystemExit("the device table and the host table give different bytes")
    dev, host, draws, probe = [], [], [], []
    for _ in range(args.reps):
        ms, dk, pk = pts.call(g, fu, stream)
        dev.append(ms); draws.append(dk); probe.append(pk)
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, 44)
        host.append(pts.call(g, fu, stream)[0])
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
    surface = torch.zeros(res * res, dtype=torch.int32, device="cuda:0")
    timed_frame(g, fu, surface, stream)
    ao = [timed_frame(g, fu, surface, stream) for _ in range(args.reps)]
    jump = {}
    for name, skip in (("skip_300x2^17", 300 << 17), ("skip_300x2^40", 300 << 40)):
        t = []
        for _ in range(20):
            t0 = time.perf_counter()
            sa.net_random_jump(1234567890, skip)
            t.append((time.perf_counter() - t0) * 1e3)
        jump[name + "_ms"] = stats(t)
    return {"res": res, "triangles": args.triangles, "points": pts.n, "generators": gens, "passes": (pts.n + (1 << 17) - 1) >> 17,
            "table_bytes_per_full_pass": (1 << 17) * 1200, "outputs_equal_host_table": equal,
            "call_device_table_ms": stats(dev), "call_host_table_ms": stats(host), "k_draws_ms": stats(draws), "k_aop_probe_ms": stats(probe),
            "probes_per_s": round(gens * 100 / (float(np.median(probe)) * 1e-3), 0) if gens else 0,
            "draws_per_s": round(gens * 300 / (float(np.median(draws)) * 1e-3), 0) if gens else 0,
            "uncached_ao_frame_ms": stats(ao), "uncached_ao_frame_concurrency": args.concurrency, "host_jump": jump}


def step_cached():
    import numpy as np
    import torch
    g = make_scene()
    res = args.res
    stream = torch.cuda.current_stream().cuda_stream
    fc = frame(res, True)
    pts = Points(g, fc)
    g.reset_ao_cache()
    pts.call(g, fc, stream)                                            # warm-up
    gens = int(pts.gen.item())
    filled = int(np.count_nonzero(g.get_ao_cache()))
    cold, warm, draws, probe = [], [], [], []
    for _ in range(args.reps):
        g.reset_ao_cache()
        ms, dk, pk = pts.call(g, fc, stream)
        cold.append(ms); draws.append(dk); probe.append(pk)
        warm.append(pts.call(g, fc, stream)[0])
        if int(pts.gen.item()) != 0:
            raise SystemExit("a warm call generated")
    surface = torch.zeros(res * res, dtype=torch.int32, device="cuda:0")
    g.reset_ao_cache()
    timed_frame(g, fc, surface, stream)
    f_cold, f_warm = [], []
    for _ in range(args.reps):
        g.reset_ao_cache()
        f_cold.append(timed_frame(g, fc, surface, stream))
        f_warm.append(timed_frame(g, fc, surface, stream))
    return {"res": res, "triangles": args.triangles, "points": pts.n, "generators_cold": gens, "cells_filled": filled, "passes": (pts.n + (1 << 17) - 1) >> 17,
            "call_cold_ms": stats(cold), "call_warm_ms": stats(warm), "k_draws_ms": stats(draws), "k_aop_probe_ms": stats(probe),
            "ao_frame_cold_ms": stats(f_cold), "ao_frame_warm_ms": stats(f_warm), "ao_frame_concurrency": args.concurrency}


if args.step:
    print("RESULT " + json.dumps({"cached": step_cached, "uncached": step_uncached}[args.step]()))
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


doc = {"uncached": child("uncached", 600.0)}
doc["cached"] = child("cached", 600.0)
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
