"""sr_path_points_device measured on the GPU, on the unit-cube scene of the benchmark (SR_MODE_BVH, the benchmark's pose), by the method of
scripts/gpu_ao_points.py:

    python scripts/gpu_path_points.py [--out profiles/path_points/points.json]

The points are the hit points of the --res^2 (4096^2) frame in scan order (sr_render_hits_device, compacted in torch).  One child process
with a time limit of its own; if it fails or runs out of time the script ends there (nothing more is started on the GPU after it):
  call      the call with `out` only, with all three outputs, and with `dirs` only (nothing traced); the table kernels' (k_pp_window +
            k_aop_states + k_draws: "k_draws") and the second rays' (ingest, ray sort, k_bounce_prep, k_bounce_walk, k_pp_finish_walked:
            "path_points_rays") own times from the library's HIP event pairs; the same call with the table made on the host
            (SR_DBG_KERNEL_SWITCH 45) once, for the comparison of the outputs and for scale
  frames    the plain frame and the path-traced frame of the same size in the same session: their difference is what the frame pays
            for the same second rays -- the yardstick
  jump      host time of the jump-ahead per pass: sr_net_random_jump over 3 x 2^22 and over 3 x 2^40 draws
--step profile runs the all-outputs call three times and nothing else: the program a kernel-trace profiler is put in front of.
A call never waits for the host, so it is timed with the host clock from the call to the end of a device synchronise; the frames alike.
Reads neither the reference nor anything the oracle built.
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["call", "profile"], help="(internal) run one step in this process")
args = ap.parse_args()
MAX_PASS = 1 << 22


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


def frame(res, path=False):
    import numpy as np
    import softray_amd as sa
    f = sa.Frame()
    f.width = f.height = res
    f.start_row, f.end_row = 0, res - 1
    f.sub_pixel_res = 1
    f.background_argb = 0xff00ff
    f.flags = sa.F_SHADING | sa.F_POINT_LIGHT | sa.F_SPECULAR | (sa.F_PATH_TRACING if path else 0)
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


class Points:
    """The hit points of a frame on the device, in scan order, shaded, with the call's outputs."""

    def __init__(self, g, f):
        import softray_amd as sa
        import torch
        n = sa.GpuScene.sample_count(f)
        hit = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        pos = torch.empty((n, 3), dtype=torch.float64, device="cuda:0")
        nrm = torch.empty((n, 3), dtype=torch.float64, device="cuda:0")
        col = torch.empty(n, dtype=torch.int32, device="cuda:0")
        g.render_hits_device(f, d_hit=hit.data_ptr(), d_pos=pos.data_ptr(), d_normal=nrm.data_ptr(), d_color=col.data_ptr())
        idx = torch.nonzero(hit, as_tuple=False).reshape(-1)
        self.n = int(idx.numel())
        self.pos, self.nrm, self.col = pos[idx].contiguous(), nrm[idx].contiguous(), col[idx].contiguous()
        g.shade_points_device(f, self.n, self.pos.data_ptr(), self.nrm.data_ptr(), self.col.data_ptr(), self.col.data_ptr())
        self.out = torch.zeros(self.n, dtype=torch.int32, device="cuda:0")
        self.incoming = torch.zeros(self.n, dtype=torch.int32, device="cuda:0")
        self.dirs = torch.zeros((self.n, 3), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()

    def call(self, g, f, stream, out=True, incoming=True, dirs=True):
        """One call: (host-clock ms to the end of what it enqueued, the table kernels' ms, the second rays' ms -- every kernel from ingest to finish)."""
        import torch
        g.reset_kernel_times()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.path_points_device(f, self.n, self.pos.data_ptr(), self.nrm.data_ptr(), self.col.data_ptr(), self.out.data_ptr() if out else 0,
                             self.incoming.data_ptr() if incoming else 0, self.dirs.data_ptr() if dirs else 0, stream=stream)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        kt = g.kernel_times()
        return ms, kt.get("k_draws", (0.0, 0))[0], kt.get("path_points_rays", (0.0, 0))[0]


def timed_frame(g, f, surface, stream):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.render_device(f, surface.data_ptr(), stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def step_profile():
    import torch
    g = make_scene()
    stream = torch.cuda.current_stream().cuda_stream
    f = frame(args.res)
    pts = Points(g, f)
    for _ in range(3):
        pts.call(g, f, stream)
    return {"points": pts.n}


def step_call():
    import numpy as np
    import softray_amd as sa
    import torch
    g = make_scene()
    res = args.res
    stream = torch.cuda.current_stream().cuda_stream
    f = frame(res)
    pts = Points(g, f)
    pts.call(g, f, stream)                                             # warm-up of every kernel, the scratch and the table
    dev = [pts.out.clone(), pts.incoming.clone(), pts.dirs.clone()]
    g.debug_set(sa._lib.DBG_KERNEL_SWITCH, 45)
    host_ms = pts.call(g, f, stream)[0]
    equal = bool(torch.equal(dev[0], pts.out) and torch.equal(dev[1], pts.incoming) and torch.equal(dev[2], pts.dirs))
    g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
    if not equal:
        raise SystemExit("the device table and the host table give different outputs")
    kinds = {"out_only": dict(incoming=False, dirs=False), "all_outputs": dict(), "dirs_only": dict(out=False, incoming=False)}
    ms = {k: [] for k in kinds}
    draws = {k: [] for k in kinds}
    trace = {k: [] for k in kinds}
    for k, kw in kinds.items():
        pts.call(g, f, stream, **kw)
    surface = torch.zeros(res * res, dtype=torch.int32, device="cuda:0")
    fp = frame(res, path=True)
    for _ in range(2):
        timed_frame(g, f, surface, stream)
        timed_frame(g, fp, surface, stream)
    plain, path = [], []
    for _ in range(args.reps):                                         # alternating: drift hits all alike
        for k, kw in kinds.items():
            a, b, c = pts.call(g, f, stream, **kw)
            ms[k].append(a); draws[k].append(b); trace[k].append(c)
        plain.append(timed_frame(g, f, surface, stream))
        path.append(timed_frame(g, fp, surface, stream))
    hit_fraction = float((pts.incoming != 0).sum().item()) / pts.n
    jump = {}
    for name, skip in (("skip_3x2^22", 3 << 22), ("skip_3x2^40", 3 << 40)):
        t = []
        for _ in range(20):
            t0 = time.perf_counter()
            sa.net_random_jump(1234567890, skip)
            t.append((time.perf_counter() - t0) * 1e3)
        jump[name + "_ms"] = stats(t)
    yard = float(np.median(path)) - float(np.median(plain))
    doc = {"res": res, "triangles": args.triangles, "points": pts.n, "passes": (pts.n + MAX_PASS - 1) // MAX_PASS, "second_rays_with_nonblack_hit": round(hit_fraction, 4),
           "outputs_equal_host_table": equal, "call_host_table_once_ms": round(host_ms, 3),
           "plain_frame_ms": stats(plain), "path_traced_frame_ms": stats(path), "yardstick_path_minus_plain_ms": round(yard, 3), "host_jump": jump}
    for k in kinds:
        doc["call_%s_ms" % k] = stats(ms[k])
        doc["call_%s_table_kernels_ms" % k] = stats(draws[k])
        doc["call_%s_second_rays_all_kernels_ms" % k] = stats(trace[k])
    doc["call_all_outputs_over_yardstick"] = round(float(np.median(ms["all_outputs"])) / yard, 3) if yard > 0 else None
    doc["call_out_only_over_yardstick"] = round(float(np.median(ms["out_only"])) / yard, 3) if yard > 0 else None
    return doc


if args.step:
    print("RESULT " + json.dumps({"call": step_call, "profile": step_profile}[args.step]()))
    sys.exit(0)


def child(step, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--triangles", str(args.triangles), "--res", str(args.res), "--reps", str(args.reps)]
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


doc = {"call": child("call", 420.0)}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
