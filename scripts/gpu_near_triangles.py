"""The triangles within reach of a point, nearest first, with a count (sr_near_triangles_device) measured on the GPU, on the unit-cube scene of
the benchmark (1 M triangles, SR_MODE_BVH, device arrays, warm).

    python scripts/gpu_near_triangles.py [--out profiles/near_triangles/near_triangles.json] [--res 2048] [--reps 10]

One child process with a time limit of its own.  Point sets (gpu_closest_points.py's first three), built on the device and not timed:
  a_surface_scan      the res^2 frame's hit points (sr_render_hits_device) pushed 1 % of the box extent along their normals, scan order
  b_surface_random    the same points, randomly permuted
  c_uniform           4 M seeded uniform points in the box
Per set, after a warm-up of every side, `reps` runs in which the sides alternate, every run timed with an event pair on its stream:
  closest             sr_closest_points_device, all four outputs: the yardstick of k1
  k1                  K = 1, count NULL, all four row outputs (what the list costs: k1 / closest)
  k8, k64             K = 8 / 64 without a limit, count NULL, all four row outputs
  r16_count, r16      K = 16 under a radius chosen on the device results so that the mean count is about 8, with and without count
  r_count             the counting call (K = 0) under that radius
  k8_coherent, k8_input_order   (b_ only) K = 8 with SR_POINTS_COHERENT and under hook 54: the sort against the promise
Before any time is taken k1's rows are compared with closest's outputs, every schedule's rows (SR_POINTS_COHERENT, hook 54) with the sorted
call's, and the per-record loop's (hook 55) over the first 4096 points with the walk's, bit for bit; r16's rows with r16_count's.  Per
variant also triangles / nodes / leaves per point.  Nothing passes or fails on a time.  Reads neither the reference nor the oracle."""
import argparse
import json
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=2048)
ap.add_argument("--triangles", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--uniform", type=int, default=4_000_000)
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["measure"], help="(internal) run the measurement in this process")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    import numpy as np
    t = np.array(xs, dtype=np.float64)
    return {"median": round(float(np.median(t)), 3), "min": round(float(t.min()), 3), "max": round(float(t.max()), 3), "n": int(t.size)}


def frame(res):
    import numpy as np
    import softray_amd as sa
    f = sa.Frame()
    f.width = f.height = res
    f.start_row, f.end_row = 0, res - 1
    f.sub_pixel_res = 1
    f.background_argb = 0xff00ff
    f.flags = sa._lib.F_PRIMARY_STATS_ONLY | sa._lib.F_NO_SPLIT
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
    return f


def measure():
    import torch
    import softray_amd as sa
    L = sa._lib
    dev = torch.device("cuda", 0)
    g = sa.GpuScene(0)
    v9, argb, bmin, bmax = sa.unit_cube_scene(args.triangles)
    g.set_triangles(v9, argb, bmin, bmax)
    g.build((sa.MODE_BVH,))
    extent = float((bmax - bmin).max())
    res = args.res
    f = frame(res)
    n_px = res * res
    stream = torch.cuda.current_stream().cuda_stream
    d_hit = torch.zeros(n_px, dtype=torch.uint8, device=dev)
    d_pos = torch.zeros((n_px, 3), dtype=torch.float64, device=dev)
    d_nrm = torch.zeros((n_px, 3), dtype=torch.float64, device=dev)
    g.render_hits_device(f, d_hit=d_hit.data_ptr(), d_pos=d_pos.data_ptr(), d_normal=d_nrm.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    keep = d_hit != 0
    lifted = (d_pos[keep] + d_nrm[keep] * (0.01 * extent)).contiguous()
    del d_hit, d_pos, d_nrm, keep
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345)
    perm = torch.randperm(lifted.shape[0], device=dev, generator=gen)
    lo = torch.tensor(bmin, dtype=torch.float64, device=dev)
    span = torch.tensor(bmax - bmin, dtype=torch.float64, device=dev)
    uniform = (lo + torch.rand((args.uniform, 3), dtype=torch.float64, device=dev, generator=gen) * span).contiguous()
    sets = {"a_surface_scan": lifted, "b_surface_random": lifted[perm].contiguous(), "c_uniform": uniform}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    doc = {"res": res, "triangles": args.triangles, "reps": args.reps, "extent": extent, "sets": {}}
    KMAX = 64
    for name, pts in sets.items():
        m = pts.shape[0]
        cnt = torch.zeros(m, dtype=torch.int32, device=dev)
        idx = torch.zeros((m, KMAX), dtype=torch.int32, device=dev)
        dist = torch.zeros((m, KMAX), dtype=torch.float64, device=dev)
        pos = torch.zeros((m, KMAX, 3), dtype=torch.float64, device=dev)
        uv = torch.zeros((m, KMAX, 2), dtype=torch.float64, device=dev)
        c_tri = torch.zeros(m, dtype=torch.int32, device=dev)
        c_dist = torch.zeros(m, dtype=torch.float64, device=dev)
        c_pos = torch.zeros((m, 3), dtype=torch.float64, device=dev)
        c_uv = torch.zeros((m, 2), dtype=torch.float64, device=dev)
        lim = torch.zeros(m, dtype=torch.float64, device=dev)

        def near(k, count=False, limit=False, coherent=False, hook=-1, items=m, st=None):
            def run():
                if hook >= 0:
                    g.debug_set(L.DBG_KERNEL_SWITCH, hook)
                try:
                    g.near_triangles_device(sa.MODE_BVH, items, pts.data_ptr(), lim.data_ptr() if limit else 0, k, cnt.data_ptr() if count else 0,
                                            idx.data_ptr() if k else 0, dist.data_ptr() if k else 0, pos.data_ptr() if k else 0, uv.data_ptr() if k else 0,
                                            coherent=coherent, stream=stream, d_stats_ptr=None if st is None else st.data_ptr())
                finally:
                    if hook >= 0:
                        g.debug_set(L.DBG_KERNEL_SWITCH, -1)
            return run

        def closest():
            g.closest_points_device(sa.MODE_BVH, m, pts.data_ptr(), 0, c_tri.data_ptr(), c_dist.data_ptr(), c_pos.data_ptr(), c_uv.data_ptr(), stream=stream)

        def rows(k, items=m):
            """the first `items` rows of a call with K = k (the arrays are [items][k] at the front of the buffers)"""
            torch.cuda.synchronize()
            take = lambda a, w: a.reshape(-1)[:items * k * w].clone()                        # noqa: E731
            return take(idx, 1), take(dist, 1).view(torch.int64), take(pos, 3).view(torch.int64), take(uv, 2).view(torch.int64)

        def equal(a, b):
            return bool(all(torch.equal(x, y) for x, y in zip(a, b)))

        entry = {"points": int(m)}
        same = {}
        # ---- K = 1 against sr_closest_points ----
        closest()
        near(1)()
        r1 = rows(1)
        same["k1_is_closest"] = bool(torch.equal(r1[0], c_tri) and torch.equal(r1[1], c_dist.view(torch.int64)) and
                                     torch.equal(r1[2], c_pos.reshape(-1).view(torch.int64)) and torch.equal(r1[3], c_uv.reshape(-1).view(torch.int64)))
        # ---- the radius: the mean count is about 8 where the radius is the distance of the 8th neighbour of a typical point ----
        near(8)()
        r8 = rows(8)
        d8 = r8[1].view(torch.float64).reshape(m, 8)[:, 7]
        radius = float(d8.median().item())
        lim.fill_(radius)
        entry["radius"] = radius
        # ---- schedules and the loop against the sorted call ----
        for label, fn in (("k8_coherent", near(8, coherent=True)), ("k8_input_order", near(8, hook=54))):
            idx.fill_(90)
            fn()
            same[label] = equal(rows(8), r8)
        loop_n = min(4096, m)
        idx.fill_(90)
        loop_ms = timed(near(8, hook=55, items=loop_n))
        same["k8_loop_4096"] = equal(rows(8, loop_n), tuple(x.reshape(m, -1)[:loop_n].reshape(-1) for x in r8))
        near(16, count=True, limit=True)()
        r16 = rows(16)
        torch.cuda.synchronize()
        entry["count_mean"] = float(cnt.to(torch.float64).mean().item())
        entry["count_max"] = int(cnt.max().item())
        counted = cnt.clone()
        idx.fill_(90)
        near(16, limit=True)()
        same["r16_rows"] = equal(rows(16), r16)
        near(0, count=True, limit=True)()
        torch.cuda.synchronize()
        same["r_count"] = bool(torch.equal(cnt, counted))
        entry["equal"] = same
        if not all(same.values()):
            doc["sets"][name] = entry
            doc["error"] = "outputs differ on " + name
            return doc                                                           # no time is quoted for outputs that differ
        variants = {"closest": closest, "k1": near(1), "k8": near(8), "k64": near(64), "r16_count": near(16, count=True, limit=True),
                    "r16": near(16, limit=True), "r_count": near(0, count=True, limit=True)}
        if name == "b_surface_random":
            variants["k8_coherent"] = near(8, coherent=True)
            variants["k8_input_order"] = near(8, hook=54)
        for fn in variants.values():                                             # warm-up of every side
            timed(fn)
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for v, fn in variants.items():
                times[v].append(timed(fn))
        entry["call_ms"] = {k: stats(v) for k, v in times.items()}
        entry["loop_4096_ms_once"] = round(loop_ms, 3)
        entry["k1_over_closest"] = round(entry["call_ms"]["k1"]["median"] / entry["call_ms"]["closest"]["median"], 3)
        entry["mpoints_per_s"] = {k: round(m / v["median"] / 1e3, 1) for k, v in entry["call_ms"].items()}
        per_point = {}
        for label, kw in (("k1", dict(k=1)), ("k8", dict(k=8)), ("k64", dict(k=64)), ("r16_count", dict(k=16, count=True, limit=True)),
                          ("r16", dict(k=16, limit=True)), ("r_count", dict(k=0, count=True, limit=True))):
            st = torch.zeros(24, dtype=torch.int64, device=dev)
            near(st=st, **kw)()
            torch.cuda.synchronize()
            s = st.cpu().tolist()
            per_point[label] = {"triangles_tested": round(s[1] / m, 2), "nodes": round(s[2] / m, 2), "leaves": round(s[3] / m, 2)}
        st = torch.zeros(24, dtype=torch.int64, device=dev)
        g.closest_points_device(sa.MODE_BVH, m, pts.data_ptr(), 0, c_tri.data_ptr(), c_dist.data_ptr(), c_pos.data_ptr(), c_uv.data_ptr(), stream=stream,
                                d_stats_ptr=st.data_ptr())
        torch.cuda.synchronize()
        s = st.cpu().tolist()
        per_point["closest"] = {"triangles_tested": round(s[1] / m, 2), "nodes": round(s[2] / m, 2), "leaves": round(s[3] / m, 2)}
        entry["per_point"] = per_point
        g.debug_set(L.DBG_KERNEL_TIMING, 1)
        kernels = {}
        for label in ("closest", "k1", "k8"):
            g.reset_kernel_times()
            timed(variants[label])
            kernels[label] = {k: round(t[0], 3) for k, t in g.kernel_times().items()}
        entry["kernels_one_rep_ms"] = kernels
        g.debug_set(L.DBG_KERNEL_TIMING, -1)
        doc["sets"][name] = entry
        del cnt, idx, dist, pos, uv, c_tri, c_dist, c_pos, c_uv, lim, r1, r8, r16
    return doc


if args.step:
    print("RESULT " + json.dumps(measure()))
    sys.exit(0)

cmd = [sys.executable, os.path.abspath(__file__), "--step", "measure", "--triangles", str(args.triangles), "--res", str(args.res), "--reps", str(args.reps),
       "--uniform", str(args.uniform)]
t0 = time.perf_counter()
r = subprocess.run(cmd, capture_output=True, text=True, timeout=540.0)              # TimeoutExpired ends the script: nothing is started after it
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
if "error" in doc:
    raise SystemExit(doc["error"])
