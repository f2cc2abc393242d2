"""The closest point of the mesh for a batch of points (sr_closest_points_device) measured on the GPU, on the unit-cube scene of the benchmark
(1 M triangles, SR_MODE_BVH, device arrays, all four outputs, warm).

    python scripts/gpu_closest_points.py [--out profiles/closest_points/closest_points.json] [--res 2048] [--reps 10]

One child process with a time limit of its own.  Point sets, built on the device and not timed:
  a_surface_scan      the res^2 frame's hit points (sr_render_hits_device) pushed 1 % of the box extent along their normals, scan order
  b_surface_random    the same points, randomly permuted
  c_uniform           4 M seeded uniform points in the box
  d_lattice           a 256^3 lattice over the box (a distance field), x fastest
Per set, after a warm-up of every side, `reps` runs in which the sides alternate, every run timed with an event pair on its stream:
  sorted              the call as it is (Morton order per pass)
  coherent            SR_POINTS_COHERENT (the caller's promise: input order is kept)
  input_order         hook 52 (no sort whatever the options say; the same kernels as `coherent`, kept as the cross-check of the option)
  sorted_limit        the first three sets with max_dist = 2 % of the extent
  nearest_rays        for scale only (a_, b_): sr_nearest_rays_device over rays from the same points along -normal, hit / ray_frac / tri_index
and once: loop_4096 -- the per-record loop (hook 53) over the first 4096 points, for scale only (it is O(triangles) per point).
Before any time is taken the outputs of `coherent` and `input_order` are compared with `sorted`'s (bit for bit), and loop_4096's with the
first 4096 answers.  Nothing is measured against nearest_rays or the loop, and nothing passes or fails on a time.  Reads neither the reference
nor the oracle."""
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
ap.add_argument("--lattice", type=int, default=256)
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
    pos, nrm = d_pos[keep].contiguous(), d_nrm[keep].contiguous()
    del d_hit, d_pos, d_nrm, keep
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345)
    lifted = (pos + nrm * (0.01 * extent)).contiguous()
    down = (-nrm).contiguous()
    perm = torch.randperm(lifted.shape[0], device=dev, generator=gen)
    lo = torch.tensor(bmin, dtype=torch.float64, device=dev)
    span = torch.tensor(bmax - bmin, dtype=torch.float64, device=dev)
    uniform = (lo + torch.rand((args.uniform, 3), dtype=torch.float64, device=dev, generator=gen) * span).contiguous()
    k = (torch.arange(args.lattice, dtype=torch.float64, device=dev) + 0.5) / args.lattice
    zz, yy, xx = torch.meshgrid(k, k, k, indexing="ij")
    lattice = (lo + torch.stack([xx, yy, zz], dim=-1).reshape(-1, 3) * span).contiguous()
    del pos, nrm, k, xx, yy, zz
    # name: (points, -normals for the scale figure or None, measured with a limit too?)
    sets = {"a_surface_scan": (lifted, down, True),
            "b_surface_random": (lifted[perm].contiguous(), down[perm].contiguous(), True),
            "c_uniform": (uniform, None, True),
            "d_lattice": (lattice, None, False)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    doc = {"res": res, "triangles": args.triangles, "reps": args.reps, "extent": extent, "sets": {}}
    for name, (pts, dirs, with_limit) in sets.items():
        m = pts.shape[0]
        lim = torch.full((m,), 0.02 * extent, dtype=torch.float64, device=dev)
        tri = torch.zeros(m, dtype=torch.int32, device=dev)
        dist = torch.zeros(m, dtype=torch.float64, device=dev)
        cpos = torch.zeros((m, 3), dtype=torch.float64, device=dev)
        uv = torch.zeros((m, 2), dtype=torch.float64, device=dev)
        n_hit = torch.zeros(m, dtype=torch.uint8, device=dev)
        n_rf = torch.zeros(m, dtype=torch.float64, device=dev)
        n_tri = torch.zeros(m, dtype=torch.int32, device=dev)

        def closest(coherent=False, hook=-1, limit=False, count=m):
            def run():
                if hook >= 0:
                    g.debug_set(L.DBG_KERNEL_SWITCH, hook)
                try:
                    g.closest_points_device(sa.MODE_BVH, count, pts.data_ptr(), lim.data_ptr() if limit else 0, tri.data_ptr(), dist.data_ptr(), cpos.data_ptr(),
                                            uv.data_ptr(), coherent=coherent, stream=stream)
                finally:
                    if hook >= 0:
                        g.debug_set(L.DBG_KERNEL_SWITCH, -1)
            return run

        def nearest():
            g.nearest_device(sa.MODE_BVH, m, pts.data_ptr(), dirs.data_ptr(), 0, d_hit=n_hit.data_ptr(), d_ray_frac=n_rf.data_ptr(), d_tri_index=n_tri.data_ptr(),
                             stream=stream)

        def snapshot():
            torch.cuda.synchronize()
            return tri.clone(), dist.clone(), cpos.clone(), uv.clone()

        def equal(a, b, count=m):
            return bool(torch.equal(a[0][:count], b[0][:count]) and all(torch.equal(x[:count].contiguous().view(torch.int64), y[:count].contiguous().view(torch.int64))
                                                                         for x, y in zip(a[1:], b[1:])))

        entry = {"points": int(m)}
        variants = {"sorted": closest(), "coherent": closest(coherent=True), "input_order": closest(hook=52)}
        if with_limit:
            variants["sorted_limit"] = closest(limit=True)
        if dirs is not None:
            variants["nearest_rays"] = nearest
        for fn in variants.values():                                             # warm-up of every side
            timed(fn)
        # ---- what the sides answer ----
        variants["sorted"]()
        ref = snapshot()
        entry["answered"] = int((ref[0] >= 0).sum().item())
        entry["dist_mean"] = float(ref[1].mean().item())
        same = {}
        for v in ("coherent", "input_order"):
            tri.fill_(90)
            variants[v]()
            same[v] = equal(snapshot(), ref)
        tri.fill_(90)
        loop_n = min(4096, m)
        loop_ms = timed(closest(hook=53, count=loop_n))
        same["loop_4096"] = equal(snapshot(), ref, loop_n)
        if with_limit:
            variants["sorted_limit"]()
            cut = snapshot()
            within = ref[1] <= lim
            same["sorted_limit"] = bool(torch.equal(cut[0], torch.where(within, ref[0], torch.full_like(ref[0], -1))) and
                                        torch.equal(cut[1], torch.where(within, ref[1], torch.zeros_like(ref[1]))))
            entry["within_limit"] = int(within.sum().item())
        entry["equal_to_sorted"] = same
        if not all(same.values()):
            doc["sets"][name] = entry
            doc["error"] = "outputs differ on " + name
            return doc                                                           # no time is quoted for outputs that differ
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for v, fn in variants.items():
                times[v].append(timed(fn))
        entry["call_ms"] = {k: stats(v) for k, v in times.items()}
        entry["loop_4096_ms_once"] = round(loop_ms, 3)
        entry["mpoints_per_s_sorted"] = round(m / entry["call_ms"]["sorted"]["median"] / 1e3, 1)
        st = torch.zeros(24, dtype=torch.int64, device=dev)
        g.closest_points_device(sa.MODE_BVH, m, pts.data_ptr(), 0, tri.data_ptr(), dist.data_ptr(), cpos.data_ptr(), uv.data_ptr(), stream=stream,
                                d_stats_ptr=st.data_ptr())
        torch.cuda.synchronize()
        s = st.cpu().tolist()
        entry["per_point"] = {"triangles_tested": round(s[1] / m, 2), "nodes": round(s[2] / m, 2), "leaves": round(s[3] / m, 2)}
        g.debug_set(L.DBG_KERNEL_TIMING, 1)
        g.reset_kernel_times()
        timed(variants["sorted"])
        entry["kernels_one_rep_ms_sorted"] = {k: round(t[0], 3) for k, t in g.kernel_times().items()}
        g.debug_set(L.DBG_KERNEL_TIMING, -1)
        doc["sets"][name] = entry
        del lim, tri, dist, cpos, uv, n_hit, n_rf, n_tri, ref
    return doc


if args.step:
    print("RESULT " + json.dumps(measure()))
    sys.exit(0)

cmd = [sys.executable, os.path.abspath(__file__), "--step", "measure", "--triangles", str(args.triangles), "--res", str(args.res), "--reps", str(args.reps),
       "--uniform", str(args.uniform), "--lattice", str(args.lattice)]
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
