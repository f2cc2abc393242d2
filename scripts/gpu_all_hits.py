"""All hits along a ray (sr_all_hits_rays_device) measured on the GPU, on the unit-cube scene of the benchmark (1 M triangles, SR_MODE_BVH,
device arrays, warm).

    python scripts/gpu_all_hits.py [--out profiles/all_hits/all_hits.json] [--res 2048] [--reps 10]

One child process with a time limit of its own.  The rays are those of scripts/gpu_nearest_rays.py, built from the res^2 frame
(sr_render_hits_device) and not timed:
  c_point_to_point  segments between hit point i and hit point perm[i], both offset along their normals (end points), limit 1.0
  d_probes          seeded hemisphere probes from pos + n * 0.001, AmbientOcclusion.cs' draw
  e_mirror_scan     the mirror rays of the frame, r = dir - n (2 dir.n) from pos + n * 0.001, scan order
  e_mirror_random   the same, randomly permuted
  f_camera          the frame's own camera rays, all of them, scan order
Per workload: the histogram of `count`; then, after a warm-up of every side, `reps` runs in which the sides alternate, every run timed with an
event pair on its stream:
  nearest           sr_nearest_rays_device asked for hit, ray_frac and tri_index: the floor for K = 1 (what a caller can do today)
  peel4             what a caller does today for four hits: four sr_nearest_rays_device calls, the start moved past the hit in torch between them
                    (start += D * (ray_frac + 1e-9)); the rays whose four indices differ from this call's row are counted, not excused
  K{1,4,16,64}      the call with count, index and ray_frac
  K{..}_nocount     the call with count == NULL (the walk culls at the K-th hit)
  K4_input_order    hook 50 (no sort); hook 51, the per-record loop for every ray, is O(triangles) per ray and is not timed here
Before any time is taken the rows of every side are compared with the K = 64 call's.  Reads neither the reference nor the oracle."""
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
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["measure"], help="(internal) run the measurement in this process")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = (1, 4, 16, 64)


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
    g.set_triangles(*sa.unit_cube_scene(args.triangles))
    g.build((sa.MODE_BVH,))
    res = args.res
    f = frame(res)
    n_px = res * res
    stream = torch.cuda.current_stream().cuda_stream
    d_hit = torch.zeros(n_px, dtype=torch.uint8, device=dev)
    cam_s = torch.zeros((n_px, 3), dtype=torch.float64, device=dev)
    cam_d = torch.zeros((n_px, 3), dtype=torch.float64, device=dev)
    d_pos = torch.zeros((n_px, 3), dtype=torch.float64, device=dev)
    d_nrm = torch.zeros((n_px, 3), dtype=torch.float64, device=dev)
    g.render_hits_device(f, d_starts=cam_s.data_ptr(), d_dirs=cam_d.data_ptr(), d_hit=d_hit.data_ptr(), d_pos=d_pos.data_ptr(), d_normal=d_nrm.data_ptr(),
                         stream=stream)
    torch.cuda.synchronize()
    keep = d_hit != 0
    pos, nrm, cdir = d_pos[keep].contiguous(), d_nrm[keep].contiguous(), cam_d[keep].contiguous()
    del d_hit, d_pos, d_nrm, keep
    n = pos.shape[0]
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345)
    lifted = (pos + nrm * 0.001).contiguous()
    perm2 = torch.randperm(n, device=dev, generator=gen)
    perm3 = torch.randperm(n, device=dev, generator=gen)
    probe = torch.rand((n, 3), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
    probe = torch.where(((probe * nrm).sum(dim=1) < 0.0)[:, None], -probe, probe).contiguous()
    mirror = (cdir - nrm * (2.0 * (cdir * nrm).sum(dim=1))[:, None]).contiguous()
    del pos, cdir, nrm
    # name: (starts, dirs or end points, end points?, limit)
    sets = {"c_point_to_point": (lifted, lifted[perm2].contiguous(), True, 1.0),
            "d_probes": (lifted, probe, False, None),
            "e_mirror_scan": (lifted, mirror, False, None),
            "e_mirror_random": (lifted[perm3].contiguous(), mirror[perm3].contiguous(), False, None),
            "f_camera": (cam_s, cam_d, False, None)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    doc = {"res": res, "triangles": args.triangles, "reps": args.reps, "hit_points": int(n), "sets": {}}
    for name, (starts, dirs, endpoints, limit) in sets.items():
        m = starts.shape[0]
        lim = torch.full((m,), limit, dtype=torch.float64, device=dev) if limit is not None else None
        lim_ptr = lim.data_ptr() if lim is not None else 0
        D = (dirs - starts).contiguous() if endpoints else dirs
        cnt = torch.zeros(m, dtype=torch.int32, device=dev)
        idx = {K: torch.zeros((m, K), dtype=torch.int32, device=dev) for K in KS}
        rf = {K: torch.zeros((m, K), dtype=torch.float64, device=dev) for K in KS}
        n_hit = torch.zeros(m, dtype=torch.uint8, device=dev)
        n_rf = torch.zeros(m, dtype=torch.float64, device=dev)
        n_tri = torch.zeros(m, dtype=torch.int32, device=dev)
        peel_idx = torch.zeros((m, 4), dtype=torch.int32, device=dev)

        def all_hits(K, count=True, hook=-1):
            def run():
                if hook >= 0:
                    g.debug_set(L.DBG_KERNEL_SWITCH, hook)
                try:
                    g.all_hits_device(sa.MODE_BVH, m, starts.data_ptr(), dirs.data_ptr(), lim_ptr, K, cnt.data_ptr() if count else 0, idx[K].data_ptr(),
                                      rf[K].data_ptr(), endpoints=endpoints, stream=stream)
                finally:
                    if hook >= 0:
                        g.debug_set(L.DBG_KERNEL_SWITCH, -1)
            return run

        def nearest():
            g.nearest_device(sa.MODE_BVH, m, starts.data_ptr(), dirs.data_ptr(), lim_ptr, d_hit=n_hit.data_ptr(), d_ray_frac=n_rf.data_ptr(),
                             d_tri_index=n_tri.data_ptr(), endpoints=endpoints, stream=stream)

        def peel4():
            s = starts.clone()
            left = lim.clone() if lim is not None else torch.full((m,), float("inf"), dtype=torch.float64, device=dev)
            for k in range(4):
                g.nearest_device(sa.MODE_BVH, m, s.data_ptr(), D.data_ptr(), left.data_ptr(), d_hit=n_hit.data_ptr(), d_ray_frac=n_rf.data_ptr(),
                                 d_tri_index=n_tri.data_ptr(), stream=stream)
                peel_idx[:, k] = n_tri
                step = n_rf + 1e-9
                s = s + D * step[:, None]
                left = torch.where(n_hit != 0, left - step, torch.full_like(left, -1.0))      # a ray that has missed stays missed

        entry = {"rays": int(m), "limit": limit, "end_points": endpoints}
        variants = {"nearest": nearest, "peel4": peel4}
        for K in KS:
            variants["K%d" % K] = all_hits(K)
            variants["K%d_nocount" % K] = all_hits(K, count=False)
        variants["K4_input_order"] = all_hits(4, hook=50)
        for fn in variants.values():                                             # warm-up of every side
            timed(fn)
        # ---- what the sides answer ----
        all_hits(64)()
        torch.cuda.synchronize()
        ref_idx, ref_rf = idx[64].clone(), rf[64].clone()
        c = cnt.to(torch.int64)
        hist = torch.bincount(torch.clamp(c, max=65), minlength=66).cpu().tolist()
        entry["count_histogram"] = {("%d" % k if k < 65 else ">64"): int(v) for k, v in enumerate(hist) if v}
        entry["count_mean"] = round(float(c.double().mean().item()), 3)
        equal = {}
        for K in KS:
            for count in (True, False):
                idx[K].fill_(90)
                rf[K].fill_(90.0)
                all_hits(K, count)()
                torch.cuda.synchronize()
                equal["K%d%s" % (K, "" if count else "_nocount")] = bool(torch.equal(idx[K], ref_idx[:, :K]) and
                                                                         torch.equal(rf[K].view(torch.int64), ref_rf[:, :K].contiguous().view(torch.int64)))
        idx[4].fill_(90)
        all_hits(4, hook=50)()
        torch.cuda.synchronize()
        equal["K4_input_order"] = bool(torch.equal(idx[4], ref_idx[:, :4]))
        nearest()
        torch.cuda.synchronize()
        equal["nearest_ray_frac"] = bool(torch.equal(n_rf.view(torch.int64), ref_rf[:, 0].contiguous().view(torch.int64)) and
                                         torch.equal(n_hit != 0, c > 0))
        entry["equal_to_K64"] = equal
        peel4()
        torch.cuda.synchronize()
        entry["peel4_rays_wrong"] = int((peel_idx != ref_idx[:, :4]).any(dim=1).sum().item())
        if not all(equal.values()):
            doc["sets"][name] = entry
            doc["error"] = "outputs differ on " + name
            return doc                                                           # no time is quoted for outputs that differ
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for v, fn in variants.items():
                times[v].append(timed(fn))
        entry["call_ms"] = {k: stats(v) for k, v in times.items()}
        med = {k: entry["call_ms"][k]["median"] for k in variants}
        entry["ratios"] = {"K1_over_nearest": round(med["K1"] / med["nearest"], 3), "K1_nocount_over_nearest": round(med["K1_nocount"] / med["nearest"], 3),
                           "peel4_over_K4": round(med["peel4"] / med["K4"], 3), "peel4_over_K4_nocount": round(med["peel4"] / med["K4_nocount"], 3),
                           "K4_input_order_over_K4": round(med["K4_input_order"] / med["K4"], 3)}
        g.debug_set(L.DBG_KERNEL_TIMING, 1)
        g.reset_kernel_times()
        timed(variants["K4"])
        entry["kernels_one_rep_ms_K4"] = {k: round(t[0], 3) for k, t in g.kernel_times().items()}
        g.debug_set(L.DBG_KERNEL_TIMING, -1)
        doc["sets"][name] = entry
        del lim, D, cnt, idx, rf, ref_idx, ref_rf, peel_idx
    return doc


if args.step:
    print("RESULT " + json.dumps(measure()))
    sys.exit(0)

cmd = [sys.executable, os.path.abspath(__file__), "--step", "measure", "--triangles", str(args.triangles), "--res", str(args.res), "--reps", str(args.reps)]
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
