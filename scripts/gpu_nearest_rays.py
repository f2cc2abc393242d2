"""Nearest-hit ray batches (sr_nearest_rays_device) measured on the GPU, on the unit-cube scene of the benchmark (1 M triangles, SR_MODE_BVH,
device arrays, all six outputs, warm).

    python scripts/gpu_nearest_rays.py [--out profiles/nearest_rays/nearest_rays.json] [--refill 8,48]

One child process with a time limit of its own.  The rays are built from the 4096^2 frame (sr_render_hits_device; about 15 M hit points) and
are not timed:
  a_light_scan      segments from a light point to pos + n * 0.001 of every hit point, scan order (end points)
  b_light_random    the same, randomly permuted
  c_point_to_point  segments between hit point i and hit point perm[i], both offset along their normals (end points); no limit, 1.0 and 2.0
  d_probes          seeded hemisphere probes from pos + n * 0.001, AmbientOcclusion.cs' draw; no limit, 1.0 and 2.0
  e_mirror_scan     the mirror rays of the frame, r = dir - n (2 dir.n) from pos + n * 0.001, scan order
  e_mirror_random   the same, randomly permuted
  f_camera          the frame's own camera rays, all of them, scan order (for the record beside sr_trace_origin_rays)
Per workload, after a warm-up of every side, `reps` runs in which the sides alternate, every run timed with an event pair on its stream:
  baseline          sr_trace_rays_device asked for the same six outputs -- k_trace, which the call's change does not edit -- plus, where a
                    limit is set, the blanking of the answers beyond it in torch (timed with it)
  nearest           the call without options (a pass is sorted)
  input_order       the call under hook 48 (no sort)
  coherent          scan-order workloads only: the call with SR_RAYS_COHERENT
  per_lane          the call under hook 49 (one private walk per lane, input order)
  refill_T          with --refill T[,T...]: the call under hook 100 + T
Before any time is taken the six outputs of every side are compared byte for byte with the baseline's.  Reads neither the reference nor the
oracle."""
import argparse
import json
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=4096)
ap.add_argument("--triangles", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--refill", default="", help="comma-separated T: also time the call under hook 100 + T (the walk's lanes refilled at T busy ones)")
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["measure"], help="(internal) run the measurement in this process")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEYS = ("hit", "ray_frac", "pos", "normal", "color", "tri_index")


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
    light = torch.tensor([0.2, 0.45, -0.3], dtype=torch.float64, device=dev)[None, :].expand(n, 3).contiguous()
    perm = torch.randperm(n, device=dev, generator=gen)
    perm2 = torch.randperm(n, device=dev, generator=gen)
    perm3 = torch.randperm(n, device=dev, generator=gen)
    probe = torch.rand((n, 3), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
    probe = torch.where(((probe * nrm).sum(dim=1) < 0.0)[:, None], -probe, probe).contiguous()
    mirror = (cdir - nrm * (2.0 * (cdir * nrm).sum(dim=1))[:, None]).contiguous()
    del pos, cdir
    # name: (starts, dirs or end points, end points?, limits to run, scan order?)
    sets = {"a_light_scan": (light, lifted, True, (None,), True),
            "b_light_random": (light, lifted[perm].contiguous(), True, (None,), False),
            "c_point_to_point": (lifted, lifted[perm2].contiguous(), True, (None, 1.0, 2.0), False),
            "d_probes": (lifted, probe, False, (None, 1.0, 2.0), False),
            "e_mirror_scan": (lifted, mirror, False, (None,), True),
            "e_mirror_random": (lifted[perm3].contiguous(), mirror[perm3].contiguous(), False, (None,), False),
            "f_camera": (cam_s, cam_d, False, (None,), True)}
    del nrm
    shapes = dict(hit=((n_px,), torch.uint8), ray_frac=((n_px,), torch.float64), pos=((n_px, 3), torch.float64), normal=((n_px, 3), torch.float64),
                  color=((n_px,), torch.int32), tri_index=((n_px,), torch.int32))
    out = [{k: torch.zeros(s, dtype=t, device=dev) for k, (s, t) in shapes.items()} for _ in range(2)]       # [0] the call's, [1] the baseline's

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def hooked(hook, fn):
        def run():
            g.debug_set(L.DBG_KERNEL_SWITCH, hook)
            try:
                fn()
            finally:
                g.debug_set(L.DBG_KERNEL_SWITCH, -1)
        return run

    doc = {"res": res, "triangles": args.triangles, "reps": args.reps, "hit_points": int(n), "sets": {}}
    for name, (starts, dirs, endpoints, limit_list, scan) in sets.items():
        m = starts.shape[0]
        D = (dirs - starts).contiguous() if endpoints else dirs                  # the baseline's directions: made here, not timed
        ptrs = [{k: out[i][k].data_ptr() for k in KEYS} for i in range(2)]
        for limit in limit_list:
            lim = torch.full((m,), limit, dtype=torch.float64, device=dev) if limit is not None else None

            def baseline():
                p = ptrs[1]
                g.trace_device(sa.MODE_BVH, m, starts.data_ptr(), D.data_ptr(), d_hit=p["hit"], d_ray_frac=p["ray_frac"], d_pos=p["pos"], d_normal=p["normal"],
                               d_color=p["color"], d_tri_index=p["tri_index"], stream=stream)
                if limit is not None:
                    o = out[1]
                    cut = ~((o["hit"][:m] != 0) & (o["ray_frac"][:m] <= limit))
                    o["hit"][:m].masked_fill_(cut, 0)
                    o["ray_frac"][:m].masked_fill_(cut, 0.0)
                    o["pos"][:m].masked_fill_(cut[:, None], 0.0)
                    o["normal"][:m].masked_fill_(cut[:, None], 0.0)
                    o["color"][:m].masked_fill_(cut, 0)
                    o["tri_index"][:m].masked_fill_(cut, -1)

            def nearest(coherent=False):
                p = ptrs[0]
                g.nearest_device(sa.MODE_BVH, m, starts.data_ptr(), dirs.data_ptr(), lim.data_ptr() if lim is not None else 0, p["hit"], p["ray_frac"], p["pos"],
                                 p["normal"], p["color"], p["tri_index"], endpoints=endpoints, coherent=coherent, stream=stream)

            variants = {"baseline": baseline, "nearest": nearest, "input_order": hooked(48, nearest), "per_lane": hooked(49, nearest)}
            if scan:
                variants["coherent"] = lambda: nearest(True)
            for t in [int(x) for x in args.refill.split(",") if x]:
                variants["refill_%d" % t] = hooked(100 + t, nearest)
            entry = {"rays": int(m), "limit": limit, "end_points": endpoints}
            for fn in variants.values():                                         # warm-up of every side
                timed(fn)
            baseline()
            torch.cuda.synchronize()
            entry["hits"] = int((out[1]["hit"][:m] != 0).sum().item())
            equal = {}
            for v, fn in variants.items():
                if v == "baseline":
                    continue
                for k in KEYS:
                    out[0][k].fill_(90)
                fn()
                torch.cuda.synchronize()
                equal[v] = all(bool(torch.equal(out[0][k][:m].view(torch.uint8), out[1][k][:m].view(torch.uint8))) for k in KEYS)
            entry["equal_to_baseline"] = equal
            key = name if limit is None else "%s_limit_%g" % (name, limit)
            if not all(equal.values()):
                doc["sets"][key] = entry
                doc["error"] = "outputs differ on " + key
                return doc                                                       # no time is quoted for outputs that differ
            times = {k: [] for k in variants}
            for _ in range(args.reps):
                for v, fn in variants.items():
                    times[v].append(timed(fn))
            entry["call_ms"] = {k: stats(v) for k, v in times.items()}
            med = {k: entry["call_ms"][k]["median"] for k in variants}
            entry["ratios"] = {"baseline_over_" + k: round(med["baseline"] / med[k], 3) for k in med if k != "baseline"}
            g.debug_set(L.DBG_KERNEL_TIMING, 1)
            kernels = {}
            for v, fn in variants.items():
                g.reset_kernel_times()
                timed(fn)
                kernels[v] = {k: round(t[0], 3) for k, t in g.kernel_times().items()}
            g.debug_set(L.DBG_KERNEL_TIMING, -1)
            entry["kernels_one_rep_ms"] = kernels
            st = torch.zeros(24, dtype=torch.int64, device=dev)
            for v, hook in (("nearest", -1), ("per_lane", 49)):
                g.debug_set(L.DBG_KERNEL_SWITCH, hook)
                p = ptrs[0]
                g.nearest_device(sa.MODE_BVH, m, starts.data_ptr(), dirs.data_ptr(), lim.data_ptr() if lim is not None else 0, p["hit"], p["ray_frac"], p["pos"],
                                 p["normal"], p["color"], p["tri_index"], endpoints=endpoints, stream=stream, d_stats_ptr=st.data_ptr())
                g.debug_set(L.DBG_KERNEL_SWITCH, -1)
                torch.cuda.synchronize()
                entry.setdefault("walk_counters", {})[v] = [int(x) for x in st[:4].cpu().tolist()]
            doc["sets"][key] = entry
            del lim
        del D
    return doc


if args.step:
    print("RESULT " + json.dumps(measure()))
    sys.exit(0)

cmd = [sys.executable, os.path.abspath(__file__), "--step", "measure", "--triangles", str(args.triangles), "--res", str(args.res), "--reps", str(args.reps),
       "--refill", args.refill]
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
