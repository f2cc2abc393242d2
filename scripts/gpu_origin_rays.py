"""Ray batches from one origin (sr_trace_origin_rays_device) measured on the GPU, on the unit-cube scene of the benchmark (1 M triangles,
SR_MODE_BVH, device arrays, all six outputs).

    python scripts/gpu_origin_rays.py [--out profiles/origin_rays/origin_rays.json]
    python scripts/gpu_origin_rays.py --tree OTHER_CHECKOUT --only-baseline [--out ...]     # sr_trace_rays_device of another build (the parent's)

One child process with a time limit of its own.  Ray sets:
  pinhole_scan    the 4096^2 frame's own directions (sr_render_hits_device), scan order
  pinhole_tiles   the same in 8x8-tile-major order
  pano_camera     a 4096 x 2048 equirectangular panorama from the frame's camera position, scan order
  pano_centre     the same from the box centre
  pinhole_random  pinhole_scan randomly permuted
Per set, after a warm-up of every variant, `reps` repetitions in which the variants alternate, every call timed with an event pair on its stream:
  origin_sorted   the new call without options
  origin_coherent the new call with SR_RAYS_COHERENT, where the order allows the promise (not pinhole_random)
  trace_rays      sr_trace_rays_device on the same rays with the origin tiled (one private walk per lane): the baseline
  render_hits     pinhole sets only: sr_render_hits_device with the same six outputs, the floor
and, once per set, `rekeyed`: the call right after a call from another origin (the per-origin pre-passes run) against the repeated call.
The answers of origin_sorted, origin_coherent and trace_rays are compared, all six arrays.  Reads neither the reference nor the oracle."""
import argparse
import json
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=4096)
ap.add_argument("--triangles", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--tree", default=None, help="the checkout whose softray_amd is measured (default: this one)")
ap.add_argument("--only-baseline", action="store_true", help="sr_trace_rays_device alone (a build without the new call)")
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["measure"], help="(internal) run the measurement in this process")
args = ap.parse_args()

ROOT = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    import numpy as np
    import torch
    import softray_amd as sa
    dev = torch.device("cuda", 0)
    g = sa.GpuScene(0)
    g.set_triangles(*sa.unit_cube_scene(args.triangles))
    g.build((sa.MODE_BVH,))
    res = args.res
    f = frame(res)
    n_px = res * res
    stream = torch.cuda.current_stream().cuda_stream
    # the library's own camera rays: what the frame's walk answers
    it = np.array([f.inv_transform[i] for i in range(12)]).reshape(3, 4)
    cam = it[:, :3] @ np.array([0.0, 0.0, -f.position_z])
    d_scan = torch.zeros((n_px, 3), dtype=torch.float64, device=dev)
    if args.only_baseline:
        cols = torch.arange(res, dtype=torch.float64, device=dev)
        dv = torch.empty((res, res, 3), dtype=torch.float64, device=dev)
        dv[:, :, 0] = -(cols / res - 0.5)[None, :]
        dv[:, :, 1] = -(cols / res - 0.5)[:, None]
        dv[:, :, 2] = f.fov_depth
        d_scan = (dv.reshape(-1, 3) @ torch.tensor(it[:, :3].T.copy(), device=dev)).contiguous()
    else:
        g.render_hits_device(f, d_dirs=d_scan.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    ys, xs = torch.meshgrid(torch.arange(res, device=dev), torch.arange(res, device=dev), indexing="ij")
    tile_key = ((ys // 8) * (res // 8) + xs // 8) * 64 + (ys % 8) * 8 + xs % 8
    tile_idx = torch.argsort(tile_key.reshape(-1))
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345)
    lon = (torch.arange(res, dtype=torch.float64, device=dev) + 0.5) * (2.0 * np.pi / res)
    lat = ((torch.arange(res // 2, dtype=torch.float64, device=dev) + 0.5) / (res // 2) - 0.5) * np.pi
    pano = torch.stack([(torch.cos(lat)[:, None] * torch.cos(lon)[None, :]), torch.sin(lat)[:, None].expand(res // 2, res),
                        (torch.cos(lat)[:, None] * torch.sin(lon)[None, :])], dim=-1).reshape(-1, 3).contiguous()
    sets = {"pinhole_scan": (cam, d_scan, True, True), "pinhole_tiles": (cam, d_scan[tile_idx].contiguous(), True, True),
            "pano_camera": (cam, pano, True, False), "pano_centre": (np.zeros(3), pano, True, False),
            "pinhole_random": (cam, d_scan[torch.randperm(n_px, device=dev, generator=gen)].contiguous(), False, False)}
    del ys, xs, tile_key
    shapes = dict(hit=((n_px,), torch.uint8), ray_frac=((n_px,), torch.float64), pos=((n_px, 3), torch.float64), normal=((n_px, 3), torch.float64),
                  color=((n_px,), torch.int32), tri_index=((n_px,), torch.int32))
    buf = [{k: torch.zeros(s, dtype=t, device=dev) for k, (s, t) in shapes.items()} for _ in range(2)]
    ptrs = lambda b: {"d_" + k: b[k].data_ptr() for k in KEYS}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    doc = {"res": res, "triangles": args.triangles, "reps": args.reps, "tree": "other" if args.tree else "this", "sets": {}}
    for name, (origin, dirs, may_promise, is_frame) in sets.items():
        n = dirs.shape[0]
        starts = torch.tensor(origin, dtype=torch.float64, device=dev)[None, :].expand(n, 3).contiguous()
        variants = {"trace_rays": lambda: g.trace_device(sa.MODE_BVH, n, starts.data_ptr(), dirs.data_ptr(), stream=stream, **ptrs(buf[1]))}
        if not args.only_baseline:
            variants["origin_sorted"] = lambda: g.trace_origin_device(sa.MODE_BVH, origin, n, dirs.data_ptr(), stream=stream, **ptrs(buf[0]))
            if may_promise:
                variants["origin_coherent"] = lambda: g.trace_origin_device(sa.MODE_BVH, origin, n, dirs.data_ptr(), coherent=True, stream=stream, **ptrs(buf[0]))
            if is_frame:
                variants["render_hits"] = lambda: g.render_hits_device(f, stream=stream, **ptrs(buf[0]))
        entry = {"rays": int(n), "origin": [float(x) for x in origin]}
        for fn in variants.values():
            timed(fn)
        variants["trace_rays"]()
        torch.cuda.synchronize()
        entry["hits"] = int(buf[1]["hit"][:n].sum().item())
        if not args.only_baseline:
            equal = {}
            for v in ("origin_sorted", "origin_coherent"):
                if v in variants:
                    for b in buf[0].values():
                        b.zero_()
                    variants[v]()
                    torch.cuda.synchronize()
                    equal[v] = {k: bool(torch.equal(buf[0][k][:n], buf[1][k][:n])) for k in KEYS}
            entry["equal_to_trace_rays"] = equal
            # the call right after a call from elsewhere (the per-origin pre-passes run) against the repeated call
            other = np.asarray(origin) + np.array([0.25, -0.125, 0.375])
            rekeyed = []
            for _ in range(5):
                g.trace_origin_device(sa.MODE_BVH, other, 64, dirs.data_ptr(), stream=stream)
                torch.cuda.synchronize()
                rekeyed.append(timed(variants["origin_sorted"]))
            entry["rekeyed_ms"] = stats(rekeyed)
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for v, fn in variants.items():
                times[v].append(timed(fn))
        entry["call_ms"] = {k: stats(v) for k, v in times.items()}
        med = {k: entry["call_ms"][k]["median"] for k in variants}
        entry["ratios"] = {"trace_rays_over_" + k: round(med["trace_rays"] / med[k], 3) for k in med if k != "trace_rays"}
        if not args.only_baseline:
            g.debug_set(sa._lib.DBG_KERNEL_TIMING, 1)
            kernels = {}
            for v, fn in variants.items():
                g.reset_kernel_times()
                timed(fn)
                kernels[v] = {k: round(t[0], 3) for k, t in g.kernel_times().items()}
            g.debug_set(sa._lib.DBG_KERNEL_TIMING, -1)
            entry["kernels_one_rep_ms"] = kernels
        doc["sets"][name] = entry
        del starts
    return doc


if args.step:
    print("RESULT " + json.dumps(measure()))
    sys.exit(0)

cmd = [sys.executable, os.path.abspath(__file__), "--step", "measure", "--triangles", str(args.triangles), "--res", str(args.res), "--reps", str(args.reps)]
if args.tree:
    cmd += ["--tree", args.tree]
if args.only_baseline:
    cmd += ["--only-baseline"]
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
