"""The frame G-buffer (sr_render_hits_device) measured on the GPU, on the unit-cube scene of the benchmark (SR_MODE_BVH, the benchmark's pose,
one sample per pixel, device arrays).

    python scripts/gpu_gbuffer.py [--out profiles/gbuffer/gbuffer.json]

One child process with a time limit of its own.  After a warm-up of every variant, `reps` repetitions in which the variants alternate, so that
drift of a shared machine hits them alike; every call is timed with an event pair on its stream:
  hits_all         sr_render_hits_device with all eight arrays (113 bytes per sample)
  hits_shadow_in   ... with pos + normal + hit only (what sr_shadow_points needs, 49 bytes per sample)
  hits_pick        ... with tri_index only (picking, 4 bytes per sample)
  hits_none        ... with no array (the walk alone, statistics off)
  trace_all / trace_shadow_in / trace_pick
                   the route without the call: the same outputs from sr_trace_rays_device (one lane per ray) over camera rays made with
                   torch beforehand (the making of the rays is timed on its own, `torch_rays`)
  frame_plain      sr_render_device, flags 0 (SR_F_NO_SPLIT): the same walk with 4 bytes stored per pixel -- the floor
  chain_shadowed   hits_shadow_in + colour, compaction in torch, sr_shade_points_device, sr_shadow_points_device (SR_POINTS_COHERENT), scatter
  frame_shadowed   sr_render_device of the shaded, shadowed frame: what the chain composes
A last repetition of the library's calls runs with SR_DBG_KERNEL_TIMING for the per-kernel event times.  The hits of the two routes and the
pixels of chain and frame are compared.  Reads neither the reference nor anything the oracle built."""
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
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["measure"], help="(internal) run the measurement in this process")
args = ap.parse_args()

SUBSETS = {"all": ("starts", "dirs", "hit", "ray_frac", "pos", "normal", "color", "tri_index"), "shadow_in": ("hit", "pos", "normal"), "pick": ("tri_index",),
           "none": ()}


def stats(xs):
    import numpy as np
    t = np.array(xs, dtype=np.float64)
    return {"median": round(float(np.median(t)), 3), "min": round(float(t.min()), 3), "max": round(float(t.max()), 3), "n": int(t.size)}


def frame(res, flags):
    import numpy as np
    import softray_amd as sa
    f = sa.Frame()
    f.width = f.height = res
    f.start_row, f.end_row = 0, res - 1
    f.sub_pixel_res = 1
    f.background_argb = 0xff00ff
    f.flags = flags | sa._lib.F_PRIMARY_STATS_ONLY | sa._lib.F_NO_SPLIT
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
    import torch
    import softray_amd as sa
    dev = torch.device("cuda", 0)
    g = sa.GpuScene(0)
    g.set_triangles(*sa.unit_cube_scene(args.triangles))
    g.build((sa.MODE_BVH,))
    res = args.res
    f_plain = frame(res, 0)
    f_lit = frame(res, sa.F_SHADING | sa.F_POINT_LIGHT | sa.F_SPECULAR | sa.F_SHADOWS)
    n = sa.GpuScene.sample_count(f_plain)
    stream = torch.cuda.current_stream().cuda_stream
    shapes = dict(starts=((n, 3), torch.float64), dirs=((n, 3), torch.float64), hit=((n,), torch.uint8), ray_frac=((n,), torch.float64),
                  pos=((n, 3), torch.float64), normal=((n, 3), torch.float64), color=((n,), torch.int32), tri_index=((n,), torch.int32))
    buf = {k: torch.zeros(s, dtype=t, device=dev) for k, (s, t) in shapes.items()}
    buf2 = {k: torch.zeros(s, dtype=t, device=dev) for k, (s, t) in shapes.items() if k not in ("starts", "dirs")}
    surface, surface2 = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def torch_rays():
        # the frame's one-sample camera rays restated in torch (Renderer.cs:1718-1723), as callers made them before the call existed
        it = torch.tensor([f_plain.inv_transform[i] for i in range(12)], dtype=torch.float64, device=dev).reshape(3, 4)
        cols = torch.arange(res, dtype=torch.float64, device=dev)
        dv = torch.empty((res, res, 3), dtype=torch.float64, device=dev)
        dv[:, :, 0] = -(cols / res - 0.5)[None, :]
        dv[:, :, 1] = (-(cols / res - 0.5) * (res / res))[:, None]
        dv[:, :, 2] = f_plain.fov_depth
        dirs = (dv.reshape(-1, 3) @ it[:, :3].T).contiguous()
        origin = it[:, :3] @ torch.tensor([0.0, 0.0, -f_plain.position_z], dtype=torch.float64, device=dev)
        return origin[None, :].expand(n, 3).contiguous(), dirs

    def hits(subset, into=buf):
        g.render_hits_device(f_plain, stream=stream, **{"d_" + k: into[k].data_ptr() for k in SUBSETS[subset]})

    rays = {}

    def trace(subset):
        ptr = {"d_" + k: buf2[k].data_ptr() for k in SUBSETS[subset] if k in buf2}
        g.trace_device(sa.MODE_BVH, n, rays["s"].data_ptr(), rays["d"].data_ptr(), stream=stream, **ptr)

    def chain():
        hits_for_chain()
        idx = torch.nonzero(buf["hit"]).reshape(-1)
        k = int(idx.numel())
        hp, hn, hc = buf["pos"][idx].contiguous(), buf["normal"][idx].contiguous(), buf["color"][idx].contiguous()
        surface2.fill_(-0xff01)                                                  # 0xFFFF00FF: the background with alpha
        g.shade_points_device(f_lit, k, hp.data_ptr(), hn.data_ptr(), hc.data_ptr(), hc.data_ptr(), stream=stream)
        g.shadow_points_device(f_lit, k, hp.data_ptr(), hn.data_ptr(), hc.data_ptr(), hc.data_ptr(), coherent=True, stream=stream)
        surface2[idx] = hc

    def hits_for_chain():
        g.render_hits_device(f_lit, d_hit=buf["hit"].data_ptr(), d_pos=buf["pos"].data_ptr(), d_normal=buf["normal"].data_ptr(), d_color=buf["color"].data_ptr(), stream=stream)

    variants = {}
    for s in SUBSETS:
        variants["hits_" + s] = (lambda s=s: hits(s))
    for s in ("all", "shadow_in", "pick"):
        variants["trace_" + s] = (lambda s=s: trace(s))
    variants["frame_plain"] = lambda: g.render_device(f_plain, surface.data_ptr(), stream)
    variants["chain_shadowed"] = chain
    variants["frame_shadowed"] = lambda: g.render_device(f_lit, surface.data_ptr(), stream)

    t_rays = []
    for _ in range(3):
        t_rays.append(timed(lambda: rays.update(zip(("s", "d"), torch_rays()))))
    # warm-up of every variant, and the comparisons
    for fn in variants.values():
        timed(fn)
    hits("all"); trace("all"); torch.cuda.synchronize()
    equal = {k: bool(torch.equal(buf[k], buf2[k])) for k in buf2}
    equal["starts"] = bool(torch.equal(buf["starts"], rays["s"]))
    equal["dirs"] = bool(torch.equal(buf["dirs"], rays["d"]))
    hit_count = int(buf["hit"].sum().item())
    chain(); g.render_device(f_lit, surface.data_ptr(), stream); torch.cuda.synchronize()
    chain_differs = int((surface != surface2).sum().item())
    times = {k: [] for k in variants}
    for _ in range(args.reps):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    g.debug_set(sa._lib.DBG_KERNEL_TIMING, 1)
    kernels = {}
    for name, fn in variants.items():
        g.reset_kernel_times()
        timed(fn)
        kernels[name] = {k: round(v[0], 3) for k, v in g.kernel_times().items()}
    g.debug_set(sa._lib.DBG_KERNEL_TIMING, -1)
    med = {k: stats(v) for k, v in times.items()}
    doc = {"res": res, "triangles": args.triangles, "samples": n, "hits": hit_count, "shadow_samples": args.samples,
           "hits_equal_trace_rays": equal, "chain_pixels_differing_from_frame": chain_differs,
           "torch_rays_ms": stats(t_rays), "call_ms": med, "kernels_one_rep_ms": kernels,
           "bytes_per_sample": {"hits_all": 113, "hits_shadow_in": 49, "hits_pick": 4, "frame_plain": 4},
           "ratios": {"hits_all_over_frame_plain": round(med["hits_all"]["median"] / med["frame_plain"]["median"], 3),
                      "hits_none_over_frame_plain": round(med["hits_none"]["median"] / med["frame_plain"]["median"], 3),
                      "trace_all_over_hits_all": round(med["trace_all"]["median"] / med["hits_all"]["median"], 3),
                      "trace_shadow_in_over_hits_shadow_in": round(med["trace_shadow_in"]["median"] / med["hits_shadow_in"]["median"], 3),
                      "trace_pick_over_hits_pick": round(med["trace_pick"]["median"] / med["hits_pick"]["median"], 3),
                      "chain_over_frame_shadowed": round(med["chain_shadowed"]["median"] / med["frame_shadowed"]["median"], 3)},
           "primary_rays_per_s": {k: round(n / (med[k]["median"] * 1e-3)) for k in ("hits_all", "hits_shadow_in", "hits_pick", "hits_none", "trace_all", "frame_plain")}}
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
