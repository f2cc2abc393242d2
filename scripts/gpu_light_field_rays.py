"""Light-field colours for caller-given rays (sr_light_field_rays_device) measured on the GPU, on the unit-cube scene of the benchmark
(1 M triangles, SR_MODE_BVH, N = 64, device arrays).

    python scripts/gpu_light_field_rays.py [--out profiles/light_field_rays/light_field_rays.json]

Two child processes, each with a time limit of its own; inside a step every run is timed with an event pair on its stream and the sides of a
comparison alternate inside every repetition, so that drift of the shared machine hits them alike:
  camera    the res x res camera rays of the benchmark's pose (sr_render_hits_device's starts / dirs; not timed) through the call against
            sr_render_device's light-field frame -- the unfused lookup / fill / apply, which reads no ray from memory -- on the baked table,
            nearest and interpolated; the same rays randomly permuted; and both from an EMPTY table (sr_reset_light_field before every run:
            zeroing the 4 N^4 entries is part of either side's time).  Before any time is taken the call's colours are compared with the frame's
            pixels, and the permuted call's with the permutation of them.
  panorama  a res x res/2 equirectangular panorama from the box centre through the call on a baked table,
            against the route without it: sr_trace_origin_rays_device + sr_shade_points_device; with the table baked with dynamic shadows
            (sr_set_light_field_shadows), against those plus sr_shadow_points_device.  The two routes do not compute the same thing -- a table
            entry is the colour of its cell's canonical ray -- so the share of equal colours is recorded, not required.
A failing or overrunning child ends the script: nothing more is started on the GPU after it.  Reads neither the reference nor the oracle."""
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
ap.add_argument("--lf-res", type=int, default=64, help="N of the light field's 4 N^4 entries")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["camera", "panorama"], help="(internal) run one step in this process")
args = ap.parse_args()

HBM_PEAK_TBS, HBM_MEASURED_TBS = 8.0, 6.29       # MI355X: specification, and a measured float4 copy


def stats(xs):
    import numpy as np
    t = np.array(xs, dtype=np.float64)
    return {"median": round(float(np.median(t)), 3), "min": round(float(t.min()), 3), "max": round(float(t.max()), 3), "n": int(t.size)}


def make_scene():
    import softray_amd as sa
    g = sa.GpuScene(0)
    g.set_triangles(*sa.unit_cube_scene(args.triangles))
    g.build((sa.MODE_BVH,))
    g.light_field_res = args.lf_res
    return g


def frame(res, light_field, shadows=False):
    import numpy as np
    import softray_amd as sa
    f = sa.Frame()
    f.width = f.height = res
    f.start_row, f.end_row = 0, res - 1
    f.sub_pixel_res = 1
    f.background_argb = 0xff00ff
    f.flags = sa.F_SHADING | sa.F_POINT_LIGHT | sa.F_SPECULAR | sa._lib.F_PRIMARY_STATS_ONLY | (sa.F_LIGHT_FIELD if light_field else 0) | (sa.F_SHADOWS if shadows else 0)
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


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(variants, reps, before=None):
    """`reps` runs of every variant, the variants alternating; `before` (not timed) runs ahead of each."""
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            if before:
                before()
            times[k].append(timed(fn))
    return {k: stats(v) for k, v in times.items()}


def kernel_times(g, variants, before=None):
    import softray_amd as sa
    g.debug_set(sa._lib.DBG_KERNEL_TIMING, 1)
    out = {}
    for k, fn in variants.items():
        if before:
            before()
        g.reset_kernel_times()
        timed(fn)
        out[k] = {name: round(t[0], 3) for name, t in g.kernel_times().items()}
    g.debug_set(sa._lib.DBG_KERNEL_TIMING, -1)
    return out


def step_camera():
    import torch
    import softray_amd as sa
    dev = torch.device("cuda", 0)
    g = make_scene()
    res, n = args.res, args.res * args.res
    stream = torch.cuda.current_stream().cuda_stream
    fl, fp = frame(res, True), frame(res, False)
    d_starts = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    d_dirs = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    g.render_hits_device(fp, d_starts=d_starts.data_ptr(), d_dirs=d_dirs.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345)
    perm = torch.randperm(n, device=dev, generator=gen)
    p_starts, p_dirs = d_starts[perm].contiguous(), d_dirs[perm].contiguous()
    px = torch.zeros(n, dtype=torch.int32, device=dev)
    out = torch.zeros(n, dtype=torch.int32, device=dev)
    p_out = torch.zeros(n, dtype=torch.int32, device=dev)
    inside = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_filled = torch.zeros(1, dtype=torch.int64, device=dev)
    total = 4 * args.lf_res ** 4
    doc = {"res": res, "triangles": args.triangles, "light_field_res": args.lf_res, "rays": n, "reps": args.reps,
           "hbm_tb_s": {"specification": HBM_PEAK_TBS, "measured_copy": HBM_MEASURED_TBS}}

    def frame_fn():
        g.render_device(fl, px.data_ptr(), stream)

    def call_fn():
        g.light_field_rays_device(fl, n, d_starts.data_ptr(), d_dirs.data_ptr(), out.data_ptr(), inside.data_ptr(), stream=stream, d_filled_ptr=d_filled.data_ptr())

    def permuted_fn():
        g.light_field_rays_device(fl, n, p_starts.data_ptr(), p_dirs.data_ptr(), p_out.data_ptr(), inside.data_ptr(), stream=stream)

    variants = {"frame": frame_fn, "call": call_fn, "call_permuted": permuted_fn}
    for interp in (False, True):
        key = "interpolated" if interp else "nearest"
        g.light_field_interpolation = interp
        g.reset_light_field()
        assert g.bake_light_field(fl) == total
        for fn in variants.values():                                             # warm-up of every side
            timed(fn)
        px.fill_(0x5A5A5A5A); out.fill_(0x3C3C3C3C); p_out.fill_(0x3C3C3C3C)
        frame_fn(); call_fn(); permuted_fn()
        torch.cuda.synchronize()
        entry = {"equal_to_frame": {"call": bool(torch.equal(out, px)), "call_permuted": bool(torch.equal(p_out, px[perm]))},
                 "inside": int(inside.sum().item()), "filled_on_baked_table": int(d_filled.item())}
        doc[key] = entry
        if not all(entry["equal_to_frame"].values()) or entry["filled_on_baked_table"] != 0:
            doc["error"] = "outputs differ from the frame's (%s)" % key
            return doc                                                           # no time is quoted for outputs that differ
        entry["baked_ms"] = alternate(variants, args.reps)
        entry["baked_kernels_one_run_ms"] = kernel_times(g, variants)
        # what the call must move at the least: 48 bytes of ray in, 4 of colour and 1 of `inside` out, and the entries gathered (4 or 16 x 4 bytes,
        # before any reuse in the caches)
        moved = n * (48 + 4 + 1 + (64 if interp else 4))
        entry["bytes_moved_at_least"] = moved
        for k in ("call", "call_permuted"):
            tb_s = moved / (entry["baked_ms"][k]["median"] * 1e-3) / 1e12
            entry.setdefault("tb_per_s", {})[k] = round(tb_s, 3)
            entry.setdefault("share_of_measured_hbm_copy", {})[k] = round(tb_s / HBM_MEASURED_TBS, 3)
        # from an empty table
        cold = {"frame": frame_fn, "call": call_fn}
        g.reset_light_field(); frame_fn(); torch.cuda.synchronize()
        cold_px = px.clone()
        table = g.get_light_field()
        g.reset_light_field(); call_fn(); torch.cuda.synchronize()
        entry["cold"] = {"equal_to_frame": bool(torch.equal(out, cold_px)), "filled": int(d_filled.item()),
                         "same_table": bool((g.get_light_field() == table).all())}
        del table
        if not (entry["cold"]["equal_to_frame"] and entry["cold"]["same_table"]):
            doc["error"] = "cold outputs differ from the frame's (%s)" % key
            return doc
        entry["cold"]["ms"] = alternate(cold, args.reps, before=g.reset_light_field)
        entry["cold"]["kernels_one_run_ms"] = kernel_times(g, cold, before=g.reset_light_field)
    g.light_field_interpolation = False
    return doc


def step_panorama():
    import math
    import torch
    import softray_amd as sa
    dev = torch.device("cuda", 0)
    g = make_scene()
    W, H = args.res, args.res // 2
    n = W * H
    stream = torch.cuda.current_stream().cuda_stream
    j, i = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    T = (i.reshape(-1) + 0.5) / W * (2 * math.pi)
    P = ((j.reshape(-1) + 0.5) / H - 0.5) * math.pi
    dirs = torch.stack([torch.sin(T) * torch.cos(P), torch.sin(P), torch.cos(T) * torch.cos(P)], dim=1).contiguous()
    del i, j, T, P
    eye = [0.0, 0.0, 0.0]
    starts = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    out = torch.zeros(n, dtype=torch.int32, device=dev)
    t_hit = torch.zeros(n, dtype=torch.uint8, device=dev)
    t_pos = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    t_nrm = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    t_col = torch.zeros(n, dtype=torch.int32, device=dev)
    shaded = torch.zeros(n, dtype=torch.int32, device=dev)
    total = 4 * args.lf_res ** 4
    doc = {"width": W, "height": H, "triangles": args.triangles, "light_field_res": args.lf_res, "rays": n, "reps": args.reps, "eye": eye}
    fp, fs = frame(16, False), frame(16, False, True)
    for shadows in (False, True):
        key = "shadowed_table" if shadows else "plain_table"
        g.light_field_shadows = shadows
        fl = frame(16, True, shadows)
        g.reset_light_field()
        assert g.bake_light_field(fl) == total

        def call_fn():
            g.light_field_rays_device(fl, n, starts.data_ptr(), dirs.data_ptr(), out.data_ptr(), 0, stream=stream)

        def traced_fn():
            g.trace_origin_device(sa.MODE_BVH, eye, n, dirs.data_ptr(), d_hit=t_hit.data_ptr(), d_pos=t_pos.data_ptr(), d_normal=t_nrm.data_ptr(),
                                  d_color=t_col.data_ptr(), stream=stream)
            g.shade_points_device(fp, n, t_pos.data_ptr(), t_nrm.data_ptr(), t_col.data_ptr(), shaded.data_ptr(), stream=stream)
            if shadows:
                g.shadow_points_device(fs, n, t_pos.data_ptr(), t_nrm.data_ptr(), shaded.data_ptr(), shaded.data_ptr(), stream=stream)

        variants = {"call": call_fn, "traced": traced_fn}
        for fn in variants.values():
            timed(fn)
        call_fn(); traced_fn()
        torch.cuda.synchronize()
        hit = t_hit != 0
        entry = {"hits": int(hit.sum().item()), "equal_colour_share_of_hits": round(float((out[hit] == shaded[hit]).double().mean().item()), 4)}
        entry["ms"] = alternate(variants, args.reps)
        entry["traced_over_call"] = round(entry["ms"]["traced"]["median"] / entry["ms"]["call"]["median"], 2)
        entry["kernels_one_run_ms"] = kernel_times(g, variants)
        doc[key] = entry
    return doc


if args.step:
    print("RESULT " + json.dumps({"camera": step_camera, "panorama": step_panorama}[args.step]()))
    sys.exit(0)


def child(step, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--triangles", str(args.triangles), "--res", str(args.res),
           "--lf-res", str(args.lf_res), "--reps", str(args.reps)]
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


doc = {"camera": child("camera", 300.0)}
if "error" not in doc["camera"]:
    doc["panorama"] = child("panorama", 300.0)
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
if "error" in doc["camera"]:
    raise SystemExit(doc["camera"]["error"])
