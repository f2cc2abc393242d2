"""sr_bake_light_field measured on the GPU, on the unit-cube scene of the benchmark (SR_MODE_BVH, N = 64: 4 x 64^4 = 67 M canonical rays):

    python scripts/gpu_lightfield_bake.py [--out profiles/lightfield_bake/bake.json]

Two child processes, each with a time limit of its own, `reps` timed repetitions each after a warm-up:
  bake    the whole table on an empty light field (sr_reset_light_field before every timed bake, so the call also zeroes the 256 MiB table),
          shading off and on, with the per-lane walk (production) and with the packet walk (SR_DBG_KERNEL_SWITCH 35) -- the four variants
          alternate inside every repetition, so that drift of the shared machine hits them alike.  Recorded: the call's time (host clock
          around the blocking call), the sum of k_lf_bake's HIP event pairs and their number, canonical rays per second from both, and
          whether the two walks left the same table (a 64-bit sum and the xor of the entries read back after the warm-up bakes).
  frames  at res x res: the plain SR_MODE_BVH frame without shadows (the project's yardstick for primary rays per second), the light-field
          frame on an empty table (cold, lazy fill) and the same frame after a bake (look-ups only).
A failing or overrunning child ends the script: nothing more is started on the GPU after it.
`--step one` (internal, also what a profiler is pointed at: `rocprofv3 --kernel-trace --stats -- python scripts/gpu_lightfield_bake.py --step one`)
runs one warm-up bake and one timed bake.  Reads neither the reference nor anything the oracle built.
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
ap.add_argument("--lf-res", type=int, default=64, help="N of the light field's 4 N^4 entries")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["bake", "frames", "one"], help="(internal) run one step in this process")
args = ap.parse_args()
PACKET = 35                                  # SR_DBG_KERNEL_SWITCH: the bake with one packet walk per wave


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
    g.light_field_res = args.lf_res
    return g


def frame(res, light_field, shading=True):
    import numpy as np
    import softray_amd as sa
    f = sa.Frame()
    f.width = f.height = res
    f.start_row, f.end_row = 0, res - 1
    f.sub_pixel_res = 1
    f.background_argb = 0xff00ff
    f.flags = (sa.F_SHADING if shading else 0) | sa.F_POINT_LIGHT | sa.F_SPECULAR | (sa.F_LIGHT_FIELD if light_field else 0)
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


def timed_bake(g, f, packet):
    """One whole-table bake on an empty light field: (call ms, k_lf_bake event ms, launches, entries written)."""
    import softray_amd as sa
    g.debug_set(sa._lib.DBG_KERNEL_SWITCH, PACKET if packet else -1)
    try:
        g.reset_light_field()
        g.reset_kernel_times()
        t0 = time.perf_counter()
        filled = g.bake_light_field(f)                                # blocks
        ms = (time.perf_counter() - t0) * 1e3
    finally:
        g.debug_set(sa._lib.DBG_KERNEL_SWITCH, -1)
    k = g.kernel_times().get("k_lf_bake", (0.0, 0))
    return ms, k[0], k[1], filled


def digest(g):
    """(sum, xor) over the table's entries as 64-bit integers."""
    import numpy as np
    table = g.get_light_field()
    return int(table.astype(np.uint64).sum()), int(np.bitwise_xor.reduce(table))


def step_bake():
    g = make_scene()
    total = 4 * args.lf_res ** 4
    variants = [(shading, packet) for shading in (False, True) for packet in (False, True)]
    name = lambda v: ("shading" if v[0] else "no_shading") + ("_packet" if v[1] else "_per_lane")
    digests = {}
    for v in variants:                                                # warm-up of every kernel, and the tables' digests
        _, _, _, filled = timed_bake(g, frame(16, True, v[0]), v[1])
        assert filled == total, (filled, total)
        digests[name(v)] = digest(g)
    call, kern, launches = {name(v): [] for v in variants}, {name(v): [] for v in variants}, {}
    for _ in range(args.reps):
        for v in variants:
            ms, kms, n, filled = timed_bake(g, frame(16, True, v[0]), v[1])
            assert filled == total
            call[name(v)].append(ms); kern[name(v)].append(kms); launches[name(v)] = n
    doc = {"triangles": args.triangles, "light_field_res": args.lf_res, "entries": total, "variants": {},
           "same_table_no_shading": digests["no_shading_packet"] == digests["no_shading_per_lane"],
           "same_table_shading": digests["shading_packet"] == digests["shading_per_lane"]}
    for v in variants:
        c, k = stats(call[name(v)]), stats(kern[name(v)])
        doc["variants"][name(v)] = {"call_ms": c, "k_lf_bake_ms": k, "launches": launches[name(v)],
                                    "canonical_rays_per_s_call": round(total / (c["median"] * 1e-3), 0),
                                    "canonical_rays_per_s_kernel": round(total / (k["median"] * 1e-3), 0) if k["median"] > 0 else 0}
    return doc


def timed_frame(g, f, surface, stream):
    import torch
    g.reset_kernel_times()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.render_device(f, surface.data_ptr(), stream)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    kt = g.kernel_times()
    return ms, {k: round(v[0], 3) for k, v in kt.items()}


def step_frames():
    import torch
    g = make_scene()
    res = args.res
    surface = torch.zeros(res * res, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    fl, fp = frame(res, True), frame(res, False)
    g.bake_light_field(fl)                                            # warm-up of every kernel
    timed_frame(g, fl, surface, stream)
    timed_frame(g, fp, surface, stream)
    g.reset_light_field()
    timed_frame(g, fl, surface, stream)
    plain, cold, baked = [], [], []
    kernels = {}
    for _ in range(args.reps):
        ms, kernels["plain"] = timed_frame(g, fp, surface, stream)
        plain.append(ms)
        g.reset_light_field()
        ms, kernels["cold_lazy"] = timed_frame(g, fl, surface, stream)
        cold.append(ms)
        g.reset_light_field()
        g.bake_light_field(fl)
        ms, kernels["after_bake"] = timed_frame(g, fl, surface, stream)
        baked.append(ms)
    p = stats(plain)
    return {"res": res, "triangles": args.triangles, "light_field_res": args.lf_res, "plain_frame_ms": p,
            "plain_primary_rays_per_s": round(res * res / (p["median"] * 1e-3), 0),
            "lightfield_cold_lazy_frame_ms": stats(cold), "lightfield_after_bake_frame_ms": stats(baked), "kernels_last_rep_ms": kernels}


def step_one():
    g = make_scene()
    f = frame(16, True)
    timed_bake(g, f, False)
    ms, kms, n, filled = timed_bake(g, f, False)
    return {"triangles": args.triangles, "light_field_res": args.lf_res, "call_ms": round(ms, 3), "k_lf_bake_ms": round(kms, 3), "launches": n, "filled": filled}


if args.step:
    print("RESULT " + json.dumps({"bake": step_bake, "frames": step_frames, "one": step_one}[args.step]()))
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


doc = {"bake": child("bake", 420.0)}
doc["frames"] = child("frames", 300.0)
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
