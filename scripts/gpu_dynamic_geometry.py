"""A deforming model re-rendered every frame, measured on the GPU: per update step "new vertices -> sr_build(SR_MODE_BVH) -> one plain
res x res frame" on the benchmark's unit-cube soup (1 M triangles), through the ways in:

    python scripts/gpu_dynamic_geometry.py [--out profiles/bvh_refit/update.json]
    python scripts/gpu_dynamic_geometry.py --quality [--out profiles/bvh_refit/frames.json]

  host         the vertices are a PINNED numpy array handed to sr_set_triangles: the host copies them, computes the records and the
               bounds in serial loops and uploads both arrays at the next sr_build
  device       the vertices are a torch tensor on the device handed to sr_set_triangles_device (k_tri_records + the bounds kernels)
  device_keep  the same with argb = None: every triangle keeps its colour
  device_refit the same tensor handed to sr_refit_triangles_device (argb = None): the tree of the warm-up update is refit, there is no
               sr_build ("build_ms" is 0, "set_ms" is the refit call; k_refit_leaves / k_refit_nodes are its kernels)

--quality measures what a refit tree costs a FRAME: the soup is built, every vertex is moved by up to 1 % (then 10 %) of the box, and the
plain frame and the 100-sample shadow frame are timed on the refit tree and again after sr_build, in one child process per deformation.

The routes alternate, `--reps` rounds; every (round, route) is a CHILD PROCESS under `timeout -k 10` that warms up with one update and
then times `--inner` updates (host clock around each blocking call, the device idle before and after; the new kernels' HIP event times
through SR_DBG_KERNEL_TIMING).  Every update uses another seeded displacement of the soup, the same ones on every route, and the frames'
CRC-32 must agree between the routes.  The first child that fails or overruns ends the script: nothing more is started on the GPU.
Reads neither the reference nor anything the oracle built.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=4096)
ap.add_argument("--triangles", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=3, help="timed updates per child process")
ap.add_argument("--limit", type=float, default=150.0, help="time limit of one child process, seconds")
ap.add_argument("--out", default=None)
ap.add_argument("--quality", action="store_true", help="frame times on a refit tree against a rebuilt tree instead of the update times")
ap.add_argument("--step", default=None, choices=["host", "device", "device_keep", "device_refit", "quality_0.01", "quality_0.1"],
                help="(internal) run one route in this process")
args = ap.parse_args()
ROUTES = ("host", "device", "device_keep", "device_refit")


def frame(res, shadows=False):
    import numpy as np
    import softray_amd as sa
    f = sa.Frame()
    f.width = f.height = res
    f.start_row, f.end_row = 0, res - 1
    f.sub_pixel_res = 1
    f.background_argb = 0xff00ff
    f.flags = sa.F_SHADING | sa.F_POINT_LIGHT | sa.F_SPECULAR | (sa.F_SHADOWS if shadows else 0)
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


def step(route):
    import numpy as np
    import torch
    import softray_amd as sa
    v9, argb, bmin, bmax = sa.unit_cube_scene(args.triangles)
    bmin, bmax = bmin - 0.05, bmax + 0.05                                 # room for the displacements
    rnd = np.random.RandomState(2024)
    sets = [v9 + rnd.uniform(-0.02, 0.02, size=(1, 1, 3)) + rnd.uniform(-0.005, 0.005, size=(args.triangles, 1, 3)) for _ in range(args.inner + 1)]
    g = sa.GpuScene(0)
    g.debug_set(sa._lib.DBG_KERNEL_TIMING, 1)
    f = frame(args.res)
    surface = torch.zeros(args.res * args.res, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    if route == "host":
        pinned = [torch.from_numpy(np.ascontiguousarray(s)).pin_memory() for s in sets]
        sets = [p.numpy() for p in pinned]
    else:
        sets = [torch.from_numpy(np.ascontiguousarray(s)).to("cuda:0") for s in sets]
        d_argb = torch.from_numpy(argb.view(np.int32)).to("cuda:0")
    rows = []
    for k, verts in enumerate(sets):                                      # update 0 is the warm-up (and gives device_keep its colours)
        torch.cuda.synchronize()
        g.reset_kernel_times()
        t0 = time.perf_counter()
        if route == "host":
            g.set_triangles(verts, argb, bmin, bmax)
        elif route == "device_refit" and k > 0:
            g.refit_triangles_device(verts, None, bmin, bmax, stream)
        else:
            g.set_triangles_device(verts, None if (route == "device_keep" and k > 0) else d_argb, bmin, bmax, stream)
        t1 = time.perf_counter()
        if not (route == "device_refit" and k > 0):
            g.build((sa.MODE_BVH,))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        g.render_device(f, surface.data_ptr(), stream)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        kt = g.kernel_times()
        rows.append({"set_ms": (t1 - t0) * 1e3, "build_ms": (t2 - t1) * 1e3, "frame_ms": (t3 - t2) * 1e3, "update_ms": (t3 - t0) * 1e3,
                     "k_tri_records_ms": kt.get("k_tri_records", (0.0, 0))[0], "k_tri_bounds_ms": kt.get("k_tri_bounds", (0.0, 0))[0],
                     "k_refit_leaves_ms": kt.get("k_refit_leaves", (0.0, 0))[0], "k_refit_nodes_ms": kt.get("k_refit_nodes", (0.0, 0))[0],
                     "crc": zlib.crc32(surface.cpu().numpy().tobytes())})
    assert g.bvh_stats()[3] == 1
    return {"route": route, "triangles": args.triangles, "res": args.res, "updates": rows[1:]}


def quality(amount):
    """Frame times on the tree refit to a deformation of `amount` x the box, and on the tree rebuilt for it; the frames must agree."""
    import numpy as np
    import torch
    import softray_amd as sa
    v9, argb, bmin, bmax = sa.unit_cube_scene(args.triangles)
    bmin, bmax = bmin - 0.1, bmax + 0.1
    moved = v9 + np.random.RandomState(7).uniform(-amount, amount, size=v9.shape)      # every VERTEX on its own: triangles change shape
    g = sa.GpuScene(0)
    g.set_triangles(v9, argb, bmin, bmax)
    g.build((sa.MODE_BVH,))
    assert g.bvh_stats()[3] == 1
    surface = torch.zeros(args.res * args.res, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    frames = {"plain": frame(args.res), "shadows100": frame(args.res, shadows=True)}

    def timed():
        out = {}
        for name, f in frames.items():
            ms = []
            for _ in range(1 + args.inner):                               # the first one warms the per-origin records up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                g.render_device(f, surface.data_ptr(), stream)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            out[name + "_ms"] = median(ms[1:])
            out[name + "_crc"] = zlib.crc32(surface.cpu().numpy().tobytes())
        return out
    built = timed()
    g.refit_triangles_device(torch.from_numpy(np.ascontiguousarray(moved)).to("cuda:0"), None, bmin, bmax, stream)
    refit = timed()
    g.build((sa.MODE_BVH,))
    rebuilt = timed()
    return {"amount": amount, "triangles": args.triangles, "res": args.res, "undeformed": built, "refit": refit, "rebuilt": rebuilt,
            "same_frames": all(refit[k] == rebuilt[k] for k in refit if k.endswith("_crc"))}


def median(xs):
    xs = sorted(xs)
    m = len(xs) // 2
    return xs[m] if len(xs) % 2 else 0.5 * (xs[m - 1] + xs[m])


if args.step:
    print("RESULT " + json.dumps(quality(float(args.step[8:])) if args.step.startswith("quality_") else step(args.step)))
    sys.exit(0)


def child(route):
    cmd = ["timeout", "-k", "10", "%d" % args.limit, sys.executable, os.path.abspath(__file__), "--step", route, "--triangles", str(args.triangles),
           "--res", str(args.res), "--inner", str(args.inner)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("route %s: exit status %d -- stopping here" % (route, r.returncode))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def finish(doc, ok, why):
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    if not ok:
        raise SystemExit(why)


if args.quality:
    doc = {"triangles": args.triangles, "res": args.res, "inner": args.inner, "deformations": [child("quality_0.01"), child("quality_0.1")]}
    for d in doc["deformations"]:
        for k in ("plain_ms", "shadows100_ms"):
            d[k[:-3] + "_refit_over_rebuilt"] = round(d["refit"][k] / d["rebuilt"][k], 3)
    finish(doc, all(d["same_frames"] for d in doc["deformations"]), "a refit tree's frame differs from the rebuilt tree's")
    sys.exit(0)

runs = {r: [] for r in ROUTES}
for rep in range(args.reps):
    for route in ROUTES:
        t0 = time.perf_counter()
        runs[route].append(child(route))
        print("round %d %s: %.1f s" % (rep, route, time.perf_counter() - t0), flush=True)
doc = {"triangles": args.triangles, "res": args.res, "reps": args.reps, "inner": args.inner, "routes": {}}
keys = ("set_ms", "build_ms", "frame_ms", "update_ms", "k_tri_records_ms", "k_tri_bounds_ms", "k_refit_leaves_ms", "k_refit_nodes_ms")
for route in ROUTES:
    per_child = {k: [median([u[k] for u in run["updates"]]) for run in runs[route]] for k in keys}
    doc["routes"][route] = {k: {"median": round(median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)} for k, v in per_child.items()}
crcs = {route: [u["crc"] for u in runs[route][0]["updates"]] for route in ROUTES}
doc["same_frames"] = crcs["host"] == crcs["device"] == crcs["device_keep"] == crcs["device_refit"]
h, d, r = doc["routes"]["host"], doc["routes"]["device"], doc["routes"]["device_refit"]
doc["refit_over_set_and_build"] = round((d["set_ms"]["median"] + d["build_ms"]["median"]) / r["set_ms"]["median"], 2) if r["set_ms"]["median"] > 0 else None
doc["set_speedup"] = round(h["set_ms"]["median"] / d["set_ms"]["median"], 2) if d["set_ms"]["median"] > 0 else None
doc["update_speedup"] = round(h["update_ms"]["median"] / d["update_ms"]["median"], 2) if d["update_ms"]["median"] > 0 else None
finish(doc, doc["same_frames"], "the routes' frames differ")
