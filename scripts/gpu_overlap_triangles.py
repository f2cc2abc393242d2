"""The triangles of the scene that cross a batch of triangles (sr_overlap_triangles_device) measured on the GPU, on the unit-cube scene of the
benchmark (1 M triangles, SR_MODE_BVH, device arrays, warm).

    python scripts/gpu_overlap_triangles.py [--out profiles/overlap_triangles/overlap_triangles.json] [--reps 10]

One child process with a time limit of its own.  Query sets, built on the host and not timed:
  a_moved     the scene's own triangles, each moved by 1 % of the box (about 1 M queries, in the scene's order: no spatial order)
  b_object    a sphere of radius 0.25 about the box centre, 100 k triangles in latitude rows (a connected surface inside the scene)
Per set, after a warm-up of every side, `reps` runs in which the sides alternate, every run timed with an event pair on its stream:
  count             the counting call (K = 0, count alone)
  k4                K = 4 with count, index and mask
  any               SR_OVERLAP_ANY
  count_coherent, count_input_order   the counting call with SR_POINTS_COHERENT and under hook 56: the sort against the promise
  near_candidates   the only candidate route without this call: sr_near_triangles_device from the query's centroid with max_dist = the largest
                    distance from the centroid to a vertex (a sphere that holds the query), K = 64 with count and index -- candidates, not
                    crossings: the caller would still have to test them
Once each, over the first 4096 queries: the per-record loop (hook 57) and SR_MODE_BRUTE.
Before any time is taken k4's count is compared with the counting call's, `any` with count > 0, every schedule (SR_POINTS_COHERENT, hook 56)
with the sorted call, and hook 57 and SR_MODE_BRUTE over the first 4096 queries with the walk's rows, bit for bit.  Per variant also pairs /
nodes / leaves per query.  Nothing passes or fails on a time.  Reads neither the reference nor the oracle."""
import argparse
import json
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--triangles", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["measure"], help="(internal) run the measurement in this process")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    import numpy as np
    t = np.array(xs, dtype=np.float64)
    return {"median": round(float(np.median(t)), 3), "min": round(float(t.min()), 3), "max": round(float(t.max()), 3), "n": int(t.size)}


def sphere(radius, rows, cols):
    """2 x rows x cols triangles of a latitude / longitude sphere about the origin, row by row."""
    import numpy as np
    th = np.linspace(0.0, np.pi, rows + 1)[:, None]
    ph = np.linspace(0.0, 2.0 * np.pi, cols + 1)[None, :]
    p = radius * np.stack([np.sin(th) * np.cos(ph), np.cos(th) * np.ones_like(ph), np.sin(th) * np.sin(ph)], axis=-1)
    a, b, c, d = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    return np.ascontiguousarray(np.stack([np.stack([a, b, c], axis=2), np.stack([b, d, c], axis=2)], axis=2).reshape(-1, 3, 3))


def measure():
    import numpy as np
    import torch
    import softray_amd as sa
    L = sa._lib
    dev = torch.device("cuda", 0)
    g = sa.GpuScene(0)
    v9, argb, bmin, bmax = sa.unit_cube_scene(args.triangles)
    g.set_triangles(v9, argb, bmin, bmax)
    g.build((sa.MODE_BVH,))
    extent = float((bmax - bmin).max())
    stream = torch.cuda.current_stream().cuda_stream
    scene = np.asarray(v9, dtype=np.float64).reshape(-1, 3, 3)
    sets = {"a_moved": torch.from_numpy(np.ascontiguousarray(scene + 0.01 * extent)).to(dev),
            "b_object": torch.from_numpy(sphere(0.25, 224, 224) + (bmin + bmax) * 0.5).to(dev)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    doc = {"triangles": args.triangles, "reps": args.reps, "extent": extent, "sets": {}}
    for name, q in sets.items():
        m = q.shape[0]
        cnt = torch.zeros(m, dtype=torch.int32, device=dev)
        idx = torch.zeros((m, 4), dtype=torch.int32, device=dev)
        msk = torch.zeros((m, 4), dtype=torch.uint8, device=dev)
        centroid = q.mean(dim=1).contiguous()
        reach = (q - centroid[:, None, :]).norm(dim=2).max(dim=1).values.contiguous()
        n_cnt = torch.zeros(m, dtype=torch.int32, device=dev)
        n_idx = torch.zeros((m, 64), dtype=torch.int32, device=dev)

        def overlap(k, mode=sa.MODE_BVH, coherent=False, any_hit=False, hook=-1, items=m, st=None):
            def run():
                if hook >= 0:
                    g.debug_set(L.DBG_KERNEL_SWITCH, hook)
                try:
                    g.overlap_triangles_device(mode, items, q.data_ptr(), k, cnt.data_ptr(), idx.data_ptr() if k else 0, msk.data_ptr() if k else 0,
                                               coherent=coherent, any_hit=any_hit, stream=stream, d_stats_ptr=None if st is None else st.data_ptr())
                finally:
                    if hook >= 0:
                        g.debug_set(L.DBG_KERNEL_SWITCH, -1)
            return run

        def near(st=None):
            def run():
                g.near_triangles_device(sa.MODE_BVH, m, centroid.data_ptr(), reach.data_ptr(), 64, n_cnt.data_ptr(), n_idx.data_ptr(), 0, 0, 0, stream=stream,
                                        d_stats_ptr=None if st is None else st.data_ptr())
            return run

        def got(items=m):
            torch.cuda.synchronize()
            return cnt[:items].clone(), idx.reshape(-1)[:items * 4].clone(), msk.reshape(-1)[:items * 4].clone()

        def equal(a, b):
            return bool(all(torch.equal(x, y) for x, y in zip(a, b)))

        entry = {"queries": int(m)}
        same = {}
        overlap(4)()
        r4 = got()
        entry["count_mean"] = float(r4[0].to(torch.float64).mean().item())
        entry["count_max"] = int(r4[0].max().item())
        entry["queries_with_any"] = int((r4[0] > 0).sum().item())
        hist = torch.bincount(torch.clamp(r4[0], max=16).to(torch.int64), minlength=17)
        entry["count_histogram_0_to_16_plus"] = [int(x) for x in hist.cpu().tolist()]
        overlap(0)()
        same["count_alone"] = bool(torch.equal(got()[0], r4[0]))
        overlap(0, any_hit=True)()
        same["any"] = bool(torch.equal(got()[0], (r4[0] > 0).to(torch.int32)))
        for label, fn in (("k4_coherent", overlap(4, coherent=True)), ("k4_input_order", overlap(4, hook=56))):
            idx.fill_(90)
            fn()
            same[label] = equal(got(), r4)
        loop_n = min(4096, m)
        head = tuple(x[:loop_n * w].clone() for x, w in zip(r4, (1, 4, 4)))
        idx.fill_(90)
        loop_ms = timed(overlap(4, hook=57, items=loop_n))
        same["k4_loop_4096"] = equal(got(loop_n), head)
        idx.fill_(90)
        brute_ms = timed(overlap(4, mode=sa.MODE_BRUTE, items=loop_n))
        same["k4_brute_4096"] = equal(got(loop_n), head)
        near()()
        torch.cuda.synchronize()
        entry["near_candidates_mean"] = float(n_cnt.to(torch.float64).mean().item())
        entry["near_candidates_over_64"] = int((n_cnt > 64).sum().item())
        entry["equal"] = same
        if not all(same.values()):
            doc["sets"][name] = entry
            doc["error"] = "outputs differ on " + name
            return doc                                                           # no time is quoted for outputs that differ
        variants = {"count": overlap(0), "k4": overlap(4), "any": overlap(0, any_hit=True), "count_coherent": overlap(0, coherent=True),
                    "count_input_order": overlap(0, hook=56), "near_candidates": near()}
        for fn in variants.values():                                             # warm-up of every side
            timed(fn)
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for v, fn in variants.items():
                times[v].append(timed(fn))
        entry["call_ms"] = {k: stats(v) for k, v in times.items()}
        entry["loop_4096_ms_once"] = round(loop_ms, 3)
        entry["brute_4096_ms_once"] = round(brute_ms, 3)
        entry["mqueries_per_s"] = {k: round(m / v["median"] / 1e3, 1) for k, v in entry["call_ms"].items()}
        per_query = {}
        for label, fn in (("count", lambda st: overlap(0, st=st)), ("k4", lambda st: overlap(4, st=st)), ("any", lambda st: overlap(0, any_hit=True, st=st)),
                          ("near_candidates", lambda st: near(st=st))):
            st = torch.zeros(24, dtype=torch.int64, device=dev)
            fn(st)()
            torch.cuda.synchronize()
            s = st.cpu().tolist()
            per_query[label] = {"pairs_tested": round(s[1] / m, 2), "nodes": round(s[2] / m, 2), "leaves": round(s[3] / m, 2)}
        entry["per_query"] = per_query
        g.debug_set(L.DBG_KERNEL_TIMING, 1)
        kernels = {}
        for label in ("count", "k4", "any"):
            g.reset_kernel_times()
            timed(variants[label])
            kernels[label] = {k: round(t[0], 3) for k, t in g.kernel_times().items()}
        entry["kernels_one_rep_ms"] = kernels
        g.debug_set(L.DBG_KERNEL_TIMING, -1)
        doc["sets"][name] = entry
        del cnt, idx, msk, centroid, reach, n_cnt, n_idx, r4
    return doc


if args.step:
    print("RESULT " + json.dumps(measure()))
    sys.exit(0)

cmd = [sys.executable, os.path.abspath(__file__), "--step", "measure", "--triangles", str(args.triangles), "--reps", str(args.reps)]
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
