"""Frame time of the path-traced 1 M-triangle 4096^2 frame (shading on, one sample per pixel, SR_MODE_BVH) next to the plain shaded
frame and the one-bounce mirror frame of the same scene: device frames (sr_render_device into a torch tensor, no host copy), three
variants alternating inside one process, device events around each frame, median and spread over the repetitions.

    python scripts/gpu_pathtrace.py                 # the three frame times + the library's own per-stage event times
    python scripts/gpu_pathtrace.py --profile       # few frames, for a `rocprofv3 --kernel-trace --stats -- python ...` run
    python scripts/gpu_pathtrace.py --parts 8       # + the path-traced frame through a multi-device scene over device 0 eight times:
                                                    #   the split's overhead on one card (not a speed-up), the first part's stage times
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import softray_amd as sa
from helpers import make_frame

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=4096)
ap.add_argument("--triangles", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--profile", action="store_true")
ap.add_argument("--parts", type=int, default=0, help="N > 0: also a multi-device scene over device 0 N times")
ap.add_argument("--out", default=None)
args = ap.parse_args()

g = sa.GpuScene(0)
g.set_triangles(*sa.unit_cube_scene(args.triangles))
g.build((sa.MODE_BVH,))
res = args.res


def frame(**kw):
    f = sa.Frame.from_buffer_copy(bytes(make_frame(res, depth=1.5, mode=sa.MODE_BVH)))
    for k, v in kw.items():
        setattr(f, k, v)
    return f


plain = frame()
path = frame()
path.flags |= sa.F_PATH_TRACING
bounce = frame(max_bounces=1, reflectivity=0.5)
variants = [("plain", g, plain), ("path_tracing", g, path), ("one_bounce", g, bounce)]
multi = None
if args.parts > 0:
    multi = sa.GpuScene(devices=[0] * args.parts)
    multi.set_triangles(*sa.unit_cube_scene(args.triangles))
    multi.build((sa.MODE_BVH,))
    variants.append(("path_tracing_%d_parts" % args.parts, multi, path))
surface = torch.zeros(res * res, dtype=torch.int32, device="cuda:0")
stream = torch.cuda.current_stream().cuda_stream
reps = 3 if args.profile else args.reps
for _ in range(2 if args.profile else 5):                               # warm-up: code objects, scratch, the random table, per-origin records
    for _, s, f in variants:
        s.render_device(f, surface.data_ptr(), stream)
torch.cuda.synchronize()
times = {n: [] for n, _, _ in variants}
for _ in range(reps):
    for n, s, f in variants:                                        # alternating: drift hits all alike
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        s.render_device(f, surface.data_ptr(), stream)
        b.record()
        b.synchronize()
        times[n].append(a.elapsed_time(b))
doc = {"res": res, "triangles": args.triangles, "reps": reps, "frames_ms": {}}
for n, _, _ in variants:
    t = np.array(times[n])
    doc["frames_ms"][n] = {"median": round(float(np.median(t)), 3), "min": round(float(t.min()), 3), "max": round(float(t.max()), 3)}
if not args.profile:
    # the library's own event pairs per stage (one frame each, one pipeline on one stream)
    # (a multi-device scene reports its first part: k_primary + k_pathtrace_count are that part's first phase, pathtrace_exchange its
    # counts out, the wait for the other parts and all counts back)
    doc["stages_ms"] = {}
    for n, s, f in variants:
        s.debug_set(sa._lib.DBG_KERNEL_TIMING, 1)
        f2 = sa.Frame.from_buffer_copy(bytes(f))
        f2.flags |= sa._lib.F_NO_SPLIT
        s.reset_kernel_times()
        s.render_device(f2, surface.data_ptr(), stream)
        torch.cuda.synchronize()
        doc["stages_ms"][n] = {k: round(v[0], 3) for k, v in s.kernel_times().items()}
    if multi is not None:
        doc["parts_last_frame"] = multi.last_frame_parts()
        single_px = None
        for s in (g, multi):                                            # the split frame is the frame
            surface.zero_()
            s.render_device(path, surface.data_ptr(), stream)
            torch.cuda.synchronize()
            px = surface.cpu().numpy()
            if single_px is None:
                single_px = px
        doc["parts_equal_single"] = bool(np.array_equal(single_px, px))
    px = surface.cpu().numpy().view(np.uint32)
    doc["checksum_last_frame"] = int(np.bitwise_xor.reduce(px))
print(json.dumps(doc), flush=True)
if args.out:
    with open(args.out, "w") as o:
        json.dump(doc, o, indent=1)
