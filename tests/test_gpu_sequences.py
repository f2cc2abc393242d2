"""Frame sequences on one scene against the CPU oracle, bit for bit.  The library keeps records from one frame to the next -- the
facing partition (keyed on the camera origin, the light position and radius), the camera-cone records and the camera-ordered node
copy (camera origin), the light-ordered node copy (light position and radius), the persistent shaft walk's longest-first tile lists
(tile grid only: made by the previous frame, whatever its pose), the frame tables and the static shadow cache -- and a record that is
not re-made when it should be gives a plausible, wrong image.  Every step below changes one thing, names the record it targets and
asserts the precondition that makes it a reuse test; sr_debug_counters [5..7] show which ordered copies and tile orders a frame used.

    python tests/test_gpu_sequences.py 20 [first_seed] [big]      # a longer random-sequence soak by hand
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import softray_amd as sa  # noqa: E402
from helpers import (EDGE_GAPS, EDGE_RADII, EDGE_SIGNS, c1_spheres, edge_light_case, edge_light_frame, make_frame, orc,  # noqa: E402
                     random_triangles, unit_cube_scene)
from sequence_cases import L_IN, L_OUT, L_X, NCPU, PERSISTENT, SMALL, Pair, frame, model_origin_and_light, set_model_light  # noqa: E402, F401
from test_gpu_fuzz import big_case_of, case_of, frame_of  # noqa: E402

pytestmark = pytest.mark.gpu

def known_axes(p, radius, lo=-0.5, hi=0.5):
    """The axes on which a ball lies outside the unit cube's slab by more than the library's margin (point_outside_axes)."""
    m = 0.01 + 1e-3 * (hi - lo) + radius
    return sum(1 << a for a in range(3) if p[a] > hi + m or p[a] < lo - m)


def roll_keeping_origin_and_light(size, pose, light):
    """A roll that leaves the camera origin and the model-space light bit-identical (the light goes through the view transform and
    back, which need not round-trip exactly: search a few rolls)."""
    ref = model_origin_and_light(frame(size, pose, light))
    for roll in (45.0, 90.0, 30.0, 60.0, 15.0, 120.0, 10.0, 75.0):
        if model_origin_and_light(frame(size, (pose[0], pose[1], roll), light)) == ref:
            return roll
    raise AssertionError("no roll keeps the origin and the light bit-identical")


def depth_keeping_light(size, pose, light):
    """A camera distance that moves the camera origin but leaves the model-space light bit-identical (as above)."""
    ref = model_origin_and_light(frame(size, pose, light))
    for depth in (1.375, 1.25, 1.625, 1.125, 1.75, 1.3, 1.7, 1.4, 1.6, 1.8):
        o, l = model_origin_and_light(frame(size, pose, light, depth=depth))
        if o != ref[0] and l == ref[1]:
            return depth
    raise AssertionError("no camera distance keeps the light bit-identical")


def cube_pair(size, n=20000, **kw):
    v9, argb, lo, hi = unit_cube_scene(n)
    return Pair(v9, argb, lo, hi, hook=size["hook"], **kw)


def scripted_sequence(size):
    p = cube_pair(size)
    persistent = size["hook"] is not None
    seen = []                                                      # (label, counters) of every frame
    seen_frames = []

    def step(label, f, mode=sa.MODE_BVH, table=None, persistent_reuse=False):
        got, c = p.render(f, mode, table, label)
        seen.append((label, c))
        if persistent and persistent_reuse:        # the frame's tiles were walked in the order a frame with another pose / light made
            assert c[6] > 0 and c[7] > 0, (label, c)
        return got

    A = (135.0, -22.0, 0.0)
    B = (100.0, 15.0, 0.0)
    f0 = frame(size, A)
    first = step("first frame", f0)
    c0 = seen[-1][1]
    assert c0[5] == 0x77, c0                     # light outside on all axes (light-ordered copy: KNOWN 7), camera too (k_primary PKT 3)
    # 1. roll only: same origin and light -- partition, camera cones, both ordered copies are reused
    roll = roll_keeping_origin_and_light(size, A, L_OUT)
    f1 = frame(size, (A[0], A[1], roll))
    assert model_origin_and_light(f1) == model_origin_and_light(f0)
    step("roll only", f1, persistent_reuse=True)
    # 2. camera moves, light stays (camera cones, camera-ordered copy, partition re-made; light-ordered copy kept)
    depth = depth_keeping_light(size, A, L_OUT)
    f2 = frame(size, A, depth=depth)
    o2, l2 = model_origin_and_light(f2)
    assert o2 != model_origin_and_light(f0)[0] and l2 == model_origin_and_light(f0)[1]
    step("camera moves", f2, persistent_reuse=True)
    # ... the light moves, the camera stays: into the box (no known axis), out on x only, out on all axes (light-ordered copy, KNOWN)
    for name, light, known in (("light inside", L_IN, 0), ("light out on all axes", L_OUT, 7), ("light out on x", L_X, 1)):
        f = frame(size, A, light, depth=depth)
        assert model_origin_and_light(f)[0] == model_origin_and_light(f2)[0]
        step(name, f, persistent_reuse=True)
        seen_frames.append(f)
        assert seen[-1][1][5] & 7 == known, (name, seen[-1][1])
    # 3. only the light radius changes: a caller's offset table x0.5, x1.5 at the same position (partition and light-ordered copy keys)
    base_table = orc.area_light_offsets(1234567890, size["samples"])
    for scale in (0.5, 1.5):
        t = np.ascontiguousarray(base_table * scale)
        f = frame(size, A, L_X, depth=depth)
        assert model_origin_and_light(f) == model_origin_and_light(seen_frames[-1])
        step("radius x%g" % scale, f, table=t, persistent_reuse=True)
        assert seen[-1][1][5] & 7 == known_axes(L_X, scale * np.sqrt((base_table * base_table).sum(axis=1)).max()), seen[-1]
    # 4. shadows off / on; point light, directional, point (the partition's want_light / want_cam)
    step("shadows off", frame(size, B, L_X, shadows=False))
    step("shadows on", frame(size, B, L_X))
    step("directional", frame(size, B, L_X, point_light=False))
    step("point again", frame(size, B, L_X))
    # 5. a MODE_REF_TREE shadowed frame between MODE_BVH frames: its shadow rays take the BVH (shadows_on_bvh)
    step("ref tree", frame(size, A, L_X), mode=sa.MODE_REF_TREE)
    step("bvh after ref tree", frame(size, A, L_X))
    # 6. a new tile grid, a strip set, a row range, 2x2 sub-pixels (tile_order_tag, tile_n2), then the first grid again
    w, h = size["res"]
    step("resolution", frame(size, A, res=(w + 48, h - 16)))
    step("strips", frame(size, A, strips=(16, 4, 1)))
    step("row range", frame(size, A, start_row=h // 4, end_row=h - 9))
    step("sub-pixel 2", frame(size, A, sub_pixel_res=2, shadow_samples=max(5, size["samples"] // 4)))
    step("first grid again", frame(size, B, L_OUT), persistent_reuse=False)
    # 7. mirror bounces, then a shadowed frame
    fb = frame(size, A, shadows=False)
    fb.max_bounces, fb.reflectivity = 2, 0.5
    step("mirror bounces", fb)
    step("shadows after bounces", frame(size, A, L_X))
    # 8. geometry changes with the pose unchanged: extras on, off; another soup in the same box (nothing of the old tree may be reused)
    p.extra(c1_spheres(6))
    step("extras", frame(size, A))
    p.extra([])
    step("extras cleared", frame(size, A))
    v9, argb, lo, hi = unit_cube_scene(12000, seed=777)
    p.load(v9, argb, lo, hi)
    step("other soup", frame(size, A))
    v9, argb, lo, hi = unit_cube_scene(20000)
    p.load(v9, argb, lo, hi)
    # 9. static shadows over two poses without a reset, then after reset_shadow_cache (the oracle runs the same sequence)
    for label, pose in (("static A", A), ("static B", B), ("static A after reset", A)):
        if label.endswith("reset"):
            p.g.reset_shadow_cache()
            p.o.reset_shadow_cache()
        step(label, frame(size, pose, static_shadows=True))
    # 10. back to the first frame
    again = step("first frame again", frame(size, A))
    assert np.array_equal(again, first)
    return seen


@pytest.mark.parametrize("size", [SMALL, PERSISTENT], ids=["small", "persistent"])
def test_scripted_sequence_equals_oracle(size):
    seen = scripted_sequence(size)
    print("\n".join("%-24s %s" % (label, c[5:]) for label, c in seen))


@pytest.mark.parametrize("size", [SMALL, PERSISTENT], ids=["small", "persistent"])
def test_radius_change_without_the_facing_partition(size):
    """Hook 71 (no facing partition): its key is then not there to reset the light-ordered copy when only the radius changes."""
    p = cube_pair(size)
    p.g.debug_set(sa._lib.DBG_KERNEL_SWITCH, 71)
    table = orc.area_light_offsets(1234567890, size["samples"])
    pos = (0.5 + 0.011 + 0.15, 0.1, -0.05)                 # outside x by 0.161: known with radius <= 0.15, not with more
    radius = np.sqrt((table * table).sum(axis=1)).max()
    for scale in (0.5, 1.5, 0.5):
        t = np.ascontiguousarray(table * scale)
        f = frame(size, (60.0, -10.0, 0.0), pos)
        f.flags &= ~orc.F_SPECULAR
        _, c = p.render(f, table=t, label="hook 71, radius x%g" % scale)
        assert c[5] & 7 == known_axes(pos, radius * scale), (scale, c)


def test_production_grid_persistent_sequence():
    """No hook: a frame of 1024 x 800 crosses the default threshold of the persistent shaft walk; the second and third frames (other
    pose, other light) walk the tile order the frame before made."""
    size = dict(res=(1024, 800), samples=5, hook=None)
    p = cube_pair(size)
    f0 = frame(size, (135.0, -22.0, 0.0))
    first, c = p.render(f0, label="production first")
    assert c[6] > 0, c
    _, c = p.render(frame(size, (110.0, 10.0, 0.0)), label="production pose")
    assert c[6] > 0 and c[7] > 0, c
    again, c = p.render(frame(size, (135.0, -22.0, 0.0)), label="production first again")
    assert c[6] > 0 and c[7] > 0, c
    assert np.array_equal(again, first)


def test_persistent_frames_on_two_streams_against_the_oracle():
    """sr_render_device, persistent-size frames with other poses, lights and tables alternating between two streams with no host
    synchronisation, every one compared with the oracle (not with the GPU's own blocking render)."""
    import torch
    size = PERSISTENT
    p = cube_pair(size)
    table = np.ascontiguousarray(orc.area_light_offsets(1234567890, size["samples"]) * 1.5)
    frames = []
    for k, (pose, light) in enumerate((((135.0, -22.0, 0.0), L_OUT), ((100.0, 15.0, 0.0), L_OUT), ((100.0, 15.0, 0.0), L_IN),
                                       ((135.0, -22.0, 0.0), L_X), ((135.0, -22.0, 0.0), L_OUT), ((100.0, 15.0, 0.0), L_X))):
        f = frame(size, pose, light)
        if k == 3:
            f.area_light_offsets = table.ctypes.data
        frames.append((f, table if k == 3 else None))
    wants = [p.want(f, t) for f, t in frames]
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    outs = [torch.zeros(wants[k].size, dtype=torch.int32, device=dev) for k in range(len(frames))]
    for rep in range(2):
        for k, (f, _) in enumerate(frames):
            sf = sa.Frame.from_buffer_copy(bytes(f))
            sf.trace_mode = sa.MODE_BVH
            p.g.render_device(sf, outs[k].data_ptr(), streams[k % 2].cuda_stream)
    torch.cuda.synchronize(dev)
    for k in range(len(frames)):
        got = outs[k].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, wants[k]), "frame %d: %d pixels differ" % (k, int((got != wants[k]).sum()))


def test_sequence_on_two_parts_of_one_device():
    """GpuScene(devices=[0, 0]): every part keeps its own records."""
    size = SMALL
    p = cube_pair(size, devices=[0, 0])
    A, B = (135.0, -22.0, 0.0), (100.0, 15.0, 0.0)
    first, _ = p.render(frame(size, A), label="parts first")
    p.render(frame(size, B), label="parts camera")
    p.render(frame(size, B, L_IN), label="parts light inside")
    p.render(frame(size, B, L_X), table=np.ascontiguousarray(orc.area_light_offsets(1234567890, size["samples"]) * 1.5), label="parts radius")
    again, _ = p.render(frame(size, A), label="parts first again")
    assert np.array_equal(again, first)


# ---- seeded random sequences ----
def random_sequence(seed, big=False, steps=5):
    c = big_case_of(seed) if big else case_of(seed)
    if big:
        c["samples"] = int(np.random.RandomState(seed).choice([5, 7, 9]))
    v9, argb, _ = random_triangles(c["n"], c["seed"] + 1000, space=1.0 - c["extent"], extent=c["extent"], origin=-0.5, mask_color=True)
    p = Pair(v9, argb, np.array([-0.5] * 3), np.array([0.5] * 3), hook=831 if big else None)
    p.g.debug_set(sa._lib.DBG_BVH_LEAF, c["leaf"])
    p.load(v9, argb, np.array([-0.5] * 3), np.array([0.5] * 3))
    r = np.random.RandomState(seed + 5150)
    log = []
    for k in range(steps + 1):
        if k:
            what = r.choice(["pose", "roll", "light", "table", "samples", "flags", "surface", "mode", "extras"])
            if what == "pose":
                c.update(yaw=float(r.uniform(0, 360)), pitch=float(r.uniform(-60, 60)), depth=float(r.uniform(0.9, 1.7)))
            elif what == "roll":
                c["roll"] = float(r.uniform(-40, 40))
            elif what == "light":
                c.pop("light_view", None)
                c.update(light_scale=float(r.choice([0.15, 0.5, 1.0, 2.5])), light_turn=float(r.uniform(0, 2 * math.pi)))
            elif what == "table":
                c["table_scale"] = float(r.choice([0.0, 0.5, 1.5, 3.0]))
            elif what == "samples":
                c["samples"] = int(r.choice([5, 9]) if big else r.choice([1, 5, 33, 100]))
            elif what == "flags":
                flag = r.choice(["shadows", "point_light", "specular"])
                c[flag] = not c[flag]
                if c["shadows"]:
                    c["bounces"], c["spp"] = 0, 1
                    c["samples"] = c["samples"] or 5
            elif what == "surface":
                c["surface"] = r.choice(["res", "strips", "rows", "whole"])
                if c["surface"] == "res":
                    c["res"] = (c["res"][0] + 16 * int(r.randint(-2, 3)), c["res"][1] + 8 * int(r.randint(-2, 3)))
            elif what == "mode":
                c["mode"] = sa.MODE_REF_TREE if c.get("mode", sa.MODE_BVH) == sa.MODE_BVH else sa.MODE_BVH
            elif what == "extras":
                c["extras"] = 0 if c.get("extras") else int(r.randint(1, 6))
                p.extra(c1_spheres(c["extras"], seed=seed) if c["extras"] else [])
            log.append(what)
        f = frame_of(c)
        h = c["res"][1]
        if c.get("surface") == "strips":
            f.strip_rows, f.strip_count, f.strip_index = 16, 3, 1
        elif c.get("surface") == "rows":
            f.start_row, f.end_row = h // 5, h - 7
        table = None
        if "table_scale" in c and c["shadows"]:
            table = np.ascontiguousarray(orc.area_light_offsets(c["rng_seed"], c["samples"] or 100) * c["table_scale"])
        p.render(f, c.get("mode", sa.MODE_BVH), table, label="seed %d after %s: %r" % (seed, log, c))
    return log


@pytest.mark.parametrize("seed", [5, 7, 11, 19])
def test_random_sequence_equals_oracle(seed):
    random_sequence(seed)


@pytest.mark.parametrize("seed", [1, 2])
def test_random_persistent_sequence_equals_oracle(seed):
    random_sequence(seed, big=True, steps=4)


# ---- lights at the box edge with geometry beyond them ----
def edge_pair(size):
    v9, argb, lo, hi = unit_cube_scene(20000)
    return Pair(v9, argb, lo, hi, hook=size["hook"])


def run_edge_cases(size, cases, res):
    p = edge_pair(size)
    for signs, gap, radius in cases:
        c = edge_light_case(signs, gap, radius, samples=size["samples"])
        p.extra(c["prims"])
        for mode in (sa.MODE_BVH, sa.MODE_REF_TREE):
            f = edge_light_frame(c, *res)
            _, counters = p.render(f, mode, c["table"], label="light %r gap %g radius %g mode %d" % (signs, gap, radius, mode))
            mask = sum(1 << a for a in range(3) if signs[a])
            want_known = mask if radius == 0 else known_axes(c["light"], radius)
            assert counters[5] & 7 == want_known, (signs, gap, radius, mode, counters)


@pytest.mark.parametrize("signs", EDGE_SIGNS)
def test_edge_lights_small(signs):
    run_edge_cases(dict(samples=17, hook=None), [(signs, g, r) for g in EDGE_GAPS for r in EDGE_RADII], (96, 72))


def test_edge_lights_persistent():
    cases = [((1, 0, 0), 0.02, 0.2), ((-1, 1, 0), 0.1, 0.6), ((1, 1, -1), 0.02, 0.6), ((1, 1, -1), 0.02, 0.0)]
    run_edge_cases(dict(samples=5, hook=831), cases, (512, 384))


if __name__ == "__main__":
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    big = len(sys.argv) > 3 and sys.argv[3] == "big"
    for seed in range(first, first + count):
        print(seed, random_sequence(seed, big=big, steps=6), "ok", flush=True)
    print("all", count, "sequences equal")
