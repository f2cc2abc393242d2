"""Scenes, poses and frame shapes of the G-buffer tests (tests/test_gpu_gbuffer.py), shared with tests/test_gbuffer_model.py, which checks on
the CPU that the hit count of every non-degenerate case lies strictly between 10 % and 90 % of its samples.

Scenes: obj.3ds (152 triangles); unit_cube_scene(2000) with edge_light_case's extra geometry (a plane, a sphere and a box outside the root
box); 48 large random triangles in the unit cube (at most 64: the own BVH of such a model is built on the host).
Poses: "out" -- the camera lies outside the root box's slab on all three axes (the camera-ordered copy holds (near, far) planes); "in" --
inside it on at least one; "away" -- looking away from everything.
Shapes: 37x21 (tiles clipped in both directions, one partial workgroup row), 16x16, 1x1, 100x100 in the goldens' pose, rows 5..17 of 48x40,
48x40 whole (three row bands of 16 rows under SR_DBG_BAND_SAMPLES), sub_pixel_res 1..3 with and without focal blur."""
import numpy as np

from helpers import edge_light_case, load_obj3ds, make_frame, orc, random_triangles, unit_cube_scene

EDGE = edge_light_case((1, 0, -1), 0.1, 0.6)

POSES = {
    ("obj", "out"): dict(),                                                   # RendererTests' pose: yaw 135, pitch -22, depth 1
    ("obj", "in"): dict(yaw_deg=180.0, pitch_deg=-5.0, depth=1.2),
    ("obj", "away"): dict(position=(0.0, 0.0, -3.0)),                         # the model lies behind the camera: every ray leaves it behind
    ("cube", "out"): dict(yaw_deg=30.0, pitch_deg=-20.0, depth=2.4),
    ("cube", "in"): dict(yaw_deg=EDGE["yaw"], pitch_deg=EDGE["pitch"], depth=EDGE["depth"]),
    ("small", "out"): dict(depth=2.0),
}

# (scene, pose, width, height, (start_row, end_row) or None, sub_pixel_res, focal blur)
CASES = [
    ("obj", "out", 100, 100, None, 1, False),
    ("obj", "in", 37, 21, None, 1, False),
    ("obj", "in", 37, 21, None, 2, False),
    ("obj", "in", 37, 21, None, 2, True),
    ("obj", "out", 16, 16, None, 3, False),
    ("obj", "out", 16, 16, None, 3, True),
    ("obj", "out", 1, 1, None, 1, False),
    ("obj", "out", 1, 1, None, 2, True),
    ("obj", "out", 48, 40, (5, 17), 1, False),
    ("obj", "in", 48, 40, (5, 17), 2, True),
    ("obj", "out", 48, 40, None, 2, False),
    ("obj", "away", 16, 16, None, 2, False),
    ("cube", "in", 37, 21, None, 1, False),
    ("cube", "out", 37, 21, None, 2, False),
    ("cube", "in", 16, 16, None, 3, True),
    ("cube", "out", 48, 40, (5, 17), 1, False),
    ("cube", "out", 48, 40, None, 1, False),
    ("small", "out", 37, 21, None, 1, False),
    ("small", "out", 37, 21, None, 2, True),
]


def case_id(c):
    return "%s-%s-%dx%d%s-n%d%s" % (c[0], c[1], c[2], c[3], "" if c[4] is None else "-rows%d..%d" % c[4], c[5], "-blur" if c[6] else "")


def scene_data(name):
    """((v9, argb, bmin, bmax), extra primitives) of a scene."""
    if name == "obj":
        return load_obj3ds(), ()
    if name == "cube":
        return unit_cube_scene(2000), tuple(EDGE["prims"])
    v9, argb, _ = random_triangles(48, 777, space=0.6, extent=0.4, origin=-0.5, mask_color=True)
    return (v9, argb, np.array([-0.5] * 3), np.array([0.5] * 3)), ()


def frame_of(case, **kw):
    """The oracle frame of a case: shading on, no shadows unless asked for (make_frame's keywords)."""
    scene, pose, w, h, rows, n, blur = case
    args = dict(POSES[(scene, pose)], sub_pixel_res=n, focal_blur=blur)
    if rows is not None:
        args.update(start_row=rows[0], end_row=rows[1])
    args.update(kw)
    return make_frame(w, h, **args)


def oracle_scenes(name):
    """(the scene with its reference tree, the same without a tree: the root geometry of a SR_MODE_BRUTE frame)."""
    tris, prims = scene_data(name)
    out = []
    for tree in (True, False):
        o = orc.Scene()
        o.set_triangles(*tris)
        if prims:
            o.set_extra(list(prims))
        if tree:
            assert o.build_tree() == 0
        out.append(o)
    return out


def outside_axes(f, tris):
    """Bit a set: the frame's camera origin lies outside [bmin, bmax] on axis a."""
    import pathtrace_model as ptm
    o = ptm.camera_samples(f)[0][0]
    return sum(1 << a for a in range(3) if o[a] < tris[2][a] or o[a] > tris[3][a])
