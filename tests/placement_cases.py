"""Models away from the origin-centred unit cube (tests/test_placement_cases.py on the CPU oracle alone, tests/test_gpu_placement.py on
the device): one triangle soup mapped v' = v * aspect * scale + offset, with the root box mapped the same way unless the placement says
otherwise, a camera and lights that follow the placed model, and CPU-side predicates.  No library calls are made here.

The mapped coordinates are rounded, so every yardstick is the oracle run on the PLACED arrays; nothing is compared with the unplaced
frame.  What the placements move: the fp32 frame of reference of the fast path (everything fp32 is taken relative to the root box's
centre, which is zero in every other test), the absolute constants in the classification's error bounds (tuned for a unit box), the
size of the reference's FP64 noise (it works on absolute coordinates) and a root box that is not the vertex bounds."""
import math

import numpy as np

from helpers import c1_spheres, make_frame, orc, unit_cube_scene

BASE_N = 6000
OFFSET_LIMIT = 1.0e6                        # supported |box centre| / largest box extent (include/softray.h at sr_set_triangles)
SEED = 1234567890                           # make_frame's random_seed: the offset table is derived from it
# name: scale, aspect, offset, box rule (None = the mapped box, else (factor, shift): box = factor * [-0.5, 0.5]^3 + shift)
PLACEMENTS = {
    "origin":     dict(s=1.0, a=(1.0, 1.0, 1.0), c=(0.0, 0.0, 0.0)),                                  # the control
    "near":       dict(s=1.0, a=(1.0, 1.0, 1.0), c=(0.37, -0.21, 0.13)),                              # the centre is no fp32 number
    "far":        dict(s=1.0, a=(1.0, 1.0, 1.0), c=(1234.5678, -987.654321, 0.1), n=20000),
    "far_scaled": dict(s=37.7, a=(1.0, 1.0, 1.0), c=(10000.3, 3.3, -777.7)),
    "big":        dict(s=1024.0, a=(1.0, 1.0, 1.0), c=(0.0, 0.0, 0.0)),                               # the directional light's 1000-unit start is inside the model's reach
    "small":      dict(s=1.0 / 1024, a=(1.0, 1.0, 1.0), c=(0.001, 0.002, 0.0007)),                    # hit + 0.001 n leaves the box unless n is close to a diagonal
    "tiny":       dict(s=1.0 / 2048, a=(1.0, 1.0, 1.0), c=(0.001, 0.002, 0.0007)),                    # 0.001 / sqrt(3) > extent: no start is "inside"
    "flat":       dict(s=1.0, a=(1.0, 1.0, 0.03), c=(0.03, -0.02, 0.4)),                              # a slab, seen face-on (the camera looks along c)
    "loose":      dict(s=1.0, a=(1.0, 1.0, 1.0), c=(0.0, 0.0, 0.0), box=(3.0, 0.4)),                  # the geometry in one corner region of a larger, off-centre box
    "cut":        dict(s=1.0, a=(1.0, 1.0, 1.0), c=(0.0, 0.0, 0.0), box=(0.6, 0.0)),                  # triangles stick out of the box and cross its faces
    "far_probe":  dict(s=1.0, a=(1.0, 1.0, 1.0), c=(3.3, 0.7, -60000.1)),                             # |centre| / extent = 6e4 ("the offset limit")
    "far_limit":  dict(s=1.0, a=(1.0, 1.0, 1.0), c=(3.3, 0.7, -250000.1)),                            # a quarter of the documented limit of 1e6
}
EXTRA = ("tiny", "far_limit")                # soft-shadow frames only (tiny's penumbra is a few dozen pixels: the samples' crossings lie outside the box)
NAMES = tuple(n for n in PLACEMENTS if n not in EXTRA)
HAS_TREE = tuple(n for n in PLACEMENTS if n != "cut")            # the reference tree refuses a model with vertices outside the box
FP32_MUST_RUN = tuple(n for n in PLACEMENTS if PLACEMENTS[n]["s"] >= 1.0 and n != "cut")
BLUR_AT = ("near", "far", "small")
DEVICE_FED_AT = ("near", "far", "small", "cut")
SPHERES_AT = ("far", "big")
BIG_FRAME_AT = ("near", "far")


def placed(name, n=None):
    """(v9 [n, 3, 3], argb, box_min, box_max) of the placement: float64, as the library and the oracle get them."""
    p = PLACEMENTS[name]
    v9, argb, lo, hi = unit_cube_scene(p.get("n", BASE_N) if n is None else n)
    a, s, c = np.array(p["a"]), p["s"], np.array(p["c"])
    v = np.ascontiguousarray(np.asarray(v9, dtype=np.float64).reshape(-1, 3, 3) * a * s + c)
    if p.get("box") is None:
        blo, bhi = lo * a * s + c, hi * a * s + c
    else:
        factor, shift = p["box"]
        blo, bhi = lo * factor + shift, hi * factor + shift
    return v, argb, np.ascontiguousarray(blo), np.ascontiguousarray(bhi)


def placed_spheres(name, count=5):
    """c1_spheres mapped like the vertices (uniform placements only): centres * s + c, radii * s."""
    p = PLACEMENTS[name]
    assert p["a"] == (1.0, 1.0, 1.0)
    return [(kind, argb, [q[0] * p["s"] + p["c"][0], q[1] * p["s"] + p["c"][1], q[2] * p["s"] + p["c"][2], q[3] * p["s"]])
            for kind, argb, q in c1_spheres(count)]


def pose(name):
    """Camera of the placement.  The reference's camera orbits the model-space origin (its start is inverseTransform(3x3) * (0, 0,
    -positionZ), Renderer.cs:1717), not the model: with the origin seen in the direction of the offset and depth = |c| + 1.5 s the
    placed model sits at view (0, 0, 1.5 s), where every other test has it."""
    p = PLACEMENTS[name]
    c = np.array(p["c"])
    ln = float(np.sqrt((c * c).sum()))
    if ln == 0.0:
        return dict(yaw_deg=135.0, pitch_deg=-22.0, depth=1.5 * p["s"])
    cam = c / ln
    return dict(yaw_deg=math.degrees(math.atan2(-cam[0], -cam[2])), pitch_deg=math.degrees(math.asin(-cam[1])), depth=ln + 1.5 * p["s"])


def offset_table(name, samples, zero=False):
    """The area light's offsets at the placement's scale (the caller keeps the array alive while a frame points at it)."""
    t = orc.area_light_offsets(SEED, samples) * PLACEMENTS[name]["s"]
    return np.ascontiguousarray(t * 0.0 if zero else t)


def frame(name, w, h, table=None, light_model=None, **kw):
    """make_frame at the placement's pose, the point light's position scaled with the model; `table`: the offset table of a soft-shadow
    frame (offset_table); `light_model`: a model-space position of the point light, set through the frame's transform."""
    f = make_frame(w, h, **dict(pose(name), **kw))
    scale = PLACEMENTS[name]["s"]
    for i in range(3):
        f.light_pos_view[i] *= scale
    f.focal_depth, f.focal_blur_strength = 2.0 * scale, 10.0 * scale        # the model is 1.5 s from the camera: make_frame's depth + 0.5, in the model's units
    if light_model is not None:
        t = [f.transform[i] for i in range(12)]
        m = light_model
        for r in range(3):
            f.light_pos_view[r] = t[4 * r] * m[0] + t[4 * r + 1] * m[1] + t[4 * r + 2] * m[2] + t[4 * r + 3]
    if table is not None:
        f.area_light_offsets = table.ctypes.data
    return f


def light_inside(box_min, box_max):
    """A model-space light position inside the root box: centre + 0.1 x extent."""
    lo, hi = np.asarray(box_min), np.asarray(box_max)
    return 0.5 * (lo + hi) + 0.1 * (hi - lo)


# ---- predicates ----
def centre(box_min, box_max):
    return 0.5 * (np.asarray(box_min, dtype=np.float64) + np.asarray(box_max, dtype=np.float64))


def centre_is_no_fp32_number(box_min, box_max):
    c = centre(box_min, box_max)
    return bool((c.astype(np.float32).astype(np.float64) != c).any())


def offset_ratio(box_min, box_max):
    """|centre| / largest extent of the root box: what the supported-offset limit of include/softray.h is stated in."""
    c = centre(box_min, box_max)
    return float(np.sqrt((c * c).sum()) / (np.asarray(box_max) - np.asarray(box_min)).max())


def sticks_out(v9, box_min, box_max):
    """Per triangle: (a vertex outside the box, vertices on both sides of one of the box's face planes)."""
    p = np.asarray(v9).reshape(-1, 3, 3)
    out = ((p < box_min) | (p > box_max)).any(axis=(1, 2))
    crosses = (((p < box_min).any(axis=1) & (p > box_min).any(axis=1)) | ((p > box_max).any(axis=1) & (p < box_max).any(axis=1))).any(axis=1)
    return out, crosses


def outside_box(points, box_min, box_max, slack=1e-10):
    """Points the reference's containment test (AxisAlignedBox.cs:143-149, 1e-10 slack) puts outside the box."""
    q = np.asarray(points)
    return ((q < np.asarray(box_min) - slack) | (q > np.asarray(box_max) + slack)).any(axis=-1)
