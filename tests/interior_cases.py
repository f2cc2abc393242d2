"""Scenes of the "interior triangle" shortcut of the shadow classification (tests/test_gpu_interior.py on the device,
tests/test_interior_cases.py on the CPU oracle alone): one triangle soup under different root boxes, and lights given in model space.

A candidate list whose triangles all lie inside the root box (shrunk by 1e-5 x its largest extent) lets the classification skip the
per-sample box exits; a triangle that touches or leaves the box must keep them, because the reference discards crossings outside the
root box (SpatialSubdivision.cs:394-401, 652)."""
import numpy as np

from helpers import make_frame, orc, random_triangles

SOUP_N = 6000
SAMPLES = 100
DELTA_REL = 1e-5                            # the library's margin: interior = inside the box shrunk by DELTA_REL x its largest extent
SMALL = 0.44                                # half size of the box smaller than the model: triangles up to 0.06 beyond every face
# model-space light positions (the camera of make_frame(depth=1.5) looks at the cube from (+x, +y, -z)-ish; both lights light faces it sees)
LIGHT_OUTSIDE = (0.35, 1.1, -0.55)          # beyond the band of triangles that sticks out of the small box's +y and -z faces
LIGHT_INSIDE = (0.05, 0.1, -0.02)


def soup(n=SOUP_N, seed=777):
    """Triangles with v1 in [-0.5, 0.45]^3 and extents U[0, 0.05]^3: inside [-0.5, 0.5]^3, never touching it."""
    v9, argb, _ = random_triangles(n, seed, space=0.95, extent=0.05, origin=-0.5, mask_color=True)
    return v9, argb


def tight_box(v9):
    """The exact vertex bounds: what a real model gives as its root box."""
    p = np.asarray(v9).reshape(-1, 3)
    return p.min(axis=0), p.max(axis=0)


def small_box():
    return np.array([-SMALL] * 3), np.array([SMALL] * 3)


def roomy_box():
    return np.array([-0.5] * 3), np.array([0.5] * 3)


def light_frame(res_w, res_h, light_model, mode=orc.MODE_REF_TREE, **kw):
    """A soft-shadow frame (SAMPLES samples, offsets derived from the frame's seed) whose point light sits at `light_model` (model space)."""
    f = make_frame(res_w, res_h, depth=1.5, shadows=True, shadow_samples=SAMPLES, mode=mode, **kw)
    t = [f.transform[i] for i in range(12)]
    m = light_model
    for r in range(3):
        f.light_pos_view[r] = t[4 * r] * m[0] + t[4 * r + 1] * m[1] + t[4 * r + 2] * m[2] + t[4 * r + 3]
    return f
