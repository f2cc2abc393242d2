"""Which timing pairs a call opens, and how often: {kernel name: launches} of kernel_times() for every frame kind and every frame-based batch
call, once without and once with statistics, compared exactly with tests/golden/launch_counts.json.  The golden file was recorded by
collect() below on a build of the commit it names (the one before the launch layer of sr_pipeline.hip was restated through timed / launch /
with_flag / for_mode); it is a record of that build and is never regenerated from the code under test.  Frames are 64x48 (one is 72x40: its
width is no multiple of 16, so the tile-indexed queue's padded slot count differs from the pixel count) of the obj.3ds golden model, in
16-row bands (SR_DBG_BAND_SAMPLES) where the path allows bands; the batch calls run in two passes.  Launch counts under a hook that swaps
kernels are asserted where the hook was introduced (test_gpu_lightfield_tri.py, test_gpu_tight_boxes.py), not here."""
import json
import os

import numpy as np
import pytest

import ao_model as aom
import lightfield_bake as lfb
import lightfield_model as lfm
import lightfield_rays_model as lfr
import lightfield_shadow_model as lsm
import sequence_cases as sqc
import softray_amd as sa
from helpers import GOLDEN, camera_rays, make_frame

pytestmark = pytest.mark.gpu
L = sa._lib
W, H = 64, 48
SMALL = dict(res=(W, H), samples=33, hook=None)          # sequence_cases.SMALL at this file's size
GOLDEN_FILE = os.path.join(GOLDEN, "launch_counts.json")


def as_sr(frame, mode, extra_flags=0):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = mode
    f.flags |= extra_flags
    return f


def scene(modes):
    g = sa.GpuScene(0)
    g.load_3ds(open(os.path.join(GOLDEN, "obj.3ds"), "rb").read())
    g.build(modes)
    return g


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(name):
        if name not in made:
            made[name] = scene((sa.MODE_REF_TREE, sa.MODE_BVH) if name == "both" else (sa.MODE_REF_TREE,))
        return made[name]
    yield get
    for g in made.values():
        g.close()


def bands_of(f):
    """SR_DBG_BAND_SAMPLES for 16-row bands of the frame (the queue counts whole 16-pixel tiles across)."""
    return 16 * ((f.width + 15) // 16 * 16) * f.sub_pixel_res ** 2


# ---- the frames: name -> (scene, frame, trace mode, what to switch on in the scene) ----
def mirror_frame():
    f = make_frame(W, H)
    f.max_bounces, f.reflectivity = 2, 0.5
    return f


def path_frame():
    f = make_frame(W, H)
    f.flags |= L.F_PATH_TRACING
    return f


FRAMES = {
    "plain_tree": ("both", lambda: make_frame(W, H), sa.MODE_REF_TREE, {}),
    "plain_bvh": ("both", lambda: make_frame(W, H), sa.MODE_BVH, {}),
    "sub2_bvh": ("both", lambda: make_frame(W, H, sub_pixel_res=2), sa.MODE_BVH, {}),
    "shadows_bvh": ("both", lambda: sqc.frame(SMALL), sa.MODE_BVH, {}),
    "shadows_bvh_72x40": ("both", lambda: sqc.frame(SMALL, res=(72, 40)), sa.MODE_BVH, {}),
    "shadows_bvh_sub2": ("both", lambda: sqc.frame(SMALL, sub_pixel_res=2), sa.MODE_BVH, {}),
    "shadows_tree_on_bvh": ("both", lambda: sqc.frame(SMALL), sa.MODE_REF_TREE, {}),
    "shadows_tree": ("tree", lambda: sqc.frame(SMALL), sa.MODE_REF_TREE, {}),
    "shadows_130_samples": ("both", lambda: sqc.frame(SMALL, shadow_samples=130), sa.MODE_BVH, {}),
    "static_shadows": ("both", lambda: sqc.frame(SMALL, static_shadows=True), sa.MODE_BVH, dict(one_band=True)),
    "mirror_2": ("both", mirror_frame, sa.MODE_BVH, {}),
    "path_bvh": ("both", path_frame, sa.MODE_BVH, {}),
    "path_tree": ("both", path_frame, sa.MODE_REF_TREE, {}),
    "ao_cached": ("both", lambda: aom.ao_frame(make_frame(W, H)), sa.MODE_BVH, dict(one_band=True)),        # (a static or AO frame is one band)
    "ao_shadows": ("both", lambda: aom.ao_frame(sqc.frame(SMALL)), sa.MODE_BVH, dict(one_band=True)),
    "lf_plain": ("both", lambda: lfm.gpu_frame("view0_n8")[3], sa.MODE_BVH, {}),
    "lf_shadows": ("both", lambda: lsm.gpu_frame("view0_n8")[3], sa.MODE_BVH, dict(shadows=True)),
    "lf_interp": ("both", lambda: lfm.gpu_frame("view0_n8")[3], sa.MODE_BVH, dict(interp=True)),
    "lf_interp_shadows": ("both", lambda: lsm.gpu_frame("view0_n8")[3], sa.MODE_BVH, dict(interp=True, shadows=True)),
    "lf_triangles": ("both", lambda: lfm.gpu_frame("view0_n8")[3], sa.MODE_BVH, dict(tris=True)),
}
LF_RES = 8                                               # N of view0_n8


class Setup:
    """The scene's switches and caches for one measured call: set before, put back after."""

    def __init__(self, g, band=None, shadows=False, interp=False, tris=False, res=LF_RES):
        self.g, self.band, self.shadows, self.interp, self.tris, self.res = g, band, shadows, interp, tris, res

    def __enter__(self):
        g = self.g
        g.debug_set(L.DBG_KERNEL_TIMING, 1)
        if self.band:
            g.debug_set(L.DBG_BAND_SAMPLES, self.band)
        g.light_field_res = self.res
        g.light_field_shadows, g.light_field_interpolation, g.light_field_triangles = self.shadows, self.interp, self.tris
        return self

    def fresh(self):
        """What a new Renderer starts with: a call's launches may depend on what the caches hold."""
        g = self.g
        g.reset_light_field()
        g.reset_ao_cache()
        g.reset_shadow_cache()
        g.reset_kernel_times()

    def __exit__(self, *a):
        g = self.g
        g.light_field_shadows = g.light_field_interpolation = g.light_field_triangles = False
        g.debug_set(L.DBG_BAND_SAMPLES, -1)
        g.debug_set(L.DBG_KERNEL_TIMING, -1)


def launches(g):
    return {name: n for name, (_, n) in sorted(g.kernel_times().items())}


def collect_frame(scenes, name):
    which, make, mode, switches = FRAMES[name]
    g = scenes(which)
    f = as_sr(make(), mode)
    switches = dict(switches)
    band = None if switches.pop("one_band", False) else bands_of(f)
    out = {}
    with Setup(g, band=band, **switches) as s:
        for key, stats in (("warm_up", False), ("stats_off", False), ("stats_on", True)):      # (warm_up: what a scene does once, k_tight_boxes)
            s.fresh()
            g.render(f, stats=stats)
            out[key] = launches(g)
    del out["warm_up"]
    return out


# ---- the batch calls: a few hundred items in two passes ----
_POINTS = {}


def hit_points(g, count=600):
    """The first `count` hit points of the plain frame (made once per scene, outside the measured calls)."""
    if id(g) not in _POINTS:
        hits = g.render_hits(as_sr(make_frame(W, H), sa.MODE_REF_TREE))
        hit = hits["hit"].astype(bool)
        assert int(hit.sum()) >= count
        _POINTS[id(g)] = tuple(np.ascontiguousarray(hits[k][hit][:count]) for k in ("pos", "normal", "color"))
    return _POINTS[id(g)]


def quiet(stats):
    return 0 if stats else L.F_PRIMARY_STATS_ONLY


def call_render_hits(g, stats):
    g.render_hits(as_sr(make_frame(W, H, sub_pixel_res=2), sa.MODE_BVH), rays=True, stats=stats)


def call_trace_origin(g, stats):
    origin, dirs = camera_rays(make_frame(32, 24))
    g.trace_origin(sa.MODE_BVH, origin, dirs, stats=stats)


def call_trace_origin_tree(g, stats):
    origin, dirs = camera_rays(make_frame(32, 24))
    g.trace_origin(sa.MODE_REF_TREE, origin, dirs, stats=stats)


def lf_rays(count=600):
    _, f, starts, dirs = lfr.camera("view0_n8")
    return f, starts[:count].copy(), dirs[:count].copy()


def call_lf_rays(g, stats):
    f, starts, dirs = lf_rays()
    g.light_field_rays(as_sr(f, sa.MODE_BVH, quiet(stats)), starts, dirs)


def call_lf_rays_shadows(g, stats):
    f, starts, dirs = lf_rays()
    g.light_field_rays(as_sr(lsm.shadow_frame(f), sa.MODE_BVH, quiet(stats)), starts, dirs)


def call_shadow_points(g, stats):
    g.shadow_points(as_sr(sqc.frame(SMALL), sa.MODE_BVH, quiet(stats)), *hit_points(g))


def call_shadow_points_tree(g, stats):
    g.shadow_points(as_sr(sqc.frame(SMALL), sa.MODE_REF_TREE, quiet(stats)), *hit_points(g))


def call_static_shadow_points(g, stats):
    g.static_shadow_points(as_sr(sqc.frame(SMALL, static_shadows=True), sa.MODE_BVH, quiet(stats)), *hit_points(g))


def call_ao_points(g, stats):
    g.ao_points(as_sr(make_frame(W, H), sa.MODE_BVH, quiet(stats)), *hit_points(g))


def call_path_points(g, stats):
    g.path_points(as_sr(make_frame(W, H), sa.MODE_BVH, quiet(stats)), *hit_points(g))


def call_path_points_tree(g, stats):
    g.path_points(as_sr(make_frame(W, H), sa.MODE_REF_TREE, quiet(stats)), *hit_points(g))


def call_bake_shadows(g, stats):
    # N = 4: 32 cells per origin patch; four patches in passes of two
    g.bake_light_field(as_sr(lsm.shadow_frame(lfb.bake_frame(shadow_samples=33)), sa.MODE_BVH, quiet(stats)), first=0, count=128)


def call_bake(g, stats):
    g.bake_light_field(as_sr(lfb.bake_frame(), sa.MODE_BVH, quiet(stats)), first=0, count=128)


# name -> (scene, call, Setup keywords)
CALLS = {
    "render_hits": ("both", call_render_hits, dict(band=16 * W * 4)),
    "trace_origin": ("both", call_trace_origin, dict(band=512)),
    "trace_origin_tree": ("both", call_trace_origin_tree, dict(band=512)),
    "light_field_rays": ("both", call_lf_rays, dict(band=320)),
    "light_field_rays_shadows": ("both", call_lf_rays_shadows, dict(band=320, shadows=True)),
    "shadow_points": ("both", call_shadow_points, dict(band=320)),
    "shadow_points_tree": ("tree", call_shadow_points_tree, dict(band=320)),
    "static_shadow_points": ("both", call_static_shadow_points, dict(band=320)),
    "ao_points": ("both", call_ao_points, dict(band=320)),
    "path_points": ("both", call_path_points, dict(band=320)),
    "path_points_tree": ("both", call_path_points_tree, dict(band=320)),
    "bake_shadows": ("both", call_bake_shadows, dict(band=64, shadows=True, res=4)),
    "bake": ("both", call_bake, dict(band=64, res=4)),
}


def collect_call(scenes, name):
    which, call, kw = CALLS[name]
    g = scenes(which)
    hit_points(g)
    out = {}
    with Setup(g, **kw) as s:
        for key, stats in (("warm_up", False), ("stats_off", False), ("stats_on", True)):
            s.fresh()
            call(g, stats)
            out[key] = launches(g)
    del out["warm_up"]
    return out


def collect(scenes, name):
    return collect_frame(scenes, name) if name in FRAMES else collect_call(scenes, name)


CASES = list(FRAMES) + list(CALLS)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN_FILE))


@pytest.mark.parametrize("name", CASES)
def test_launch_counts(scenes, golden, name):
    got = collect(scenes, name)
    want = golden["cases"][name]
    print(name, json.dumps(got, sort_keys=True))
    assert any(got[key] for key in got), "no timing pair at all: the case measures nothing"
    assert got == want


def test_golden_names_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES) and len(golden["commit"]) == 40
