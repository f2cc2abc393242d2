"""sr_refit_triangles_device on the GPU: a scene whose device-built BVH was REFIT to moved vertices must answer as a scene that was
fed the new vertices through the host route and built from scratch ("fresh").  Pixels and ray outputs never depend on the tree, so
every comparison is an exact equality; the traversal statistics of a refit tree legitimately differ and are compared only where the
refit must reproduce the build's boxes bit for bit (identity, exact translation)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bvh_shape_cases as cases
import softray_amd as sa
import voxel_model as vm
from helpers import make_frame
from lightfield_model import F_LIGHT_FIELD

pytestmark = pytest.mark.gpu
L = sa._lib
DEV = torch.device("cuda", 0)
BOX = (np.array([-0.5] * 3), np.array([0.5] * 3))
W, H = 100, 60                                                           # partial 8x8 tiles on both axes
KEYS = ("hit", "ray_frac", "pos", "normal", "color", "tri_index")
GRID = 2.0 ** 20
BOXES_ONLY = [0, 1, 2, 3, 4, 6, 7]                                       # sr_last_ray_stats entries that the boxes alone decide (test 4)


def on_grid(v9):
    """Vertices rounded to multiples of 2^-20: translations by dyadic offsets are then exact."""
    return np.round(np.asarray(v9) * GRID) / GRID


def soup(n, seed=4711):
    v9, argb = sa.make_random_triangles(n, seed, space=0.95, extent=0.05, origin=-0.5, opaque=True)
    return on_grid(v9), argb


def as_sr(frame, mode=sa.MODE_BVH, extra_flags=0):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = mode
    f.flags |= extra_flags
    return f


def dev_v9(v9):
    return torch.from_numpy(np.ascontiguousarray(v9, dtype=np.float64).reshape(-1, 3, 3)).to(DEV)


def dev_argb(argb):
    return torch.from_numpy(np.ascontiguousarray(argb, dtype=np.uint32).view(np.int32)).to(DEV)


def built(v9, argb, box=BOX, leaf=None, modes=(sa.MODE_BVH,), **kw):
    """A host-fed scene with the own BVH built on the device: the "fresh" scene of every test, and the scene a refit starts from."""
    g = sa.GpuScene(**kw) if kw else sa.GpuScene(0)
    if leaf is not None:
        g.debug_set(L.DBG_BVH_LEAF, leaf)
    g.set_triangles(v9, argb, *box)
    g.build(modes, on_device=True)
    return g


def refit(g, v9, argb=None, box=BOX, **kw):
    g.refit_triangles_device(dev_v9(v9), None if argb is None else dev_argb(argb), *box, **kw)


def code_of(call):
    with pytest.raises(sa.SoftrayError) as e:
        call()
    return e.value.code


PLAIN = as_sr(make_frame(W, H, depth=1.6))
SHADOWS = as_sr(make_frame(W, H, shadows=True, depth=1.6))


def frames_equal(got, want, frames=(PLAIN, SHADOWS), tag=None):
    for k, f in enumerate(frames):
        a, b = got.render(f)[0], want.render(f)[0]
        assert np.array_equal(a, b), (tag, k, int(np.count_nonzero(a != b)))
        assert np.count_nonzero(b != b[0]) > 0.002 * b.size, (tag, k)      # (the soup shows in the frame)


def ray_batch(v9, count=1500, seed=99):
    """`count` random rays plus three rays aimed at every triangle: each starts outside the box, on the triangle's front side (the
    reference's triangles are one-sided), and passes, half way, through the point with barycentrics (0.98, 0.01, 0.01) or one of its
    two rotations -- a box that is too small loses one of them."""
    u = sa.net_random_doubles(seed, 6 * count).reshape(count, 6)
    starts = 2.4 * u[:, :3] - 1.2
    starts[::3] = 0.98 * (u[::3, :3] - 0.5)                              # every third random ray starts INSIDE the box
    dirs = (1.2 * u[:, 3:] - 0.6) - starts
    v = np.asarray(v9).reshape(-1, 3, 3)
    aimed_s, aimed_d = [], []
    for r in range(3):
        w = np.roll(np.array([0.98, 0.01, 0.01]), r)
        target = w[0] * v[:, 0] + w[1] * v[:, 1] + w[2] * v[:, 2]
        un = sa.net_random_doubles(seed + 1 + r, 3 * len(v)).reshape(-1, 3) - 0.5
        un /= np.sqrt((un * un).sum(axis=1))[:, None]
        front = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])           # Triangle.cs: a ray hits only from the side the normal points to
        un = np.where(((un * front).sum(axis=1) < 0)[:, None], -un, un)
        s = target + 3.0 * un                                            # at distance 3 from a point of the unit box: outside it
        aimed_s.append(s)
        aimed_d.append(2.0 * (target - s))
    starts = np.concatenate([starts] + aimed_s)
    dirs = np.concatenate([dirs] + aimed_d)
    return np.ascontiguousarray(starts), np.ascontiguousarray(dirs), count


def rays_equal(got, want, v9, tag=None, brute=True):
    """SR_MODE_BVH batches of the refit scene against the fresh scene's, field for field, and against its own SR_MODE_BRUTE batches.

    The two MODES are not one arithmetic for a ray that starts outside the root box: SR_MODE_BVH has the reference tree's semantics
    (sr_trace.h bvh_intersect: the start is clipped to the root box, rayFrac = the fraction from the clipped start + the clipped
    length / |dir|), SR_MODE_BRUTE intersects from the start as given -- on a scene built from scratch as on a refit one.  So against
    brute force: `hit`, `tri_index`, `color` and `normal` (copied from the hit record) are equal for every ray; `ray_frac` and `pos`
    are equal bit for bit for the rays that start inside the box (no clip, offset 0.0).  For a clipped ray the two differ by the
    rounding of the clip: the clipped start s' = a + (b - a) f is a few ulp (< 1e-14 for coordinates below 4) off the exact ray, and
    the plane equation turns an offset e of the start into e / |n.d^| along the ray (n the unit normal, d^ the unit direction): a
    grazing hit amplifies it without bound.  Hence |pos - pos_brute| <= 1e-13 (1 + 1 / |n.d^|) and, in units of |dir|,
    |ray_frac - ray_frac_brute| <= 1e-13 (1 + 1 / (|n.d^| |dir|)) max(1, ray_frac) -- ten times the estimate; a lost triangle is
    another hit or none and fails `hit` / `tri_index`.  Seen on an MI355X: at most 0.6 % of either bound (2.9e-12 in `pos`, grazing)."""
    starts, dirs, first_aimed = ray_batch(v9)
    a = got.trace(sa.MODE_BVH, starts, dirs)
    c = want.trace(sa.MODE_BVH, starts, dirs)
    for key in KEYS:
        assert np.array_equal(a[key], c[key]), (tag, "fresh", key, int(np.count_nonzero(a[key] != c[key])))
    if not brute:
        return None, first_aimed
    b = got.trace(sa.MODE_BRUTE, starts, dirs)
    fb = want.trace(sa.MODE_BRUTE, starts, dirs)
    inner = np.all(np.abs(starts) < 0.5, axis=1)
    assert inner[:first_aimed].sum() >= 500 and not inner[first_aimed:].any()
    for key in KEYS:
        assert np.array_equal(b[key], fb[key]), (tag, "brute records", key)          # (the TriangleIndex-order records are the fresh scene's)
        if key in ("ray_frac", "pos"):
            assert np.array_equal(a[key][inner], b[key][inner]), (tag, "brute, starts inside", key)
            h = b["hit"] != 0
            dlen = np.sqrt((dirs[h] ** 2).sum(axis=1))
            cosine = np.abs((b["normal"][h] * dirs[h]).sum(axis=1)) / dlen
            if key == "pos":
                err, bound = np.abs(a[key][h] - b[key][h]).max(axis=1), 1e-13 * (1.0 + 1.0 / cosine)
            else:
                err, bound = np.abs(a[key][h] - b[key][h]), 1e-13 * (1.0 + 1.0 / (cosine * dlen)) * np.maximum(1.0, b[key][h])
            print(tag, key, "largest difference to brute force / its bound:", (err / bound).max(), "absolute:", err.max())
            assert np.all(err <= bound), (tag, "brute", key, (err / bound).max())
        else:
            assert np.array_equal(a[key], b[key]), (tag, "brute", key, int(np.count_nonzero(a[key] != b[key])))
    return b, first_aimed


# ---- 1. counts and leaf sizes: refit to fresh random positions, the strongest deformation ----
@pytest.mark.parametrize("leaf", [1, None, 15], ids=["leaf1", "leaf_default", "leaf15"])
@pytest.mark.parametrize("n", [65, 255, 256, 257, 2000])
def test_counts_and_leaf_sizes(n, leaf):
    (v0, argb), (v1, _) = soup(n, 4711), soup(n, 1234)
    g = built(v0, argb, leaf=leaf)
    stats = (g.bvh_stats(), g.wide_tree_stats())
    assert stats[0][3] == 1
    refit(g, v1)
    assert (g.bvh_stats(), g.wide_tree_stats()) == stats
    fresh = built(v1, argb, leaf=leaf)
    brute, first_aimed = rays_equal(g, fresh, v1, (n, leaf))
    assert brute["hit"][first_aimed:].all()                               # every aimed ray hits something (its triangle or a nearer one)
    assert g.trace(sa.MODE_BVH, *ray_batch(v1)[:2])["hit"][first_aimed:].all()
    assert np.array_equal(g.get_triangles()[0], v1)


# ---- 2. warm per-origin state: the partition, the ordered copies, the cones, the penumbra planes, the interior bytes ----
def test_warm_per_origin_state_is_remade():
    (v0, argb), (v1, _) = soup(2000, 4711), soup(2000, 1234)
    v1 = on_grid(0.5 * (v0 + v1))
    g = built(v0, argb)
    frames_equal(g, built(v0, argb), tag="before")                        # (warms every per-origin / per-light record of g)
    refit(g, v1)
    frames_equal(g, built(v1, argb), tag="after")                         # same camera, same light: a stale record would be reused


# ---- 3. every schedule on a refit tree ----
def _sched(name, kw=None, flags=0, dbg=(), bounces=0):
    return pytest.param(kw or {}, flags, dbg, bounces, id=name)


@pytest.fixture(scope="module")
def refit_and_fresh():
    (v0, argb), (v1, _) = soup(2000, 4711), soup(2000, 77)
    v1 = on_grid(0.7 * v0 + 0.3 * v1)
    g = built(v0, argb)
    g.render(SHADOWS)
    refit(g, v1)
    return g, built(v1, argb)


@pytest.mark.parametrize("kw,flags,dbg,bounces", [
    _sched("plain", dict(shading=False)),
    _sched("shading"),
    _sched("shadows", dict(shadows=True)),
    _sched("per_lane_shadows", dict(shadows=True), flags=L.F_PER_LANE_SHADOWS),
    _sched("per_lane_shaft_1", dict(shadows=True), dbg=((L.DBG_PER_LANE_SHAFT, 1),)),
    _sched("per_lane_shaft_2", dict(shadows=True), dbg=((L.DBG_PER_LANE_SHAFT, 2),)),
    _sched("bvh2_packets", dict(shadows=True), dbg=((L.DBG_BVH2_PACKETS, 1),)),
    _sched("per_lane_primary", dict(shadows=True), dbg=((L.DBG_PER_LANE_PRIMARY, 1),)),
    _sched("focal_blur_sub2", dict(focal_blur=True, sub_pixel_res=2)),
    _sched("one_bounce", dict(shadows=True, shadow_samples=16), bounces=1),
    _sched("path_tracing", dict(shading=False), flags=L.F_PATH_TRACING),
    _sched("single_kernel", dict(shadows=True, shadow_samples=16), flags=L.F_SINGLE_KERNEL),
])
def test_every_schedule_on_a_refit_tree(refit_and_fresh, kw, flags, dbg, bounces):
    g, fresh = refit_and_fresh
    f = as_sr(make_frame(W, H, depth=1.6, **kw), sa.MODE_BVH, flags)
    if bounces:
        f.max_bounces, f.reflectivity = bounces, 0.5
    try:
        for s in (g, fresh):
            for key, value in dbg:
                s.debug_set(key, value)
        frames_equal(g, fresh, frames=(f,))
    finally:
        for s in (g, fresh):
            for key, _ in dbg:
                s.debug_set(key, -1)


# ---- 4. tightness: the refit boxes are the build's boxes, not merely conservative ones ----
def test_identity_and_exact_translation_reproduce_the_builds_boxes():
    """Identity: the same vertices and box -- sr_last_ray_stats[0..7] of the same frame are what they were before the refit.
    Translation by (0.25, -0.5, 0.125) of vertices and box together: exact on the 2^-20 grid, so every coordinate relative to the
    root centre, every pad, every Morton key and every rounding is that of the build.  The camera cannot follow an x / y translation
    (a frame's rays start at R^-1 (0, 0, -position.z)), so "before" for the translated scene is a scene BUILT at the translated
    vertices: its tree is the refit scene's tree node for node, and the statistics of the same frame must agree exactly.
    One of the eight counters does not depend on the boxes alone: [5], the triangle tests of the shadow rays, stops at a leaf's first
    occluder, so it depends on the ORDER of the records inside a leaf, which the facing partition permutes (by swaps) for every new
    (camera, light, geometry) -- with or without a refit.  The identity refit right after a frame leaves that order alone and must
    reproduce all eight; once the geometry has been elsewhere the order is another one, and the seven counters that the boxes
    decide -- rays, node and leaf visits, and the primary rays' tests (every live record of a visited leaf) -- must agree."""
    v0, argb = soup(2000)
    g = built(v0, argb)

    def stats(s):
        s.render(SHADOWS, stats=True)
        return s.ray_stats()[:8].copy()
    before = stats(g)
    assert before[0] > 0 and before[2] > 0 and before[4] > 0 and before[6] > 0      # primary and secondary rays, primary and secondary nodes
    refit(g, v0)
    assert np.array_equal(stats(g), before)                              # all eight: the boxes AND the records' places are the build's
    t = np.array([0.25, -0.5, 0.125])
    v1, box1 = v0 + t, (BOX[0] + t, BOX[1] + t)
    assert np.array_equal(v1 - t, v0)
    refit(g, v1, box=box1)
    fresh = built(v1, argb, box=box1)
    frames_equal(g, fresh)
    assert np.array_equal(stats(g)[BOXES_ONLY], stats(fresh)[BOXES_ONLY])
    refit(g, v0)                                                          # ... and back: the very numbers of the build
    assert np.array_equal(stats(g)[BOXES_ONLY], before[BOXES_ONLY])


# ---- 5. degenerate and out-of-box input ----
def degenerate(v9):
    """A tenth of the triangles collapsed: to a point, and to needles whose normal's only component lies just below / just above the
    1e-10 of the reference's zero-normal test."""
    v = v9.copy()
    h = (0.99e-10, 1.01e-10)
    for j, i in enumerate(range(0, len(v), 10)):
        if j % 3 == 0:
            v[i, 1] = v[i, 2] = v[i, 0]
        else:
            v[i, 1] = v[i, 0] + np.array([0.25, 0.0, 0.0])
            v[i, 2] = v[i, 0] + np.array([0.0, 4 * h[j % 3 - 1], 0.0])
    return v


def test_degenerate_triangles_and_a_box_smaller_than_the_vertex_bounds():
    v0, argb = soup(2000)
    v1 = degenerate(soup(2000, 31)[0])
    g = built(v0, argb)
    g.render(SHADOWS)
    refit(g, v1)
    fresh = built(v1, argb)
    rays_equal(g, fresh, v1, "degenerate", brute=False)                   # (needles reach out of the box: brute force sees more than any tree)
    frames_equal(g, fresh, tag="degenerate")
    small = (np.array([-0.3, -0.25, -0.35]), np.array([0.3, 0.35, 0.25]))
    v2 = soup(2000, 32)[0]
    refit(g, v2, box=small)
    fresh = built(v2, argb, box=small)
    rays_equal(g, fresh, v2, "small box", brute=False)
    frames_equal(g, fresh, tag="small box")
    assert np.array_equal(g.get_triangles()[2], small[0]) and np.array_equal(g.get_triangles()[3], small[1])


# ---- 6. a sequence ----
def test_five_refits_in_a_row_then_a_build():
    v, argb = soup(2000)
    g = built(v, argb)
    stats = (g.bvh_stats(), g.wide_tree_stats())
    rnd = np.random.RandomState(11)
    for k in range(5):
        v = np.clip(v + rnd.uniform(-0.03, 0.03, size=(len(v), 1, 3)) + rnd.uniform(-0.01, 0.01, size=v.shape), -0.5, 0.5)
        refit(g, v)
        assert (g.bvh_stats(), g.wide_tree_stats()) == stats, k           # same depth, nodes, slots, leaves; links intact
        frames_equal(g, built(v, argb), tag=k)
    last = [g.render(f)[0].copy() for f in (PLAIN, SHADOWS)]
    g.build((sa.MODE_BVH,), on_device=True)
    assert all(np.array_equal(a, g.render(f)[0]) for a, f in zip(last, (PLAIN, SHADOWS)))


# ---- 7. what is dropped and what is kept ----
def test_colours_are_kept_or_replaced():
    (v0, argb), (v1, _) = soup(300), soup(300, 5)
    g = built(v0, argb)
    refit(g, v1)
    assert np.array_equal(g.get_triangles()[1], argb)
    frames_equal(g, built(v1, argb), tag="kept")
    argb2 = argb[::-1].copy()
    refit(g, v0, argb2)
    got = g.get_triangles()
    assert np.array_equal(got[1], argb2) and np.array_equal(got[0], v0)
    frames_equal(g, built(v0, argb2), tag="replaced")


def cache_frames(g):
    """A voxel frame, a static-shadow frame and a light-field frame: each fills (and would reuse) a cache that belongs to the model."""
    out = [g.render(as_sr(make_frame(48, 32, depth=2.0), sa.MODE_BVH, vm.F_VOXELS))[0],
           g.render(as_sr(make_frame(48, 32, shadows=True, static_shadows=True, depth=1.6), sa.MODE_BVH))[0],
           g.render(as_sr(make_frame(48, 32, depth=1.6), sa.MODE_BVH, F_LIGHT_FIELD))[0]]
    return [o.copy() for o in out]


def test_caches_and_the_reference_tree_are_dropped():
    v0, argb = soup(2000)
    v1 = on_grid(np.clip(v0 + np.random.RandomState(5).uniform(-0.05, 0.05, size=(len(v0), 1, 3)), -0.5, 0.5))
    both = (sa.MODE_BVH, sa.MODE_REF_TREE)
    g = sa.GpuScene(0)
    g.light_field_res = 8
    g.set_triangles(v0, argb, *BOX)
    g.build(both, on_device=True)
    before = cache_frames(g)                                              # fills the voxel grid, the static-shadow cache, the light field
    g.render(as_sr(SHADOWS, sa.MODE_REF_TREE))
    refit(g, v1)
    fresh = sa.GpuScene(0)
    fresh.light_field_res = 8
    fresh.set_triangles(v1, argb, *BOX)
    fresh.build(both, on_device=True)
    after, want = cache_frames(g), cache_frames(fresh)
    assert all(np.array_equal(a, b) for a, b in zip(after, want))
    assert all(not np.array_equal(a, b) for a, b in zip(after, before))   # (the moved model shows in all three: a kept cache would not pass)
    assert code_of(lambda: g.render(as_sr(SHADOWS, sa.MODE_REF_TREE))) == L.SR_ERR_NOT_BUILT
    assert code_of(g.tree_stats) == L.SR_ERR_NOT_BUILT
    frames_equal(g, fresh, tag="bvh after the refusal")
    g.build((sa.MODE_REF_TREE,))
    assert g.tree_stats() == fresh.tree_stats()
    ref = (as_sr(PLAIN, sa.MODE_REF_TREE), as_sr(SHADOWS, sa.MODE_REF_TREE))   # (its shadow rays are answered on the refit BVH)
    frames_equal(g, fresh, frames=ref, tag="ref tree")
    frames_equal(g, fresh, tag="bvh after the ref build")


# ---- 8. refusals with a device: each leaves frames as they were ----
def test_refusals_leave_the_scene_as_it_was():
    v0, argb = soup(300)
    v1 = soup(300, 5)[0]
    brute = (as_sr(PLAIN, sa.MODE_BRUTE), as_sr(SHADOWS, sa.MODE_BRUTE))
    want = built(v0, argb)
    # no own BVH: never built / dropped by a device set
    g = sa.GpuScene(0)
    g.set_triangles(v0, argb, *BOX)
    assert code_of(lambda: refit(g, v1)) == L.SR_ERR_NOT_BUILT
    frames_equal(g, want, frames=brute, tag="never built")
    g.build((sa.MODE_BVH,), on_device=True)
    g.set_triangles_device(dev_v9(v0), None, *BOX)
    assert code_of(lambda: refit(g, v1)) == L.SR_ERR_NOT_BUILT
    assert code_of(lambda: g.render(PLAIN)) == L.SR_ERR_NOT_BUILT
    frames_equal(g, want, frames=brute, tag="after a set")
    # a host-built tree: SR_BUILD_ON_HOST, and n = 64 (the device build is not used at all)
    g.build((sa.MODE_BVH,), on_device=False)
    digest = g.bvh_digest()
    assert code_of(lambda: refit(g, v1)) == L.SR_ERR_UNSUPPORTED
    assert g.bvh_digest() == digest
    frames_equal(g, want, tag="host built")
    small = sa.GpuScene(0)
    small.set_triangles(v0[:64], argb[:64], *BOX)
    small.build((sa.MODE_BVH,))
    assert small.bvh_stats()[3] == 0
    assert code_of(lambda: refit(small, v1[:64])) == L.SR_ERR_UNSUPPORTED
    small_want = sa.GpuScene(0)
    small_want.set_triangles(v0[:64], argb[:64], *BOX)
    small_want.build((sa.MODE_BVH,))
    frames_equal(small, small_want, frames=brute[:1] + (PLAIN,), tag="n = 64")
    # n differs from the model's count
    g.build((sa.MODE_BVH,), on_device=True)
    for m in (299, 301):
        big = np.concatenate([v1, v1[:1]])[:m]
        assert code_of(lambda: refit(g, big)) == L.SR_ERR_INVALID_ARG
    assert g.num_triangles() == 300
    frames_equal(g, want, tag="n mismatch")
    # no model at all
    none = sa.GpuScene(0)
    assert code_of(lambda: refit(none, v1)) == L.SR_ERR_INVALID_ARG       # (its count is 0)
    lib = L.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.sr_refit_triangles_device(none._h, C.c_void_p(dev_v9(v1).data_ptr()), None, 0, p(BOX[0]), p(BOX[1]), None) == L.SR_ERR_NO_MODEL


def test_refused_build_leaves_nothing_to_refit():
    v9, argb, bmin, bmax = cases.scene("limit")
    g = sa.GpuScene(0)
    g.set_triangles(v9, argb, bmin, bmax)
    g.build((sa.MODE_BVH,), on_device=True)
    f = as_sr(cases.frame("limit", "plain"), sa.MODE_BVH)
    want, want_brute = g.render(f)[0].copy(), g.render(as_sr(f, sa.MODE_BRUTE))[0].copy()
    refit(g, v9, box=(bmin, bmax))                                        # (the deepest accepted tree, depth 62, refits)
    assert g.bvh_stats()[0] == 62 and np.array_equal(g.render(f)[0], want)
    g.debug_set(L.DBG_BVH_LEAF, 1)
    assert code_of(lambda: g.build((sa.MODE_BVH,), on_device=True)) == L.SR_ERR_UNSUPPORTED
    assert code_of(lambda: refit(g, v9, box=(bmin, bmax))) == L.SR_ERR_NOT_BUILT
    assert np.array_equal(g.render(as_sr(f, sa.MODE_BRUTE))[0], want_brute)
    assert code_of(lambda: g.render(f)) == L.SR_ERR_NOT_BUILT


# ---- 9. stream ordering ----
def test_tensor_produced_on_another_stream_without_synchronisation():
    v0, argb = soup(2000)
    d_v9 = dev_v9(v0)
    g = built(v0, argb)
    g.render(SHADOWS)
    st = torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)
    big = torch.ones((4096, 4096), dtype=torch.float64, device=DEV)
    with torch.cuda.stream(st):
        for _ in range(3):
            big = big @ big * 1e-4                                        # keeps the stream busy ahead of the producer
        moved = d_v9 * 0.5 + 0.125                                        # the tensor the scene is fed, produced on `st`
        g.refit_triangles_device(moved, None, *BOX, stream=st)            # no synchronisation in between
    assert np.array_equal(g.get_triangles()[0], v0 * 0.5 + 0.125)
    frames_equal(g, built(v0 * 0.5 + 0.125, argb))


def test_frame_in_flight_keeps_the_old_geometry():
    v0, argb = soup(2000)
    new = v0 * 0.5
    g, old_scene, new_scene = built(v0, argb), built(v0, argb), built(new, argb)
    f = as_sr(make_frame(256, 192, shadows=True, sub_pixel_res=2, depth=1.6), sa.MODE_BVH)
    want_old, want_new = old_scene.render(f)[0].copy(), new_scene.render(f)[0].copy()
    assert not np.array_equal(want_old, want_new)
    d_new = dev_v9(new)
    out = torch.zeros(256 * 192, dtype=torch.int32, device=DEV)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)
    big = torch.ones((4096, 4096), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(s1):
        for _ in range(3):
            big = big @ big * 1e-4                                        # holds the frame back: it cannot have run when the refit is enqueued
    g.render_device(f, out.data_ptr(), s1.cuda_stream)
    g.refit_triangles_device(d_new, None, *BOX, stream=s2)                # at once, on another stream
    s1.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want_old)
    assert np.array_equal(g.render(f)[0], want_new)


# ---- 10. a multi-device scene ----
def test_multi_device_scene_listing_one_ordinal_twice():
    (v0, argb), (v1, _) = soup(2000), soup(2000, 5)
    v1 = on_grid(0.6 * v0 + 0.4 * v1)
    multi = built(v0, argb, devices=[0, 0])
    frames_equal(multi, built(v0, argb), tag="before")
    assert multi.last_frame_parts() == 2
    refit(multi, v1)
    frames_equal(multi, built(v1, argb), tag="after")
    assert multi.last_frame_parts() == 2
    got = multi.get_triangles()
    assert np.array_equal(got[0], v1) and np.array_equal(got[1], argb)
    multi.close()
