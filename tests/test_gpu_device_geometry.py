"""sr_set_triangles_device on the GPU: a scene fed from DEVICE tensors must be the scene that sr_set_triangles makes from the same
arrays -- the yardstick of every test here is a fresh scene fed through the host route -- in its records (ray batches in every mode,
sr_get_triangles), its trees, its frames, its dropped caches, its stream ordering and on a multi-device scene.  Every comparison is an
exact equality."""
import os

import numpy as np
import pytest
import torch

import softray_amd as sa
import voxel_model as vm
from helpers import GOLDEN, load_obj3ds, make_frame, read_bmp_rgb
from lightfield_model import F_LIGHT_FIELD

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BOX = (np.array([-0.5] * 3), np.array([0.5] * 3))
WIDE = (np.array([-1.0] * 3), np.array([1.0] * 3))
MODES = (sa.MODE_BVH, sa.MODE_REF_TREE, sa.MODE_BRUTE)
KEYS = ("hit", "ray_frac", "pos", "normal", "color", "tri_index", "counters")


def as_sr(frame, mode, extra_flags=0):
    f = sa.Frame.from_buffer_copy(bytes(frame))
    f.trace_mode = mode
    f.flags |= extra_flags
    return f


def dev_arrays(v9, argb):
    """The arrays as device tensors: float64 [n, 3, 3] and int32 [n] (the colour's bits)."""
    return (torch.from_numpy(np.ascontiguousarray(v9, dtype=np.float64).reshape(-1, 3, 3)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(argb, dtype=np.uint32).view(np.int32)).to(DEV))


def host_scene(v9, argb, box, **kw):
    g = sa.GpuScene(**kw) if kw else sa.GpuScene(0)
    g.set_triangles(v9, argb, *box)
    return g


def device_scene(v9, argb, box, **kw):
    g = sa.GpuScene(**kw) if kw else sa.GpuScene(0)
    d_v9, d_argb = dev_arrays(v9, argb)
    g.set_triangles_device(d_v9, d_argb, *box)
    return g


def soup(n, seed=4711):
    """n seeded triangles inside the unit cube's box, the first ones replaced by the cases a record can get wrong (as many as n holds):
    a triangle with vertices OUTSIDE the caller's box (the vertex bounds differ from it), needles whose normal's only component is just
    below / just above the 1e-10 of the zero-normal test, two equal vertices, three exactly collinear vertices."""
    v9, argb = sa.make_random_triangles(n, seed, space=0.95, extent=0.05, origin=-0.5, opaque=True)
    h0, h1 = 0.99e-10, 1.01e-10
    special = [[[0.3, 0.2, 0.7], [0.8, 0.1, 0.6], [0.4, 0.75, 0.9]],
               [[0.0, 0.0, 0.1], [0.25, 0.0, 0.1], [0.0, 4 * h0, 0.1]],
               [[0.0, 0.0, 0.2], [0.25, 0.0, 0.2], [0.0, 4 * h1, 0.2]],
               [[0.125, -0.25, 0.375], [0.125, -0.25, 0.375], [0.25, -0.25, 0.375]],
               [[-0.25, -0.25, -0.25], [0.0, 0.0, 0.0], [0.25, 0.25, 0.25]]]
    k = min(n, len(special))
    v9[:k] = np.array(special[:k])
    return v9, argb


def rays(count=1500, seed=99):
    u = sa.net_random_doubles(seed, 6 * count).reshape(count, 6)
    starts = 2.4 * u[:, :3] - 1.2
    target = 1.2 * u[:, 3:] - 0.6
    return np.ascontiguousarray(starts), np.ascontiguousarray(target - starts)


def assert_same_batches(got, want, modes, tag):
    starts, dirs = rays()
    hits = 0
    for mode in modes:
        for target in (mode, sa.TARGET_ROOT | mode):
            a, b = got.trace(target, starts, dirs, counters=True), want.trace(target, starts, dirs, counters=True)
            for key in KEYS:
                assert np.array_equal(a[key], b[key]), (tag, target, key)
            hits += int(b["hit"].sum())
    return hits


# ---- 1. counts at the edges: records, bounds, trees ----
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 2000])
def test_counts_at_the_edges(n):
    v9, argb = soup(n)
    # (a) the caller's box as given: one triangle lies outside it.  The reference tree refuses such a model (a vertex outside the box,
    #     SR_ERR_OUT_OF_RANGE) on both routes alike; the own BVH and brute force take it
    got, want = device_scene(v9, argb, BOX), host_scene(v9, argb, BOX)
    for g in (got, want):
        with pytest.raises(sa.SoftrayError) as e:
            g.build((sa.MODE_REF_TREE,))
        assert e.value.code == sa._lib.SR_ERR_OUT_OF_RANGE
        g.build((sa.MODE_BVH,))
    assert got.bvh_stats() == want.bvh_stats() and got.bvh_stats()[3] == (1 if n > 64 else 0)
    assert got.wide_tree_stats() == want.wide_tree_stats()
    hits = assert_same_batches(got, want, (sa.MODE_BVH, sa.MODE_BRUTE), ("tight", n))
    for point_light in (False, True):                                   # (a directional light's frame reads the vertex bounds on the host)
        f = as_sr(make_frame(48, 32, shadows=True, depth=2.5, point_light=point_light), sa.MODE_BVH)
        assert np.array_equal(got.render(f)[0], want.render(f)[0]), point_light
    # (b) a box that holds every vertex: all three structures
    got, want = device_scene(v9, argb, WIDE), host_scene(v9, argb, WIDE)
    for g in (got, want):
        g.build(MODES[:2])
    assert got.tree_stats() == want.tree_stats()
    assert got.bvh_stats() == want.bvh_stats() and got.bvh_stats()[3] == (1 if n > 64 else 0)
    hits += assert_same_batches(got, want, MODES, ("wide", n))
    assert n < 255 or hits > 0                                          # (the batches of the larger soups are not all misses)
    r_v9, r_argb, r_min, r_max = got.get_triangles()
    assert np.array_equal(r_v9.view(np.uint64), v9.view(np.uint64)) and np.array_equal(r_argb, argb)
    assert np.array_equal(r_min, WIDE[0]) and np.array_equal(r_max, WIDE[1]) and got.num_triangles() == n
    assert_same_batches(got, want, MODES[:1], ("after get_triangles", n))   # reading the host copy back changes nothing on the device


def test_host_sah_build_of_a_device_fed_scene():
    """SR_BUILD_ON_HOST reads the host arrays: they are fetched from the device first."""
    v9, argb = soup(300)
    got, want = device_scene(v9, argb, BOX), host_scene(v9, argb, BOX)
    for g in (got, want):
        g.build((sa.MODE_BVH,), on_device=False)
    assert got.bvh_digest() == want.bvh_digest() and got.bvh_stats() == want.bvh_stats() and got.bvh_stats()[3] == 0
    assert_same_batches(got, want, (sa.MODE_BVH,), "host sah")


def test_empty_model_and_refusals_on_a_device_scene():
    g = sa.GpuScene(0)
    d_v9, d_argb = dev_arrays(*soup(10))
    bad = sa._lib.SR_ERR_INVALID_ARG
    L = sa._lib.lib()
    import ctypes as C
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda v, a, n, lo=BOX[0], hi=BOX[1]: L.sr_set_triangles_device(g._h, C.c_void_p(v) if v else None, C.c_void_p(a) if a else None, n,
                                                                          p(lo) if lo is not None else None, p(hi) if hi is not None else None, None)
    assert call(d_v9.data_ptr(), d_argb.data_ptr(), -1) == bad
    assert call(0, d_argb.data_ptr(), 10) == bad
    assert call(d_v9.data_ptr(), d_argb.data_ptr(), 10, lo=None) == bad and call(d_v9.data_ptr(), d_argb.data_ptr(), 10, hi=None) == bad
    assert call(d_v9.data_ptr(), d_argb.data_ptr(), 0x7fffff01) == bad
    assert call(d_v9.data_ptr(), 0, 10) == bad                          # keep-colours without a model
    assert g.num_triangles() == 0
    assert call(d_v9.data_ptr(), d_argb.data_ptr(), 10) == 0
    assert call(d_v9.data_ptr(), 0, 9) == bad and call(d_v9.data_ptr(), 0, 11) == bad and g.num_triangles() == 10
    assert call(d_v9.data_ptr(), 0, 10) == 0
    # what the Python layer refuses itself
    for v, a in ((d_v9.cpu(), d_argb), (d_v9.float(), d_argb), (d_v9.reshape(-1, 9), d_argb), (d_v9, d_argb.double()), (d_v9, d_argb[:5]),
                 (d_v9, d_argb.reshape(-1, 1)), (d_v9.permute(0, 2, 1), d_argb), (d_v9[::2], d_argb[:5])):
        with pytest.raises(ValueError):
            g.set_triangles_device(v, a, *BOX)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            g.set_triangles_device(d_v9.to("cuda:1"), d_argb.to("cuda:1"), *BOX)
    assert g.num_triangles() == 10
    # n == 0: a model without triangles, as sr_set_triangles leaves it
    g.set_triangles_device(d_v9[:0].contiguous(), d_argb[:0].contiguous(), *BOX)
    e = sa.GpuScene(0)
    e.set_triangles(np.zeros((0, 3, 3)), np.zeros(0, dtype=np.uint32), *BOX)
    assert g.num_triangles() == e.num_triangles() == 0
    f = as_sr(make_frame(16), sa.MODE_BRUTE)
    for s in (g, e):
        with pytest.raises(sa.SoftrayError) as err:
            s.render(f)
        assert err.value.code == sa._lib.SR_ERR_NO_MODEL


# ---- 2. frames ----
def golden_rgb(name):
    return read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", name + ".bmp"))


def test_goldens_of_obj3ds_set_from_device_tensors():
    v9, argb, bmin, bmax = load_obj3ds()
    assert len(argb) == 152
    g = device_scene(v9, argb, (bmin, bmax))
    g.build((sa.MODE_REF_TREE, sa.MODE_BVH))
    for name, kw in (("shading", dict()), ("shading_shadows", dict(shadows=True)), ("noShading_4xAA", dict(shading=False, sub_pixel_res=4))):
        for mode in (sa.MODE_REF_TREE, sa.MODE_BVH):
            got, _ = g.render(as_sr(make_frame(100, **kw), mode))
            assert int(np.count_nonzero((got.reshape(100, 100) & 0xFFFFFF) != golden_rgb(name))) == 0, (name, mode)
    got, _ = g.render(as_sr(make_frame(100, depth=4.0, shading=True), sa.MODE_BVH, vm.F_VOXELS))
    assert int(np.count_nonzero((got.reshape(100, 100) & 0xFFFFFF) != golden_rgb("voxels_shading"))) == 0


def test_soup_frames_in_every_mode():
    v9, argb = soup(2000)
    got, want = device_scene(v9, argb, WIDE), host_scene(v9, argb, WIDE)
    for g in (got, want):
        g.build(MODES[:2])
    for mode in MODES:
        for shadows in (False, True):
            f = as_sr(make_frame(96, 64, shadows=shadows, depth=1.6), mode)
            (a, sa_), (b, sb) = got.render(f), want.render(f)
            assert np.array_equal(a, b) and np.array_equal(sa_, sb), (mode, shadows)
            assert np.array_equal(got.ray_stats(), want.ray_stats()), (mode, shadows)
            assert np.count_nonzero(b != b[0]) > 0.02 * b.size                  # (the soup shows in the frame)


# ---- 3. animation: one scene, three vertex sets, caches dropped ----
def cache_frames(g):
    """A voxel frame, a static-shadow frame and a light-field frame: each fills (and would reuse) a cache that belongs to the model."""
    out = [g.render(as_sr(make_frame(48, 32, depth=2.0), sa.MODE_BVH, vm.F_VOXELS))[0],
           g.render(as_sr(make_frame(48, 32, shadows=True, static_shadows=True, depth=1.6), sa.MODE_BVH))[0],
           g.render(as_sr(make_frame(48, 32, depth=1.6), sa.MODE_BVH, F_LIGHT_FIELD))[0]]
    return [o.copy() for o in out]


def test_animation_keeps_colours_and_drops_caches():
    v9, argb = soup(2000)
    box = (np.array([-0.8] * 3), np.array([0.8] * 3))
    rnd = np.random.RandomState(5)
    steps = [v9, v9 + rnd.uniform(-0.05, 0.05, size=(len(v9), 1, 3)), v9 * 0.9 + rnd.uniform(-0.03, 0.03, size=(len(v9), 3, 3))]
    g = sa.GpuScene(0)
    g.light_field_res = 8
    frame = as_sr(make_frame(96, 64, shadows=True, depth=1.6), sa.MODE_BVH)
    before = None
    for k, v in enumerate(steps):
        d_v9, d_argb = dev_arrays(v, argb)
        g.set_triangles_device(d_v9, d_argb if k == 0 else None, *box)
        with pytest.raises(sa.SoftrayError) as e:
            g.render(frame)
        assert e.value.code == sa._lib.SR_ERR_NOT_BUILT
        g.build((sa.MODE_BVH,))
        fresh = host_scene(v, argb, box)
        fresh.light_field_res = 8
        fresh.build((sa.MODE_BVH,))
        assert np.array_equal(g.render(frame)[0], fresh.render(frame)[0]), k
        if k == 0:
            before = cache_frames(g)                                     # fills the voxel grid, the static-shadow cache, the light field
            assert all(np.array_equal(a, b) for a, b in zip(before, cache_frames(fresh)))
        if k == 1:
            after, want = cache_frames(g), cache_frames(fresh)
            assert all(np.array_equal(a, b) for a, b in zip(after, want))
            assert all(not np.array_equal(a, b) for a, b in zip(after, before))   # (the moved model shows in all three: a kept cache would not pass)
        assert np.array_equal(g.get_triangles()[1], argb)                # the colours stayed


# ---- 4. stream ordering ----
def test_tensor_produced_on_another_stream_without_synchronisation():
    v9, argb = soup(2000)
    d_v9, d_argb = dev_arrays(v9, argb)
    st = torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)
    big = torch.ones((4096, 4096), dtype=torch.float64, device=DEV)
    with torch.cuda.stream(st):
        for _ in range(3):
            big = big @ big * 1e-4                                        # keeps the stream busy ahead of the producer
        moved = d_v9 * 0.5 + 0.125                                        # the tensor the scene is fed, produced on `st`
        g = sa.GpuScene(0)
        g.set_triangles_device(moved, d_argb, *BOX, stream=st)            # no synchronisation in between
    want = host_scene(v9 * 0.5 + 0.125, argb, BOX)
    assert np.array_equal(g.get_triangles()[0], v9 * 0.5 + 0.125)
    for s in (g, want):
        s.build((sa.MODE_BVH,))
    f = as_sr(make_frame(96, 64, depth=1.6), sa.MODE_BVH)
    assert np.array_equal(g.render(f)[0], want.render(f)[0])


def test_frame_in_flight_keeps_the_old_geometry():
    v9, argb = soup(2000)
    new = v9 * 0.5
    old_scene, new_scene = host_scene(v9, argb, BOX), host_scene(new, argb, BOX)
    g = device_scene(v9, argb, BOX)
    for s in (g, old_scene, new_scene):
        s.build((sa.MODE_BVH,))
    f = as_sr(make_frame(256, 192, shadows=True, sub_pixel_res=2, depth=1.6), sa.MODE_BVH)
    want_old, want_new = old_scene.render(f)[0].copy(), new_scene.render(f)[0].copy()
    assert not np.array_equal(want_old, want_new)
    d_new, _ = dev_arrays(new, argb)
    out = torch.zeros(256 * 192, dtype=torch.int32, device=DEV)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)
    big = torch.ones((4096, 4096), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(s1):
        for _ in range(3):
            big = big @ big * 1e-4                                        # holds the frame back: it cannot have run when the set is enqueued
    g.render_device(f, out.data_ptr(), s1.cuda_stream)
    g.set_triangles_device(d_new, None, *BOX, stream=s2)                  # at once, on another stream
    s1.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want_old)
    g.build((sa.MODE_BVH,))
    assert np.array_equal(g.render(f)[0], want_new)


# ---- 5. a multi-device scene ----
def test_multi_device_scene_listing_one_ordinal_twice():
    v9, argb = soup(2000)
    single = host_scene(v9, argb, WIDE)
    multi = sa.GpuScene(devices=[0, 0])
    d_v9, d_argb = dev_arrays(v9, argb)
    multi.set_triangles_device(d_v9, d_argb, *WIDE)
    for modes in ((sa.MODE_BVH,), (sa.MODE_REF_TREE,)):
        single.build(modes); multi.build(modes)
    for mode in (sa.MODE_BVH, sa.MODE_REF_TREE, sa.MODE_BRUTE):
        f = as_sr(make_frame(96, 64, shadows=True, depth=1.6), mode)
        assert np.array_equal(multi.render(f)[0], single.render(f)[0]), mode
        assert multi.last_frame_parts() == 2
    moved = v9 * 0.75
    multi.set_triangles_device(dev_arrays(moved, argb)[0], None, *WIDE)   # keep-colours on every part
    multi.build((sa.MODE_BVH,))
    f = as_sr(make_frame(96, 64, shadows=True, depth=1.6), sa.MODE_BVH)
    assert np.array_equal(multi.render(f)[0], host_scene_built(moved, argb, WIDE).render(f)[0]) and multi.last_frame_parts() == 2
    got = multi.get_triangles()
    assert np.array_equal(got[0], moved) and np.array_equal(got[1], argb)
    multi.close()


def host_scene_built(v9, argb, box):
    g = host_scene(v9, argb, box)
    g.build((sa.MODE_BVH,))
    return g


# ---- 6. keep-colours right after a HOST set: the colours are on the host only until the model is uploaded ----
@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["single", "two_parts"])
def test_keep_colours_after_a_host_set_that_was_never_uploaded(devices):
    v9, argb = soup(300)
    moved = v9 * 0.75 + 0.0625
    g = sa.GpuScene(0) if devices is None else sa.GpuScene(devices=devices)
    g.set_triangles(v9, argb, *WIDE)                                      # no build, no frame: nothing is on the device yet
    g.set_triangles_device(dev_arrays(moved, argb)[0], None, *WIDE)
    g.build((sa.MODE_BVH,))
    got = g.get_triangles()
    assert np.array_equal(got[1], argb) and np.array_equal(got[0], moved)
    want = host_scene_built(moved, argb, WIDE)
    for mode in (sa.MODE_BVH, sa.MODE_BRUTE):
        f = as_sr(make_frame(96, 64, shadows=True, depth=1.6), mode)
        assert np.array_equal(g.render(f)[0], want.render(f)[0]), mode
        assert g.last_frame_parts() == (1 if devices is None else 2)
    # ... and over an EARLIER model's records: a host set of other colours, then keep-colours at once
    argb2 = argb[::-1].copy()
    g.set_triangles(v9, argb2, *WIDE)
    g.set_triangles_device(dev_arrays(moved, argb)[0], None, *WIDE)
    g.build((sa.MODE_BVH,))
    assert np.array_equal(g.get_triangles()[1], argb2)
    want = host_scene_built(moved, argb2, WIDE)
    f = as_sr(make_frame(96, 64, shadows=True, depth=1.6), sa.MODE_BVH)
    assert np.array_equal(g.render(f)[0], want.render(f)[0])
    g.close()
