"""The CPU model of the triangle-index light field (tests/lightfield_tri_model.py) pinned without a GPU: its two restatements against the oracle
and the library's host side (a three-way agreement), the input conditions of the frames tests/test_gpu_lightfield_tri.py renders, and the new
entry points' host behaviour."""
import ctypes as C
import os

import numpy as np
import pytest

import lightfield_model as lfm
import lightfield_tri_model as ltm
import pathtrace_model as ptm
import softray_amd as sa
from helpers import ROOT, load_obj3ds, orc, random_triangles, unit_cube_scene

KATS = [(10, 5, 3), (5, 3, 1), (8, 3, 1), (4, 100, 1), (1000, 10, 5)]          # tests/test_abi.py: seed 12345, box [0, 110]^3
SCENES = ["kat%d" % i for i in range(len(KATS))] + ["obj.3ds", "obj2.3DS"]


def scene_data(name):
    """(v9, argb, bmin, bmax, max_depth, max_per_leaf)"""
    if name.startswith("kat"):
        n, depth, per_leaf = KATS[int(name[3:])]
        v9, argb, _ = random_triangles(n, seed=12345)
        return v9, argb, np.zeros(3), np.full(3, 110.0), depth, per_leaf
    return load_obj3ds(name) + (15, 25)


# ---- (a) the triangle test against the oracle's brute-force trace on single-triangle scenes, bit for bit ----
def test_triangle_test_is_the_oracles():
    rng = np.random.default_rng(20240611)
    v9, argb, _ = random_triangles(40, seed=777, space=0.8, extent=0.3, origin=-0.5)
    rec = ltm.tri_records(v9)
    total = hits = 0
    for k in range(v9.shape[0]):
        tri = v9[k]
        o = orc.Scene()
        o.set_triangles(tri[None], argb[k:k + 1], [-1.0] * 3, [1.0] * 3)
        n = 300
        a, b = rng.random((n, 2)).T
        flip = a + b > 1
        a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
        target = tri[0] + a[:, None] * (tri[1] - tri[0]) + b[:, None] * (tri[2] - tri[0])
        target[n // 3:] += (rng.random((n - n // 3, 3)) - 0.5) * 0.4          # two thirds aim near the triangle, through its edges and past it
        starts = (rng.random((n, 3)) - 0.5) * 3.0
        side = (starts - tri[0]) @ rec[k, 0:3]                                 # one-sided triangles: most rays start in front of the plane
        front = (side < 0) & (rng.random(n) < 0.8)
        starts[front] -= 2.0 * side[front, None] * rec[k, 0:3]
        dirs = (target - starts) * rng.uniform(0.2, 3.0, n)[:, None]          # rayFrac on both sides of 1
        # grazing: directions almost in the triangle's plane; behind the start: the triangle lies the other way
        graze = slice(0, 30)
        inplane = (tri[1] - tri[0]) * rng.normal(size=(30, 1)) + (tri[2] - tri[0]) * rng.normal(size=(30, 1))
        dirs[graze] = inplane + rec[k, 0:3] * rng.normal(size=(30, 1)) * 1e-9
        dirs[30:60] = -dirs[30:60]
        want = o.trace(0, starts, dirs)
        ok, rf, pos = ltm.tri_hit(rec[k], starts, dirs)
        assert np.array_equal(ok, want["hit"].astype(bool))
        assert np.array_equal(rf.view(np.uint64), want["ray_frac"].view(np.uint64))
        assert np.array_equal(pos.view(np.uint64), want["pos"].view(np.uint64))
        assert np.array_equal(np.broadcast_to(rec[k, 0:3], (n, 3))[ok].view(np.uint64), want["normal"][ok].view(np.uint64))
        total += n
        hits += int(ok.sum())
    assert total >= 10000 and total // 10 < hits < total


# ---- (b), (c) the tree: counts against the oracle and the library, every handle leaf against sr_tree_handle_leaf on a host-only scene ----
@pytest.mark.parametrize("name", SCENES)
def test_tree_and_handle_leaves_three_way(name):
    v9, argb, bmin, bmax, depth, per_leaf = scene_data(name)
    tree = ltm.build_tree(v9, bmin, bmax, depth, per_leaf)
    o = orc.Scene()
    o.set_triangles(v9, argb, bmin, bmax)
    assert o.build_tree(depth, per_leaf) == 0
    s = sa.GpuScene(device=-1)
    s.set_triangles(v9, argb, bmin, bmax)
    s.build((sa.MODE_REF_TREE,), depth, per_leaf)
    assert tree.stats() == o.tree_stats() == s.tree_stats()
    n = np.asarray(v9).reshape(-1, 9).shape[0]
    assert (tree.handle >= 0).all()
    for t in range(n):
        box, members = s.tree_handle_leaf(t)
        want_box, want_members = ltm.handle_leaf(tree, t)
        assert np.array_equal(box.view(np.uint64), want_box.view(np.uint64)), t
        assert np.array_equal(members, want_members), t
        assert t in members.tolist()
    # the handle is the LAST leaf that lists the triangle: no later leaf holds it
    last = np.full(n, -1)
    for k, m in enumerate(tree.leaf_members):
        last[m] = k
    assert np.array_equal(last, tree.handle)


def test_handle_leaf_arguments():
    s = sa.GpuScene(device=-1)
    L = sa._lib.lib()
    box = np.zeros(6)
    p = box.ctypes.data_as(C.c_void_p)
    v9, argb, bmin, bmax = load_obj3ds()
    s.set_triangles(v9, argb, bmin, bmax)
    assert L.sr_tree_handle_leaf(s._h, 0, p, None, 0) == sa._lib.SR_ERR_NOT_BUILT
    s.build((sa.MODE_REF_TREE,))
    n = argb.size
    assert L.sr_tree_handle_leaf(s._h, 0, p, None, 0) > 0
    for tri in (-1, n):
        assert L.sr_tree_handle_leaf(s._h, tri, p, None, 0) == sa._lib.SR_ERR_INVALID_ARG
    assert L.sr_tree_handle_leaf(s._h, 0, None, None, 0) == sa._lib.SR_ERR_INVALID_ARG
    assert L.sr_tree_handle_leaf(s._h, 0, p, None, 4) == sa._lib.SR_ERR_INVALID_ARG
    few = np.full(3, -7, dtype=np.int32)                     # a short buffer gets the first members, the count is the leaf's
    full = s.tree_handle_leaf(0)[1]
    assert L.sr_tree_handle_leaf(s._h, 0, p, few.ctypes.data_as(C.c_void_p), 2) == full.size
    assert few.tolist() == full[:2].tolist() + [-7]
    s.set_triangles(v9, argb, bmin, bmax)                    # a new model: no tree
    assert L.sr_tree_handle_leaf(s._h, 0, p, None, 0) == sa._lib.SR_ERR_NOT_BUILT


# ---- the frames of the GPU test: input conditions and the census they must supply ----
@pytest.fixture(scope="module")
def census():
    """Every GPU_FRAMES_TRI frame on the model (reference tree), from an empty table: name -> (stats, stage-3 hits, stage-3 misses, margins)."""
    scenes, out = {}, {}
    for name in ltm.GPU_FRAMES_TRI:
        model, prims, n, f = lfm.gpu_frame(name)
        if model not in scenes:
            scenes[model] = ltm.oracle_scene(model)
        m = ltm.LightFieldTriModel(*scenes[model], n=n)
        m.sample_colors(f, ltm.TRACE_TREE)
        out[name] = (list(m.stats), m.stage3_hits, m.stage3_misses, m.coord_margin, m.term_margin)
    return out


@pytest.mark.parametrize("name", ltm.GPU_FRAMES_TRI)
def test_frame_input_conditions(census, name):
    stats, _, _, coord_margin, term_margin = census[name]
    assert coord_margin >= lfm.MARGIN and term_margin >= lfm.MARGIN
    assert stats[0] == sum(stats[20:24]) and stats[4] > 0


def test_frames_supply_every_stage(census):
    """A condition on the frame list, not a measurement: every stage resolves samples somewhere, and stage 3 both hits and misses."""
    total = np.sum([c[0] for c in census.values()], axis=0)
    assert total[20] > 0 and total[21] > 0 and total[22] > 0 and total[23] > 0
    assert sum(c[1] for c in census.values()) > 0 and sum(c[2] for c in census.values()) > 0


def test_frame_list_is_the_issues():
    assert all(name in lfm.GPU_FRAMES for name in ltm.GPU_FRAMES_TRI)
    res = {name: lfm.GPU_FRAMES[name][2] for name in ltm.GPU_FRAMES_TRI}
    assert res["contention"] == 4 and res["small_blur"] == 8 and res["far_n16"] == res["far_primitives"] == 16 and res["view0_n64"] == 64
    assert res["unit_cube"] == 32 and lfm.GPU_FRAMES["far_primitives"][1]


def test_extra_geometry_has_no_effect_on_the_model():
    """far_primitives carries extra geometry; the method never consults it: the model takes none, and the frame differs from far_n16 by its rows only."""
    a, b = lfm.gpu_frame("far_n16")[3], lfm.gpu_frame("far_primitives")[3]
    sc = ltm.oracle_scene("obj.3ds")
    whole = ltm.LightFieldTriModel(*sc, n=16).render(a)
    rows = ltm.LightFieldTriModel(*sc, n=16).render(b)
    assert np.array_equal(whole[b.start_row:b.end_row + 1], rows)


# ---- ABI: symbols, the setting, the host-only table ----
def test_symbols_and_versions():
    L = sa._lib.lib()
    for name in ("sr_set_light_field_triangles", "sr_get_light_field_triangles", "sr_get_light_field_tris", "sr_set_light_field_tris", "sr_tree_handle_leaf"):
        assert name in sa._lib.SYMBOLS and hasattr(L, name)
    assert L.sr_abi_version() == 5
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert "SR_DBG_COUNT          = 17" in header and "#define SR_STATS_COUNT 24" in header and "#define SR_ABI_VERSION 5" in header


def test_setting_validation_and_survival():
    s = sa.GpuScene(device=-1)
    L = sa._lib.lib()
    assert s.light_field_triangles is False
    for bad in (-1, 2, 7):
        assert L.sr_set_light_field_triangles(s._h, bad) == sa._lib.SR_ERR_INVALID_ARG
    assert L.sr_set_light_field_triangles(None, 1) == sa._lib.SR_ERR_INVALID_ARG
    assert s.light_field_triangles is False
    s.light_field_triangles = True
    assert s.light_field_triangles is True and L.sr_get_light_field_triangles(s._h) == 1
    s.set_triangles(*load_obj3ds())
    assert s.light_field_triangles is True
    s.load_3ds(open(os.path.join(ROOT, "tests", "golden", "obj2.3DS"), "rb").read())
    assert s.light_field_triangles is True
    s.light_field_triangles = False
    assert s.light_field_triangles is False


def test_host_only_table_round_trip_and_drops():
    s = sa.GpuScene(device=-1)
    s.light_field_res = 3
    total = lfm.cache_entries(3)
    assert s.get_light_field_tris().tolist() == [0] * total
    part = np.arange(5, 25, dtype=np.uint32)
    s.set_light_field_tris(part, first=7)
    want = np.zeros(total, dtype=np.uint32)
    want[7:27] = part
    assert np.array_equal(s.get_light_field_tris(), want)
    assert np.array_equal(s.get_light_field_tris(10, 4), want[10:14])
    assert not s.get_light_field().any()                     # the colour table is another table ...
    s.set_light_field(np.full(4, 9, dtype=np.uint32), first=1)
    assert np.array_equal(s.get_light_field_tris(), want)    # ... and neither touches the other
    L = sa._lib.lib()
    buf = np.zeros(4, dtype=np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    for fn in (L.sr_get_light_field_tris, L.sr_set_light_field_tris):
        assert fn(s._h, p, total - 3, 4) == sa._lib.SR_ERR_INVALID_ARG
        assert fn(s._h, None, 0, 4) == sa._lib.SR_ERR_INVALID_ARG
        assert fn(s._h, None, total, 0) == 0
    drops = [lambda: s.reset_light_field(), lambda: s.set_triangles(*load_obj3ds()), lambda: setattr(s, "light_field_res", 2),
             lambda: s.load_3ds(open(os.path.join(ROOT, "tests", "golden", "obj.3ds"), "rb").read())]
    for drop in drops:
        s.light_field_res = 3
        s.set_light_field_tris(part, first=7)
        s.set_light_field(part, first=7)
        drop()
        assert not s.get_light_field_tris().any() and not s.get_light_field().any()
    # the same resolution again keeps both tables; sr_build with other tree parameters keeps them too
    s.light_field_res = 3
    s.set_light_field_tris(part, first=7)
    s.light_field_res = 3
    s.build((sa.MODE_REF_TREE,), 6, 4)
    assert np.array_equal(s.get_light_field_tris(7, 20), part)


def test_refusals_before_the_device_is_looked_at():
    """Validation comes first: a host-only scene answers the refusal, not SR_ERR_NO_DEVICE."""
    s = sa.GpuScene(device=-1)
    s.set_triangles(*load_obj3ds())
    s.light_field_triangles = True
    f = sa.Frame.from_buffer_copy(bytes(lfm.gpu_frame("contention")[3]))

    def code(frame, call=None):
        with pytest.raises(sa.SoftrayError) as e:
            (call or s.render)(frame)
        return e.value.code

    f.trace_mode = sa.MODE_REF_TREE
    assert code(f) == sa._lib.SR_ERR_NOT_BUILT               # no reference tree
    assert code(f, s.bake_light_field) == sa._lib.SR_ERR_NOT_BUILT
    s.build((sa.MODE_BVH,), on_device=False)
    f.trace_mode = sa.MODE_BVH
    assert code(f) == sa._lib.SR_ERR_NOT_BUILT               # the own BVH alone is not enough: stages 1 and 2 read the reference tree
    s.build((sa.MODE_REF_TREE,))
    assert code(f) == sa._lib.SR_ERR_NO_DEVICE
    f.trace_mode = sa.MODE_BRUTE
    assert code(f) == sa._lib.SR_ERR_UNSUPPORTED
    assert code(f, s.bake_light_field) == sa._lib.SR_ERR_UNSUPPORTED
    s.light_field_shadows = True                             # the colour method's switch does not let shadows through here
    for change in lfm.REFUSED:
        g = lfm.apply_change(sa.Frame.from_buffer_copy(bytes(lfm.gpu_frame("contention")[3])), change)
        g.trace_mode = sa.MODE_REF_TREE
        assert code(g) == sa._lib.SR_ERR_UNSUPPORTED, change
    s.light_field_triangles = False                          # switch off: the dynamic-shadow frame is the colour method's again
    g = lfm.apply_change(sa.Frame.from_buffer_copy(bytes(lfm.gpu_frame("contention")[3])), lfm.REFUSED[0])
    g.trace_mode = sa.MODE_REF_TREE
    assert code(g) == sa._lib.SR_ERR_NO_DEVICE


def test_mirrors_text():
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "void LightFieldTriangles(bool" in hpp and "sr_set_light_field_triangles" in hpp and "LightFieldStoresTriangles = true" in hpp
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    for name in ("sr_set_light_field_triangles", "sr_get_light_field_triangles", "sr_get_light_field_tris", "sr_set_light_field_tris", "LightFieldTriangles"):
        assert name in cs
