"""Quad-linear interpolation of the colour light field, without a GPU: the CPU model (tests/lightfield_interp_model.py), the input conditions
and wrap counts of the frames tests/test_gpu_lightfield_interp.py renders, and the new switch on every layer."""
import os
import re

import numpy as np
import pytest

import lightfield_bake as lfb
import lightfield_interp_model as lim
import lightfield_model as lfm
from helpers import ROOT

FRAMES = lim.gpu_frames()


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(model, prims=()):
        key = (model, bool(prims))
        if key not in made:
            made[key] = lfb.oracle_scene(model, prims)
        return made[key]
    return get


# ---- 1. every frame meets the conditions under which colours and tables are pinned, and keeps clear of the sphere test's threshold ----
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_frame_meets_the_input_conditions(scenes, name):
    model, prims, n, f = FRAMES[name]
    coords, inside, term, _ = lim.frame_figures(name)
    m = lim.LightFieldInterpModel(lfm.LightFieldModel(n))
    got = m.render(scenes(model, prims), f, coords, inside)
    print("%s: largest F_k %.6f, channel values in [%.6f, %.6f], |term - 1e-10| >= %.3g, %d cells" %
          (name, m.coord_max, m.channel_range[0], m.channel_range[1], float(np.abs(term - lfm.EPSILON).min()), m.touched.size))
    assert m.conditions_hold()
    assert float(np.abs(term - lfm.EPSILON).min()) > lfm.MARGIN
    assert not np.isnan(coords).any()
    assert got.shape[1] == f.width and np.all(got >> 24 == 0xFF)
    assert m.filled.size == m.touched.size > 16                      # from an empty table
    nearest = lfm.LightFieldModel(n).render(scenes(model, prims), f)
    assert int(np.count_nonzero(nearest != got)) > 0                 # and it is not the nearest lookup


# ---- 2. the wraps every axis needs, as figures ----
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_wrap_counts(name):
    _, _, n, f = FRAMES[name]
    coords, inside, _, wraps = lim.frame_figures(name)
    need = lim.REQUIRED[name]
    print("%s: %d of %d samples inside, wraps u %d v %d s %d t %d" % ((name, int(inside.sum()), inside.size) + tuple(wraps)))
    for got, want in zip(wraps, need.get("wraps", (None,) * 4)):
        assert want is None or got == want
    if "inside" in need:
        assert (int(inside.sum()), inside.size) == (need["inside"], need["samples"])
    if need.get("misses"):
        assert 0 < int(inside.sum()) < inside.size and (f.start_row, f.end_row) == (5, 17)


def test_every_axis_wraps_in_some_frame():
    total = np.zeros(4, dtype=np.int64)
    for name in FRAMES:
        total += np.array(lim.frame_figures(name)[3])
    assert np.all(total > 0)


# ---- 3. the model itself ----
def test_blend_of_equal_entries_is_the_entry_up_to_one():
    rng = np.random.default_rng(5)
    coords = rng.random((4000, 4)) * np.array([8.0, 4.0, 8.0, 4.0])
    for c in (0xFF336699, 0x00FFFFFF, 0xFF000001):
        got, lo, hi = lim.blend(coords, np.full((4000, 16), c, dtype=np.uint32))
        for shift in (16, 8, 0):
            d = ((c >> shift) & 255) - ((got.astype(np.int64) >> shift) & 255)
            assert d.min() >= 0 and d.max() <= 1                   # weights sum to 1 within rounding: the byte is c or c - 1
        assert np.all(got >> 24 == 0xFF) and 0.0 <= lo and hi < 256.0


def test_blend_at_a_cell_corner_is_that_entry():
    coords = np.array([[3.0, 1.0, 5.0, 2.0]])
    entries = np.arange(16, dtype=np.uint32)[None, :] * np.uint32(0x010101) + np.uint32(0x10)
    got, _, _ = lim.blend(coords, entries)
    assert int(got[0]) == 0xFF000000 | int(entries[0, 0]) & 0xFFFFFF    # all fractions 0: neighbour (0, 0, 0, 0)


def test_neighbours_wrap_per_axis():
    n = 4
    cells = lim.neighbour_cells(np.array([[7.5, 3.5, 7.5, 3.5], [8.0, 0.0, 8.0, 0.0]]), n)
    u, v, s, t = lfm.decode(cells, n)
    assert u[0].tolist() == [7] * 8 + [0] * 8 and t[0].tolist() == [3, 0] * 8
    assert v[0].tolist() == ([3] * 4 + [0] * 4) * 2 and s[0].tolist() == ([7] * 2 + [0] * 2) * 4
    assert u[1].tolist() == [0] * 8 + [1] * 8 and s[1].tolist() == ([0] * 2 + [1] * 2) * 4     # a base coordinate of 2N is cell 0
    assert cells.max() < lfm.cache_entries(n)


def test_float4d_scales_by_2n_and_n():
    """A line along -z through the centre: p1 = (0, 0, R), p2 = (0, 0, -R): u = 0.5, s = 1.0 -- F_s = 2N exactly."""
    F, inside, term = lim.float4d(np.array([[0.0, 0.0, 2.0], [0.0, 2.0, 2.0]]), np.array([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0]]), 4)
    assert inside.tolist() == [True, False] and F[0].tolist() == [4.0, 2.0, 8.0, 2.0] and F[1].tolist() == [0.0] * 4
    assert lim.wrap_counts(F, inside, 4) == [0, 0, 1, 0]


def test_second_frame_on_the_warm_table_fills_nothing(scenes):
    _, _, n, f = FRAMES["pose_up"]
    coords, inside, _, _ = lim.frame_figures("pose_up")
    m = lim.LightFieldInterpModel(lfm.LightFieldModel(n))
    a = m.render(scenes("obj.3ds"), f, coords, inside)
    first = m.filled.size
    b = m.render(scenes("obj.3ds"), f, coords, inside)
    assert first > 0 and m.filled.size == 0 and np.array_equal(a, b)


# ---- 4. the new symbols are exported and bound on every layer ----
NEW = ["sr_set_light_field_interpolation", "sr_get_light_field_interpolation", "sr_light_field_coords"]


def _text(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_new_symbols_are_declared_exported_and_bound():
    import softray_amd as sa
    header = _text("include", "softray.h")
    api = _text("softray_amd", "csrc", "sr_api.cpp")
    cs = _text("bindings", "csharp", "GpuRenderer.cs")
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header) and re.search(r"^int(32_t)?\s+%s\(" % name, api, re.M)
        assert name in sa._lib.SYMBOLS and name in cs
        assert getattr(sa._lib.lib(), name).argtypes is not None
    assert "#define SR_ABI_VERSION 5" in header
    assert isinstance(sa.GpuScene.light_field_interpolation, property) and callable(sa.GpuScene.light_field_coords)
    hpp = _text("softray_amd", "host", "Engine3D.hpp")
    assert "void LightFieldInterpolate(bool value)" in hpp and "bool LightFieldInterpolate() const" in hpp
    assert "public bool LightFieldInterpolation" in cs
    pipe = _text("softray_amd", "csrc", "sr_pipeline.hip")
    for kernel in ("lf_float4d", "k_lf_coords", "k_lfi_lookup", "k_lfi_apply"):
        assert kernel in pipe


def test_switch_on_a_host_only_scene():
    """Setter, getter and refusals need no device; the coordinates do."""
    import softray_amd as sa
    g = sa.GpuScene(-1)
    lib, h = sa._lib.lib(), g._h
    assert g.light_field_interpolation is False
    g.light_field_interpolation = True
    assert g.light_field_interpolation is True and lib.sr_get_light_field_interpolation(h) == 1
    for bad in (2, -1, 256):
        assert lib.sr_set_light_field_interpolation(h, bad) == sa._lib.SR_ERR_INVALID_ARG
        assert lib.sr_get_light_field_interpolation(h) == 1
    assert lib.sr_set_light_field_interpolation(None, 1) == sa._lib.SR_ERR_INVALID_ARG and lib.sr_get_light_field_interpolation(None) == 0
    v = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    g.set_triangles(v, np.array([0xFFFFFFFF], dtype=np.uint32), np.zeros(3), np.ones(3))
    assert g.light_field_interpolation is True                       # survives new triangles
    g.light_field_interpolation = False
    assert lib.sr_get_light_field_interpolation(h) == 0
    one = np.zeros(3)
    out4, out1 = np.zeros(4), np.zeros(1, dtype=np.uint8)
    p = lambda a: a.ctypes.data
    assert lib.sr_light_field_coords(h, -1, p(one), p(one), p(out4), p(out1)) == sa._lib.SR_ERR_INVALID_ARG
    assert lib.sr_light_field_coords(h, 1, None, p(one), p(out4), p(out1)) == sa._lib.SR_ERR_INVALID_ARG
    assert lib.sr_light_field_coords(h, 1, p(one), p(one), p(out4), None) == sa._lib.SR_ERR_INVALID_ARG
    assert lib.sr_light_field_coords(h, 1, p(one), p(one), p(out4), p(out1)) == sa._lib.SR_ERR_NO_DEVICE
    assert lib.sr_light_field_coords(h, 0, None, None, None, None) == sa._lib.SR_ERR_NO_DEVICE


def test_python_renderer_mirror_still_refuses_light_fields():
    src = _text("softray_amd", "renderer.py")
    assert "light_field_interpolation" not in src
