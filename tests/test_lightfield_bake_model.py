"""sr_bake_light_field without a GPU: the figures of the CPU model's whole tables that tests/test_gpu_lightfield_bake.py stands on, the
symbol on every layer, and the order in which a host-only scene answers -- arguments, range and frame before the device is looked at."""
import os
import re
import subprocess

import numpy as np
import pytest

import lightfield_bake as lfb
import lightfield_model as lfm
from helpers import GOLDEN, ROOT, load_obj3ds


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(model):
        if model not in made:
            made[model] = lfb.oracle_scene(model)
        return made[model]
    return get


# ---- 1. the model's whole tables ----
# (unit cube at N = 16: the reference tree only -- its global-nearest table takes several seconds and is computed by the GPU tests, which compare it)
TABLES = [("obj.3ds", 2, "root_tree"), ("obj.3ds", 4, "root_tree"), ("obj.3ds", 8, "root_tree"), ("obj.3ds", 12, "root_tree"),
          ("obj.3ds", 8, "nearest"), ("obj.3ds", 12, "nearest"), ("unit_cube_2000", 8, "nearest"), ("unit_cube_2000", 8, "root_tree"),
          ("unit_cube_2000", 16, "root_tree")]
TARGETS = {"root_tree": lfm.TRACE_ROOT_TREE, "nearest": lfm.TRACE_NEAREST}


@pytest.mark.parametrize("model,n,target", TABLES)
def test_whole_table_of_the_model(scenes, model, n, target):
    o = scenes(model)
    want_hit, want_total = lfb.NON_BACKGROUND[(model, n)]
    tables = []
    for shading in (False, True):
        t = lfb.model_table(o, lfb.bake_frame(shading), n, TARGETS[target])
        assert t.size == want_total == lfm.cache_entries(n)
        assert not np.any(t == 0)                                                # no entry stays empty
        assert int(np.count_nonzero(t != lfb.BACKGROUND)) == want_hit
        assert np.all(t[lfb.diagonal_cells(n)] == lfb.BACKGROUND)                # zero-length directions hit nothing
        tables.append(t)
    assert np.array_equal(tables[0] != lfb.BACKGROUND, tables[1] != lfb.BACKGROUND)
    assert not np.array_equal(tables[0], tables[1])                              # (shading changes the colours, not which rays hit)


def test_resolution_one_is_all_background(scenes):
    """N = 1 has no latitude: the four patch centres are NaN, nothing is hit."""
    t = lfb.model_table(scenes("obj.3ds"), lfb.bake_frame(), 1, lfm.TRACE_ROOT_TREE)
    assert t.tolist() == [lfb.BACKGROUND] * 4
    assert np.isnan(lfm.sphere_points(1)).any()


def test_model_entries_do_not_depend_on_what_else_is_filled(scenes):
    """A range of the table is the same range of the whole table: what lets a bake be cut into chunks."""
    o, f, n = scenes("obj.3ds"), lfb.bake_frame(), 8
    whole = lfb.model_table(o, f, n, lfm.TRACE_ROOT_TREE)
    index = np.arange(5001, 11000)
    assert np.array_equal(lfb.model_entries(o, f, n, index, lfm.TRACE_ROOT_TREE), whole[index])


def test_both_targets_agree_on_obj3ds_at_8(scenes):
    """The reference tree and the global nearest hit give the same table for this model at this resolution: what lets the GPU test of extra
    geometry (which only the tree target knows) hold the SR_MODE_BVH bake to the tree target's table too."""
    o, f = scenes("obj.3ds"), lfb.bake_frame()
    assert np.array_equal(lfb.model_table(o, f, 8, lfm.TRACE_ROOT_TREE), lfb.model_table(o, f, 8, lfm.TRACE_NEAREST))


# ---- 2. the symbol on every layer ----
def test_symbol_is_declared_on_every_layer():
    import softray_amd as sa
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert re.search(r"\bint\s+sr_bake_light_field\s*\(\s*sr_scene\s*\*\s*,\s*const\s+sr_frame\s*\*", header)
    assert "sr_bake_light_field" in sa._lib.SYMBOLS
    assert hasattr(sa._lib.lib(), "sr_bake_light_field") and hasattr(sa.GpuScene, "bake_light_field")
    assert sa._lib.lib().sr_abi_version() == 5
    assert re.search(r"SR_DBG_COUNT\s*=\s*17\b", header)
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    assert "sr_bake_light_field" in cs and "BakeLightField" in cs
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "sr_bake_light_field" in hpp and "BakeLightField" in hpp
    names = open(os.path.join(ROOT, "softray_amd", "csrc", "sr_kernels.hip")).read()
    assert '"k_lf_bake"' in names


# ---- 3. a host-only scene: what is wrong with the request is said before the device is looked at ----
def host_scene(n=8):
    import softray_amd as sa
    s = sa.GpuScene(-1)
    s.set_triangles(*load_obj3ds("obj.3ds"))
    s.build((sa.MODE_REF_TREE,))
    s.light_field_res = n
    return s


def sr_frame(f):
    import softray_amd as sa
    return sa.Frame.from_buffer_copy(bytes(f))


def test_host_only_scene_answers_in_order():
    import softray_amd as sa
    s = host_scene(8)
    total = lfm.cache_entries(8)
    good = sr_frame(lfb.bake_frame())
    # no SR_F_LIGHT_FIELD: the first complaint, even for a frame that would be refused and a range beyond the table
    for change in [dict()] + lfm.REFUSED:
        plain = lfm.apply_change(sr_frame(lfb.bake_frame()), change)
        plain.flags &= ~lfm.F_LIGHT_FIELD
        for first, count in ((0, total), (0, total + 1)):
            with pytest.raises(sa.SoftrayError) as e:
                s.bake_light_field(plain, first, count)
            assert e.value.code == sa._lib.SR_ERR_INVALID_ARG and "SR_F_LIGHT_FIELD" in str(e.value), change
    # a range beyond 4 N^4, in the words of sr_get_light_field; also for a frame that would be refused
    for frame in (good, lfm.apply_change(sr_frame(lfb.bake_frame()), lfm.REFUSED[0])):
        for first, count in ((0, total + 1), (total + 1, 0), (total - 10, 11), (1, 2 ** 64 - 1)):
            with pytest.raises(sa.SoftrayError) as e:
                s.bake_light_field(frame, first, count)
            assert e.value.code == sa._lib.SR_ERR_INVALID_ARG and "the range exceeds the 4 N^4 entries" in str(e.value)
    # the combinations a light-field frame is refused with
    for change in lfm.REFUSED:
        bad = lfm.apply_change(sr_frame(lfb.bake_frame()), change)
        with pytest.raises(sa.SoftrayError) as e:
            s.bake_light_field(bad)
        assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED and "light field" in str(e.value), change
    # sr_render's other checks
    small = sr_frame(lfb.bake_frame())
    small.width = 0
    with pytest.raises(sa.SoftrayError) as e:
        s.bake_light_field(small)
    assert e.value.code == sa._lib.SR_ERR_INVALID_ARG
    unbuilt = sr_frame(lfb.bake_frame())
    unbuilt.trace_mode = sa.MODE_BVH
    with pytest.raises(sa.SoftrayError) as e:
        s.bake_light_field(unbuilt)
    assert e.value.code == sa._lib.SR_ERR_NOT_BUILT
    # a valid request only lacks a device
    for first, count in ((0, None), (5001, 5999), (total - 1, 1)):
        with pytest.raises(sa.SoftrayError) as e:
            s.bake_light_field(good, first, count)
        assert e.value.code == sa._lib.SR_ERR_NO_DEVICE
    assert not s.get_light_field().any()                                         # and nothing was written on the way


def test_null_arguments():
    import ctypes as C
    import softray_amd as sa
    L = sa._lib.lib()
    s = host_scene(2)
    good = sr_frame(lfb.bake_frame())
    assert L.sr_bake_light_field(None, C.byref(good), 0, 1, None) == sa._lib.SR_ERR_INVALID_ARG
    assert L.sr_bake_light_field(s._h, None, 0, 1, None) == sa._lib.SR_ERR_INVALID_ARG
    assert L.sr_bake_light_field(s._h, C.byref(good), 0, 1, None) == sa._lib.SR_ERR_NO_DEVICE       # filled may be NULL


def test_cpp_mirror_bake_program_builds(tmp_path):
    """tests/cpp/lightfield_bake_tests.cpp compiles against Engine3D.hpp; without a GPU the program fails loudly instead of computing anything."""
    import torch
    exe = str(tmp_path / "lightfield_bake_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "lightfield_bake_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    if not torch.cuda.is_available():
        r = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
        assert r.returncode == 3 and "no HIP device" in r.stderr
