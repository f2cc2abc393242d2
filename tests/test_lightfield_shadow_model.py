"""The colour light field with dynamic soft shadows, without a GPU: the CPU model (tests/lightfield_shadow_model.py) against the golden of
the reference's active test RaytraceLightField_Colors and against the oracle's shadowed frames, the figures and input conditions the GPU
tests (tests/test_gpu_lightfield_shadows.py) stand on, and the opt-in switch on every layer."""
import os
import re
import subprocess

import numpy as np
import pytest

import lightfield_bake as lfb
import lightfield_model as lfm
import lightfield_shadow_model as lsm
from helpers import GOLDEN, ROOT, load_obj3ds, make_frame, orc, read_bmp_rgb

# entries of the whole table that shadows change, (model, N): every entry that is not the background (lfb.NON_BACKGROUND) -- a hit's colour
# is at least modulated with 255, which is (c * 255) >> 8 per channel
SHADOW_CHANGES = {2: 24, 4: 194, 8: 3804, 12: 19166}


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(model, prims=()):
        key = (model, bool(prims))
        if key not in made:
            made[key] = lfb.oracle_scene(model, prims)
        return made[key]
    return get


# ---- 1. the reference's active golden ----
@pytest.mark.parametrize("target", [lfm.TRACE_ROOT_TREE, lfm.TRACE_NEAREST], ids=["tree", "nearest"])
def test_golden_from_an_empty_table(scenes, target):
    m = lsm.LightFieldShadowModel(64)
    got = m.render(scenes("obj.3ds"), lsm.golden_frame(), target)
    want = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", lsm.GOLDEN_NAME + ".bmp"))
    assert got.shape == want.shape == (100, 100)
    assert int(np.count_nonzero((got & 0xFFFFFF) != want)) == 0
    assert m.filled.size == 14937 and m.coord_margin > 4e-6
    plain = read_bmp_rgb(os.path.join(GOLDEN, "raytrace", "100x100", "shading_lightFieldColor_focalBlurx4.bmp"))
    assert int(np.count_nonzero(plain != want)) > 2000                       # the shadows are in it


# ---- 2. the shadow step is the oracle's ----
def _camera_frames():
    directional = make_frame(64, 48, shadows=True, point_light=False, shadow_samples=17)
    return {"obj_shaded": ("obj.3ds", (), make_frame(64, 48, shadows=True)),
            "obj_unshaded_yaw60": ("obj.3ds", (), make_frame(64, 48, shading=False, shadows=True, yaw_deg=60.0, pitch_deg=20.0)),
            "unit_cube_primitives": ("unit_cube_2000", lfm.ptm.PRIMITIVES, make_frame(64, 48, shadows=True, yaw_deg=25.0, pitch_deg=12.0, depth=1.6)),
            "directional_17": ("obj.3ds", (), directional)}


@pytest.mark.parametrize("name", sorted(_camera_frames()))
def test_shadow_step_on_camera_samples_equals_the_oracle(scenes, name):
    model, prims, f = _camera_frames()[name]
    o = scenes(model, prims)
    want, _ = o.render(f, threads=os.cpu_count() or 1)
    got = lsm.camera_shadow_render(o, f)
    assert int(np.count_nonzero(got.reshape(-1) != want)) == 0
    f.flags &= ~orc.F_SHADOWS
    plain, _ = o.render(f, threads=os.cpu_count() or 1)
    assert int(np.count_nonzero(plain != want)) > 100


# ---- 3. a cell's colour is a function of the cell ----
def test_cell_colour_does_not_depend_on_who_fills_it(scenes):
    o, n = scenes("obj.3ds"), 8
    f = lsm.gpu_frame("view0_n8")[3]
    whole = lsm.LightFieldShadowModel(n)
    whole.fill(o, f, np.arange(lfm.cache_entries(n), dtype=np.int64), lfm.TRACE_ROOT_TREE)
    lazy = lsm.LightFieldShadowModel(n)
    lazy.render(o, f)
    assert lazy.filled.size == 22                                                # (N = 8 is coarse: the frame's samples fall into 22 cells)
    assert np.array_equal(lazy.entries(lazy.filled), whole.entries(lazy.filled))
    other = lsm.LightFieldShadowModel(n)                                          # other samples of the same pose, other order of filling
    cells = lazy.filled[::-1].copy()
    for part in (cells[1::2], cells[0::2]):
        other.fill(o, f, part, lfm.TRACE_ROOT_TREE)
    assert np.array_equal(other.entries(lazy.filled), whole.entries(lazy.filled))


# ---- 4. the input conditions of the frames the GPU tests render ----
@pytest.mark.parametrize("name", sorted(lsm.gpu_frames()))
def test_gpu_frame_keeps_clear_of_cell_boundaries(name):
    _, _, n, f = lsm.gpu_frames()[name]
    _, coord_margin, term_margin = lfm.sample_cells(*lfm.ptm.camera_samples(f), n)
    print("%s: coordinate margin %.3g, term margin %.3g" % (name, coord_margin, term_margin))
    assert coord_margin > lfm.MARGIN and term_margin > lfm.MARGIN
    assert f.flags & orc.F_SHADOWS and f.flags & lfm.F_LIGHT_FIELD


# ---- 5. whole tables: shadows are in them ----
@pytest.mark.parametrize("n", [2, 4, 8, 12])
def test_whole_tables_differ_from_the_unshadowed_ones(scenes, n):
    o = scenes("obj.3ds")
    index = np.arange(lfm.cache_entries(n), dtype=np.int64)
    for shading in (False, True):
        plain = lfb.model_table(o, lfb.bake_frame(shading), n, lfm.TRACE_ROOT_TREE)
        m = lsm.LightFieldShadowModel(n)
        m.fill(o, lsm.shadow_frame(lfb.bake_frame(shading)), index, lfm.TRACE_ROOT_TREE)
        shadowed = m.entries(index)
        differ = int(np.count_nonzero(shadowed != plain))
        print("N = %d, shading %s: %d entries differ" % (n, shading, differ))
        assert differ == SHADOW_CHANGES[n] == lfb.NON_BACKGROUND[("obj.3ds", n)][0]
        assert np.array_equal(shadowed == lfb.BACKGROUND, plain == lfb.BACKGROUND) and np.all(shadowed != 0)


# ---- 6. the switch on every layer ----
def test_switch_is_declared_on_every_layer():
    header = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert re.search(r"\bint\s+sr_set_light_field_shadows\(sr_scene\*, int32_t on\);", header)
    assert re.search(r"\bint32_t\s+sr_get_light_field_shadows\(const sr_scene\*\);", header)
    assert "#define SR_ABI_VERSION 5" in header
    import softray_amd as sa
    assert sa._lib.lib().sr_abi_version() == 5
    for sym in ("sr_set_light_field_shadows", "sr_get_light_field_shadows"):
        assert sym in sa._lib.SYMBOLS and hasattr(sa._lib.lib(), sym)
    assert isinstance(sa.GpuScene.light_field_shadows, property)
    hpp = open(os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp")).read()
    assert "void LightFieldShadows(bool value)" in hpp and "sr_set_light_field_shadows" in hpp and "sr_get_light_field_shadows" in hpp
    assert "rayTraceLightField together with rayTraceShadows is out of scope (SR_F_LIGHT_FIELD)" in hpp       # the refusal keeps its text
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GpuRenderer.cs")).read()
    assert "public bool LightFieldShadows" in cs and "sr_set_light_field_shadows" in cs and "sr_get_light_field_shadows" in cs
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "sr_set_light_field_shadows" in open(os.path.join(ROOT, doc)).read(), doc
    # the Python mirror keeps refusing rayTraceLightField (tests/test_lightfield_model.py pins its list)
    assert "LightFieldShadows" not in open(os.path.join(ROOT, "softray_amd", "renderer.py")).read()


def host_scene(devices=None):
    import softray_amd as sa
    s = sa.GpuScene(-1)
    s.set_triangles(*load_obj3ds("obj2.3DS"))
    return s


def lf_shadow_frame(**kw):
    import softray_amd as sa
    return sa.Frame.from_buffer_copy(bytes(lsm.shadow_frame(lfm.lf_frame(make_frame(16, **kw)))))


def test_switch_on_a_host_only_scene():
    import softray_amd as sa
    s = host_scene()
    assert s.light_field_shadows is False
    for bad in (2, -1, 255):
        assert sa._lib.lib().sr_set_light_field_shadows(s._h, bad) == sa._lib.SR_ERR_INVALID_ARG
        assert s.light_field_shadows is False
    data = (np.arange(1000, dtype=np.uint32) * np.uint32(2654435761)) | np.uint32(1)
    s.light_field_res = 8
    s.set_light_field(data, first=100)
    s.light_field_shadows = True
    assert s.light_field_shadows is True
    assert np.array_equal(s.get_light_field(100, 1000), data)                             # the switch does not touch the table
    s.set_triangles(*load_obj3ds("obj2.3DS"))                                             # a new model keeps the setting (and drops the table)
    assert s.light_field_shadows is True and s.light_field_res == 8
    s.load_3ds(open(os.path.join(GOLDEN, "obj2.3DS"), "rb").read())
    assert s.light_field_shadows is True
    s.light_field_shadows = False
    assert s.light_field_shadows is False


def test_refusals_come_in_order_on_a_host_only_scene():
    """validate_frame runs before the device is looked at.  Switch off: the pair is SR_ERR_UNSUPPORTED with the text it always had; switch on:
    the frame and the bake only lack a device; every other refusal of a light-field frame stays."""
    import softray_amd as sa
    s = host_scene()
    s.build((sa.MODE_REF_TREE,))
    calls = (lambda f: s.render(f), lambda f: s.bake_light_field(f))
    for call in calls:
        with pytest.raises(sa.SoftrayError) as e:
            call(lf_shadow_frame())
        assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED
        assert "light field together with shadows (dynamic or static) is not supported (a cell stores a colour, not a surface point)" in str(e.value)
    s.light_field_shadows = True
    for call in calls:
        with pytest.raises(sa.SoftrayError) as e:
            call(lf_shadow_frame())
        assert e.value.code == sa._lib.SR_ERR_NO_DEVICE
        for change in lfm.REFUSED[1:]:                                                    # static shadows, AO, path tracing, voxels, bounces, one kernel, strips
            f = lfm.apply_change(lf_shadow_frame(), change)
            with pytest.raises(sa.SoftrayError) as e:
                call(f)
            assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED and "light field" in str(e.value), change
    with pytest.raises(sa.SoftrayError) as e:                                             # static shadows: the message of the pair
        s.render(lfm.apply_change(lf_shadow_frame(), lfm.REFUSED[1]))
    assert "shadows (dynamic or static)" in str(e.value)
    s.light_field_shadows = False
    with pytest.raises(sa.SoftrayError) as e:
        s.render(lf_shadow_frame())
    assert e.value.code == sa._lib.SR_ERR_UNSUPPORTED


def test_cpp_mirror_program_builds(tmp_path):
    """tests/cpp/lightfield_shadow_tests.cpp compiles against Engine3D.hpp; without a GPU the program fails loudly instead of computing anything."""
    import torch
    exe = str(tmp_path / "lightfield_shadow_tests")
    lib_dir = os.path.join(ROOT, "softray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "lightfield_shadow_tests.cpp"),
                           "-L" + lib_dir, "-lsoftray_hip", "-Wl,-rpath," + lib_dir])
    if not torch.cuda.is_available():
        r = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
        assert r.returncode == 3 and "no HIP device" in r.stderr
