"""sr_refit_triangles_device without a device: the export is in the header, in the library and in the ctypes layer, the ABI version
stays 5, and a host-only scene refuses the call in the documented order -- the arguments first, then SR_ERR_NO_DEVICE."""
import ctypes as C
import os
import re

import numpy as np

import softray_amd as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "softray.h")
NAME = "sr_refit_triangles_device"


def test_export_in_header_library_and_ctypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, text)
    assert m, "include/softray.h does not declare %s" % NAME
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 7 and args[0].startswith("sr_scene*") and "int64_t n" in args[3] and args[6].startswith("void*")
    L = sa._lib.lib()
    assert hasattr(L, NAME) and NAME in sa._lib.SYMBOLS
    f = getattr(L, NAME)
    assert f.restype is C.c_int32 and len(f.argtypes) == 7 and f.argtypes[3] is C.c_int64
    assert f.argtypes == L.sr_set_triangles_device.argtypes          # the same call, the other fate for the tree
    assert hasattr(sa.GpuScene, "refit_triangles_device")


def test_abi_version_is_still_5():
    assert sa._lib.lib().sr_abi_version() == 5
    assert re.search(r"#define\s+SR_ABI_VERSION\s+5\b", open(HEADER).read())


def test_host_only_scene_checks_the_arguments_first_then_answers_no_device():
    L = sa._lib.lib()
    g = sa.GpuScene(-1)
    v9, argb = sa.make_random_triangles(10, 7, space=0.95, extent=0.05, origin=-0.5, opaque=True)
    lo, hi = np.array([-0.5] * 3), np.array([0.5] * 3)
    g.set_triangles(v9, argb, lo, hi)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(0x1000)                                        # never dereferenced: a host-only scene refuses before any device work
    call = lambda v, n, a=lo, b=hi: L.sr_refit_triangles_device(g._h, v, None, n, p(a), p(b), None)
    bad, nodev = sa._lib.SR_ERR_INVALID_ARG, sa._lib.SR_ERR_NO_DEVICE
    assert call(fake, -1) == bad
    assert call(fake, 0x7fffff01) == bad
    assert call(None, 10) == bad
    assert call(fake, 10, a=None) == bad and call(fake, 10, b=None) == bad
    assert L.sr_refit_triangles_device(None, fake, None, 10, p(lo), p(hi), None) == bad
    assert call(fake, 10) == nodev
    assert call(fake, 11) == nodev                                   # (the device is looked at before the model: the count is not compared yet)
    assert b"host-only" in L.sr_last_error()
    # ... and nothing happened to the scene
    got = g.get_triangles()
    assert np.array_equal(got[0], v9) and np.array_equal(got[1], argb) and g.num_triangles() == 10
    empty = sa.GpuScene(-1)
    assert L.sr_refit_triangles_device(empty._h, fake, None, 10, p(lo), p(hi), None) == nodev
