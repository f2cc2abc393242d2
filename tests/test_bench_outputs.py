"""bench.py's lean default and its output dump: a plain run prints the headline line only (everything else is behind --full), and
--dump-outputs DIR writes the frame of the last timed step as float arrays that two builds can be compared with."""
import glob
import os

import numpy as np
import pytest

import bench
from test_bench_multi import _bench


def _load(d):
    return {os.path.basename(p)[:-4]: np.load(p) for p in sorted(glob.glob(os.path.join(d, "*.npy")))}


def _packed(dump):
    c = dump["frame_pixels"].astype(np.uint32)
    return (c[:, 0] << 24) | (c[:, 1] << 16) | (c[:, 2] << 8) | c[:, 3]


def test_dump_outputs_is_float_bounded_seeded_and_exact(tmp_path):
    bench._imports()
    res = 4096                                                       # the headline frame: larger than the sample
    frame = np.random.default_rng(7).integers(-2 ** 31, 2 ** 31, res * res, dtype=np.int64).astype(np.int32)
    bench.dump_outputs(str(tmp_path / "a"), frame, res)
    bench.dump_outputs(str(tmp_path / "b"), frame[::-1].copy(), res)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert set(a) == {"frame_row_xor", "frame_pixels", "frame_pixel_index"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(p) for p in glob.glob(str(tmp_path / "a" / "*.npy"))) <= 64 * 10 ** 6
    idx = a["frame_pixel_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0) and idx[-1] < res * res
    assert np.array_equal(a["frame_pixel_index"], b["frame_pixel_index"])       # the sample depends on the frame's size only
    px = frame.view(np.uint32)
    assert np.array_equal(_packed(a), px[idx])
    assert np.array_equal(a["frame_row_xor"].astype(np.uint32), np.bitwise_xor.reduce(px.reshape(res, res), axis=1))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_frame_it_timed(tmp_path):
    out = str(tmp_path / "dump")
    plain = _bench("--gpus", "1", "--verify", "--dump-outputs", out)
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0
    for k in ("hbm_resident", "roofline", "drop_in_call", "cpu_baseline", "primary_only", "surface_passes"):
        assert k not in plain
    d = _load(out)
    assert len(d["frame_pixel_index"]) == 1024 * 1024                # a 1024^2 frame is written whole
    crc = int(np.bitwise_xor.reduce(_packed(d)))
    assert crc == int(np.bitwise_xor.reduce(d["frame_row_xor"].astype(np.uint32))) == plain["verify"]["crc"]
    assert plain["verify"]["full_frame_equal"]
    full = _bench("--gpus", "1", "--full")
    assert full["frame_crc"] == crc and full["readback_equals_blocking_render"]
    for k in ("hbm_resident", "roofline", "drop_in_call", "primary_only", "surface_passes"):
        assert k in full
