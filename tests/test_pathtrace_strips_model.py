"""The row bases of a path-traced frame that a multi-device scene has split (softray_amd/csrc/sr_pipeline.hip k_pt_row_base), stated in
numpy and checked against the unsplit frame: for every row a part owns, row_k0 is the number of hits -- of any part -- that precede the
row inside its row block.  The row blocks are those of the frame's clamped row range, not of the part's rows.  No GPU."""
import os
import re

import numpy as np

from helpers import ROOT

STRIP_ROWS = 16                                  # kMultiStripRows (sr_api.cpp): part g renders the strips s with s % n == g


def clamp_rows(height, start_row, end_row):
    return min(max(0, start_row), height - 1), min(max(0, end_row), height - 1)


def owned_rows(a, b, n, g):
    """Image rows of part g, ascending: the part's row map (compact row -> image row)."""
    r = np.arange(a, b + 1)
    return r[(r // STRIP_ROWS) % n == g]


def block_height(range_rows, concurrency):
    conc = concurrency if concurrency > 0 else 4
    return (range_rows - 1 + conc) // conc


def row_k0(row_hits, a, concurrency, row_map):
    """row_hits: hits per image row of the range [a, a + len) -- the merged counts of all parts.  The exclusive prefix sum that restarts
    at every block boundary, gathered through the part's row map."""
    rows = row_hits.size
    bh = block_height(rows, concurrency)
    excl = np.zeros(rows, dtype=np.int64)
    for first in range(0, rows, bh):
        seg = row_hits[first:first + bh].astype(np.int64)
        excl[first:first + bh] = np.cumsum(seg) - seg
    return excl[np.asarray(row_map, dtype=np.int64) - a]


def merged_counts(row_hits, a, b, n):
    """What the exchange leaves on every part: each part writes the rows it owns into a zeroed array, nobody writes another's row."""
    out = np.zeros(b - a + 1, dtype=np.int64)
    written = np.zeros(b - a + 1, dtype=np.int64)
    for g in range(n):
        rows = owned_rows(a, b, n, g)
        out[rows - a] = row_hits[rows - a]
        written[rows - a] += 1
    assert np.all(written == 1)                  # every row of the range has exactly one owner
    return out


def brute_preceding(hit, width, a, concurrency, row):
    """Hits of the unsplit frame that precede image row `row` inside its block (the definition: a loop over samples)."""
    rows = hit.size // width
    bh = block_height(rows, concurrency)
    first = ((row - a) // bh) * bh
    return int(hit[first * width:(row - a) * width].sum())


def test_row_k0_is_the_count_of_preceding_hits_of_the_block():
    rng = np.random.default_rng(20240607)
    cases = 0
    for _ in range(300):
        height = int(rng.integers(1, 260))
        width = int(rng.integers(1, 9))
        start, end = int(rng.integers(-10, height + 10)), int(rng.integers(-10, height + 300))
        a, b = clamp_rows(height, start, end)
        if b < a:
            continue
        conc = int(rng.choice([0, 1, 2, 3, 4, 7, 8, 64, 500]))
        n = int(rng.choice([1, 2, 3, 5, 8, 13]))
        hit = (rng.random((b - a + 1) * width) < rng.random()).astype(np.int64)
        per_row = hit.reshape(-1, width).sum(1)
        merged = merged_counts(per_row, a, b, n)
        assert np.array_equal(merged, per_row)
        for g in range(n):
            rows = owned_rows(a, b, n, g)
            k0 = row_k0(merged, a, conc, rows)
            assert k0.size == rows.size
            for j, r in enumerate(rows):
                assert k0[j] == brute_preceding(hit, width, a, conc, int(r)), (height, a, b, conc, n, g, int(r))
            cases += 1
    assert cases > 500


def test_row_k0_agrees_with_the_models_hit_indices():
    """k of a sample = row_k0 of its row + the hits before it in the row: the same numbers as pathtrace_model.hit_indices gives the
    unsplit frame."""
    import pathtrace_model as ptm
    rng = np.random.default_rng(7)
    for rows, width, conc, n in ((67, 90, 3, 2), (67, 5, 500, 3), (100, 4, 0, 8), (5, 3, 4, 8), (48, 7, 7, 3), (200, 2, 1, 8)):
        hit = (rng.random(rows * width) < 0.4).astype(np.int64)
        want = ptm.hit_indices(hit, width, rows, conc).reshape(rows, width)
        per_row = hit.reshape(rows, width).sum(1)
        in_row = np.cumsum(hit.reshape(rows, width), axis=1) - hit.reshape(rows, width)
        a = 11                                                                # the range starts anywhere: strips are cut in image rows
        for g in range(n):
            own = owned_rows(a, a + rows - 1, n, g)
            k0 = row_k0(per_row, a, conc, own)
            assert np.array_equal(k0[:, None] + in_row[own - a], want[own - a])


def test_block_boundaries_fall_inside_strips():
    """The goldens' case: 100 rows, 7 strips of 16 rows, blocks of 25 rows -- every block boundary lies inside a strip."""
    bh = block_height(100, 0)
    assert bh == 25 and all((k * bh) % STRIP_ROWS for k in (1, 2, 3))
    assert len({int(r) // STRIP_ROWS for r in range(100)}) == 7
    per_row = np.arange(1, 101, dtype=np.int64)
    for n in (2, 3, 8):
        for g in range(n):
            own = owned_rows(0, 99, n, g)
            k0 = row_k0(per_row, 0, 0, own)
            for j, r in enumerate(own):
                first = (int(r) // 25) * 25
                assert k0[j] == per_row[first:int(r)].sum()


def test_one_row_per_block_and_one_block():
    per_row = np.array([3, 0, 9, 1, 4], dtype=np.int64)
    assert np.array_equal(row_k0(per_row, 0, 500, np.arange(5)), np.zeros(5))             # block height 1: every row starts a block
    assert np.array_equal(row_k0(per_row, 0, 1, np.arange(5)), [0, 3, 3, 12, 13])
    assert np.array_equal(row_k0(per_row, 40, 1, [41, 44]), [3, 13])


def test_header_declares_sr_last_frame_parts():
    text = open(os.path.join(ROOT, "include", "softray.h")).read()
    assert re.search(r"int32_t\s+sr_last_frame_parts\s*\(\s*const\s+sr_scene\s*\*\s*\)\s*;", text)
    from softray_amd import _lib
    assert "sr_last_frame_parts" in _lib.SYMBOLS


def test_cpp_mirror_has_the_accessor(tmp_path):
    """softray_amd/host/Engine3D.hpp: Renderer::gpuLastFrameParts() compiles against the header (compilation only: no device here)."""
    import subprocess
    src = tmp_path / "parts.cpp"
    src.write_text('#include "%s"\n'
                   "int parts_of(const Engine3D::Renderer& r) { return r.gpuLastFrameParts(); }\n"
                   "int32_t (*const export_of)(const sr_scene*) = &sr_last_frame_parts;\n" % os.path.join(ROOT, "softray_amd", "host", "Engine3D.hpp"))
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)])
