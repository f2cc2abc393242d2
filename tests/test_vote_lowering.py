"""The one toolchain behaviour the packet walks' vote idiom rests on (sr_device.h, vote helpers), checked in the ISA -- no GPU needed.

tests/cpp/vote_probe.hip runs the helpers through a loop of the walks' shape: a vote over a conjunction of comparisons and a loop-carried
mask, a per-lane update and a store under a mask.  Written with lane masks (probe_masks) the loop must hold NO pair

    v_cndmask_b32 vN, 0, 1, <mask>    ->    v_cmp_ne_u32 <mask>, 0, vN

i.e. no mask that already was in scalar registers is turned into a 0/1 vector register and compared back.  The control (probe_bools: the
same loop with `bool` predicates and __ballot(a && b && !done)) is only reported: a compiler that learns to fold the pair there is good news,
not a failure.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softray_amd", "csrc")
PROBE = os.path.join(ROOT, "tests", "cpp", "vote_probe.hip")


def hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    return None


pytestmark = pytest.mark.skipif(hipcc() is None, reason="no hipcc")

CNDMASK01 = re.compile(r"^\s*v_cndmask_b32\w*\s+(v\d+), 0, 1, (?:s\[\d+:\d+\]|vcc)\s*(?:;.*)?$")
CMPNE0 = re.compile(r"^\s*v_cmp_ne_u32\w*\s+(?:vcc|s\[\d+:\d+\]), 0, (v\d+)\s*(?:;.*)?$")
WRITES = re.compile(r"^\s*v_\w+\s+(v\d+)\b")


def makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(.+)$", text, re.M).group(1).strip()
    flags = [f for f in re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", text, re.M).group(1).split() if f not in ("-fPIC", "-pthread")]
    return arch, flags


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{kernel name: its instruction lines} of the probe, compiled with the library's flags."""
    out = str(tmp_path_factory.mktemp("vote_probe") / "vote_probe.s")
    arch, flags = makefile_flags()
    subprocess.run([hipcc(), "--offload-arch=" + arch] + flags + ["-I", CSRC, "--cuda-device-only", "-S", "-o", out, PROBE], check=True, capture_output=True)
    body, name = {}, None
    for ln in open(out):
        m = re.match(r"^(probe_\w+):", ln)
        if m:
            name = m.group(1)
            body[name] = []
        elif ln.startswith(".Lfunc_end"):
            name = None
        elif name:
            body[name].append(ln.rstrip("\n"))
    assert set(body) == {"probe_masks", "probe_bools"}, sorted(body)
    return body


def loop_lines(lines):
    """the instructions of the blocks that lie inside a loop (LLVM comments every block label with the loop it belongs to)"""
    out, inside = [], False
    for ln in lines:
        if re.match(r"^\.LBB\d+_\d+:", ln):
            inside = "Loop" in ln
        elif inside and ln.startswith("\t"):
            out.append(ln)
    return out


def vote_pairs(lines):
    pending, pairs = set(), 0
    for ln in lines:
        c = CNDMASK01.match(ln)
        if c:
            pending.add(c.group(1))
            continue
        c = CMPNE0.match(ln)
        if c and c.group(1) in pending:
            pairs += 1
            pending.discard(c.group(1))
            continue
        w = WRITES.match(ln)
        if w:
            pending.discard(w.group(1))
    return pairs


def test_the_detector_sees_a_pair():
    """the pattern itself, on the four lines the bool idiom compiles to today"""
    sample = ["\ts_and_b64 s[10:11], s[14:15], s[10:11]", "\tv_cndmask_b32_e64 v2, 0, 1, s[10:11]", "\tv_cmp_ne_u32_e32 vcc, 0, v2", "\ts_cbranch_vccz .LBB49_7"]
    assert vote_pairs(sample) == 1
    assert vote_pairs(sample[:2] + ["\tv_mov_b32_e32 v2, 0"] + sample[2:]) == 0


def test_mask_votes_compile_without_a_vector_round_trip(kernels):
    loop = loop_lines(kernels["probe_masks"])
    assert len(loop) > 10, "the probe's loop was not found"
    control = vote_pairs(loop_lines(kernels["probe_bools"]))
    print("vote pairs in the loop: masks %d, bool control %d" % (vote_pairs(loop), control))
    assert vote_pairs(loop) == 0, "\n".join(loop)
    # the vote is a scalar test of the mask, and the mask algebra stays on the scalar unit
    assert any(re.match(r"^\s*s_cmp_(eq|lg)_u64", ln) or re.match(r"^\s*s_cbranch_(scc|vcc)", ln) for ln in loop)
    assert any(re.match(r"^\s*s_(and|andn2|or)_b64", ln) for ln in loop)
    # the loop-carried mask never visits a vector register: no v_cmp reads back a 0/1 register it was parked in
    assert not any(re.match(r"^\s*v_cmp_(eq|ne)_u(16|32)\w*\s+\S+ (0|1), v\d+", ln) for ln in loop), "\n".join(loop)
