"""Static census of the wave votes in the headline kernels' gfx950 ISA (no GPU needed, about two minutes of compile time).

    python scripts/isa_vote_census.py [--asm FILE.s] [--all] > profiles/r06_votes/isa_census_new.txt

Compiles softray_amd/csrc/sr_pipeline.hip to assembly with the Makefile's flags (or reads --asm) and prints, for every instantiation of
k_shaft_pkt4 / k_primary / k_shadow_cls_g: registers, spills, scratch, occupancy, static VALU / SALU instruction counts, the number of
v_readlane / v_writelane (SGPR spills to VGPR lanes), and the VOTE PAIRS

    v_cndmask_b32 vN, 0, 1, s[..]   ->   v_cmp_ne_u32 .., 0, vN

-- a lane predicate that already was a mask in scalar registers, turned into a 0/1 vector register and compared back into a mask: what
__ballot(a && b) costs on this toolchain (sr_device.h, vote helpers) -- with the loop each pair sits in.  A loop is named by the label of
its header, innermost first; "node128" = a block of the loop reads a 128-byte node with scalar loads, i.e. the walk loop of the packet
walks.  Without --all only the headline instantiations are listed in full, the others in one line each.

For a headline instantiation every node128 loop also gets its static INSTRUCTION MIX (all blocks of the loop, nested loops included), by
mnemonic class only: scalar ALU, scalar memory, branches, s_nop, s_waitcnt -- the scalar side: one scalar unit serves the four SIMDs of
a CU -- then vector moves, other vector instructions, vector memory / LDS.  Static counts: a loop that gains branches to
skip work may count more and execute less; the SQ_INSTS_* counters are the executed side (profiles/r10_scalar_walks).
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softray_amd", "csrc")
KERNELS = ("k_shaft_pkt4", "k_primary", "k_shadow_cls_g")
# the instantiations the default frames run (every KNOWN subset of the light / both forms of the camera-ordered copy): listed pair by pair
HEADLINE = re.compile(r"^(k_shaft_pkt4<false, 6, true, \d(?:, (?:true|false)){0,2}>|k_primary<2, false, false, false, [23], false>|k_shadow_cls_g<false, false>)$")


def makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(.+)$", text, re.M).group(1).strip()
    arch = re.search(r"^ARCH\s*\?=\s*(.+)$", text, re.M).group(1).strip()
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", text, re.M).group(1).split()
    return os.environ.get("HIPCC", hipcc), arch, flags


def compile_asm(out):
    hipcc, arch, flags = makefile_flags()
    cmd = [hipcc, "--offload-arch=" + arch] + flags + ["--cuda-device-only", "-S", "-o", out, "sr_pipeline.hip"]
    subprocess.check_call(cmd, cwd=CSRC, stderr=subprocess.DEVNULL)


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {m: re.sub(r"^void (sr::)?", "", d).split("(")[0] for m, d in zip(names, out)}
    except (OSError, subprocess.CalledProcessError):
        return {m: m for m in names}


INSN = re.compile(r"^\t([vs]_[a-z0-9_]+|ds_[a-z0-9_]+|global_[a-z0-9_]+|scratch_[a-z0-9_]+|buffer_[a-z0-9_]+|flat_[a-z0-9_]+)\b(.*)$")
LABEL = re.compile(r"^(\.LBB\d+_\d+):\s*(?:;(.*))?$")
CNDMASK01 = re.compile(r"^\s*(v\d+), 0, 1, (s\[\d+:\d+\]|vcc)\s*$")
CMPNE0 = re.compile(r"^\s*(?:vcc|s\[\d+:\d+\]), 0, (v\d+)\s*$")


MIX_CLASSES = ("scalar ALU", "scalar memory", "branches", "s_nop", "s_waitcnt", "vector moves", "other vector", "vector memory / LDS")
SCALAR_SIDE = MIX_CLASSES[:5]


def mix_class(op):
    """Class of an instruction by its mnemonic alone (no operands looked at)."""
    if op == "s_nop":
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith(("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_call")):
        return "branches"
    if op.startswith(("s_load_", "s_buffer_load_", "s_scratch_load_")):
        return "scalar memory"
    if op.startswith("s_"):
        return "scalar ALU"
    if op.startswith("v_mov_"):
        return "vector moves"
    if op.startswith("v_"):
        return "other vector"
    return "vector memory / LDS"


def census(lines):
    """lines: the body of one function.  Returns counts and the list of (pair line, loop label chain)."""
    # loops: LLVM's asm printer comments every block with the loop it is in: "=>This Loop Header: Depth=d", "Parent Loop BBx_y Depth=d",
    # "in Loop: Header=BBx_y Depth=d" (innermost loop of a non-header block)
    valu = salu = lanes = 0
    mix = {}                            # block -> {class of MIX_CLASSES: instructions}
    block, block_loop = None, {}        # label -> innermost loop header label ('' outside loops)
    header_parent = {}                  # loop header -> parent header
    loaded = {}                         # block -> dwords it reads with scalar loads
    lane_blocks = []                    # block of every v_readlane / v_writelane
    pairs, recent = [], {}              # recent: vreg -> index of a pending v_cndmask 0,1
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = LABEL.match(ln)
        if m:
            block = m.group(1)
            # the label's comment and its continuation lines (blank up to the ';'): the enclosing loops outermost first, then the block's own role
            cm, j = [m.group(2) or ""], i + 1
            while j < len(lines) and re.match(r"^\s+;", lines[j]):
                cm.append(lines[j])
                j += 1
            cm = "\n".join(cm)
            if "Loop Header" in cm:
                block_loop[block] = block
                parents = re.findall(r"Parent Loop (BB\d+_\d+)", cm)
                header_parent[block] = ".L" + parents[-1] if parents else ""
            else:
                hm = re.search(r"in Loop: Header=(BB\d+_\d+)", cm)
                block_loop[block] = ".L" + hm.group(1) if hm else ""
            recent = {}
            i += 1
            continue
        m = INSN.match(ln)
        if m:
            op, args = m.group(1), m.group(2).split(";")[0]
            if block:
                per = mix.setdefault(block, {})
                per[mix_class(op)] = per.get(mix_class(op), 0) + 1
            if op.startswith("v_"):
                valu += 1
                if op.startswith(("v_readlane", "v_writelane")):
                    lanes += 1
                    lane_blocks.append(block)
                if op.startswith("v_cndmask_b32"):
                    c = CNDMASK01.match(args)
                    if c:
                        recent[c.group(1)] = i
                elif op.startswith("v_cmp_ne_u32"):
                    c = CMPNE0.match(args)
                    if c and c.group(1) in recent:
                        pairs.append(block)
                        del recent[c.group(1)]
                else:
                    # an instruction that overwrites the 0/1 register ends the candidate pair
                    d = re.match(r"\s*(v\d+)\b", args)
                    if d:
                        recent.pop(d.group(1), None)
            elif op.startswith("s_"):
                salu += 1
                ld = re.match(r"s_load_dword(?:x(\d+))?$", op)
                if ld and block:
                    loaded[block] = loaded.get(block, 0) + int(ld.group(1) or 1)
        i += 1

    def chain(b):
        out, h = [], block_loop.get(b, "")
        while h:
            out.append(h)
            h = header_parent.get(h, "")
        return out

    # a loop "loads a node" if one block whose innermost loop it is reads 128 bytes or more with scalar loads (the compiler may split the
    # node into several s_load_dwordxN; no other record of the walks is that large)
    node_loops = set()
    for b, n in loaded.items():
        if n >= 32 and block_loop.get(b):
            node_loops.add(block_loop[b])
    lanes_in_walk = sum(1 for b in lane_blocks if any(h in node_loops for h in chain(b)))
    # instruction mix of every node-loading loop: all blocks of the loop, those of the loops nested in it included
    loop_mix = {}
    for h in node_loops:
        tot = dict.fromkeys(MIX_CLASSES, 0)
        for b, per in mix.items():
            if h in chain(b):
                for k, v in per.items():
                    tot[k] += v
        loop_mix[h] = tot
    return valu, salu, lanes, lanes_in_walk, [(b, chain(b)) for b in pairs], node_loops, loop_mix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--all", action="store_true", help="list the pairs of every instantiation, not only of the headline ones")
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            compile_asm(os.path.join(d, "sr_pipeline.s"))
            text = open(os.path.join(d, "sr_pipeline.s")).read()
    lines = text.split("\n")
    funcs = {}
    start = name = None
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):\s", ln + " ")
        if m and any(k in m.group(1) for k in KERNELS) and not ln.startswith("\t"):
            name, start = m.group(1), i
        elif name and ln.startswith(".Lfunc_end"):
            funcs[name] = [start, i, {}]
            # the resource comment block follows the function
            for ln2 in lines[i:i + 60]:
                r = re.match(r"^; (TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", ln2)
                if r:
                    funcs[name][2][r.group(1)] = int(r.group(2))
            name = None
    spills = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n){0,12}?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n){0,8}?\s+\.vgpr_spill_count:\s+(\d+)", text):
        spills[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    pretty = demangle(list(funcs))
    print("# kernel | VGPR / SGPR / spilled V / spilled S / scratch B / occupancy | static VALU / SALU | v_readlane+v_writelane (in node128 walk loops) | vote pairs (in node128 walk loops)")
    for mangled in sorted(funcs, key=lambda k: pretty[k]):
        s, e, res = funcs[mangled]
        valu, salu, lanes, lanes_in_walk, pairs, node_loops, loop_mix = census(lines[s:e])
        ss, vs = spills.get(mangled, (-1, -1))
        in_walk = sum(1 for _, ch in pairs if any(h in node_loops for h in ch))
        print("%s | %d / %d / %d / %d / %d / %d | %d / %d | %d (%d) | %d (%d)" % (
            pretty[mangled], res.get("NumVgprs", -1), res.get("TotalNumSgprs", -1), vs, ss, res.get("ScratchSize", -1), res.get("Occupancy", -1),
            valu, salu, lanes, lanes_in_walk, len(pairs), in_walk))
        if a.all or HEADLINE.match(pretty[mangled]):
            for b, ch in pairs:
                where = " < ".join("%s%s" % (h, " [node128]" if h in node_loops else "") for h in ch) or "outside every loop"
                print("    pair in block %s: %s" % (b, where))
            for h in sorted(loop_mix):
                tot = loop_mix[h]
                print("    loop %s [node128] holds %d instructions, %d on the scalar side: %s" % (
                    h, sum(tot.values()), sum(tot[k] for k in SCALAR_SIDE), ", ".join("%s %d" % (k, tot[k]) for k in MIX_CLASSES)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
