#!/usr/bin/env python3
"""Compares the gfx950 machine code of two source trees kernel by kernel, without a GPU: for every kernel symbol of the
given kernel files the multiset of vector, LDS and memory opcodes (v_*, ds_*, global_*, flat_*, buffer_*) and the
compiler's resource figures (VGPRs, AGPRs, spilled registers, LDS and scratch bytes) must agree; scalar-instruction
order and the SGPR count may differ, and the SGPR counts are reported.
    python3 tools/isa_diff.py OTHER_TREE [FILE.hip ...]          # OTHER_TREE: a checkout of the commit to compare with
With --text before OTHER_TREE the whole device assembly of each file is compared line by line instead, without its
.file, .ident and comment lines and with the path hash in the name of the __hip_cuid_ object blanked: for a change that
must not reach the device code at all.
Exit status 1 when a kernel, or with --text a file, differs."""
import collections, importlib.util, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "monte-carlo-project-cuda_amd"
DEFAULT = ["localvol.hip", "localvol_smile.hip", "autocall_localvol.hip", "autocall_localvol_f32.hip", "barrier.hip",
           "basket.hip", "autocall.hip", "heston.hip", "heston_smile.hip", "heston_cliquet.hip", "heston_barrier.hip", "heston_greeks.hip", "smile.hip", "cliquet.hip", "localvol_greeks.hip",
           "lookback.hip", "asian.hip", "american.hip", "american_dual.hip", "greeks.hip"]
OPCODE = re.compile(r"^\s+((?:v|ds|global|flat|buffer)_[a-z0-9_]+)\b")
FIGURES = {"vgpr": ".vgpr_count", "agpr": ".agpr_count", "vgpr_spill": ".vgpr_spill_count",
           "sgpr_spill": ".sgpr_spill_count", "lds": ".group_segment_fixed_size", "scratch": ".private_segment_fixed_size",
           "sgpr": ".sgpr_count"}


def device_asm(tree, src):
    """the device assembly of one kernel file of one tree, compiled with that tree's flags"""
    spec = importlib.util.spec_from_file_location("build_" + str(abs(hash(tree))), os.path.join(tree, PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.check_call([build.hipcc(), *build._flags(), "-S", "--cuda-device-only", os.path.join(build.CSRC, src),
                               "-o", out], stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()


def text_of(tree, src):
    """the device assembly without what names the tree or the compiler (.file, .ident; the hash in the one-byte
    __hip_cuid_<hash> object, which hipcc forms from the source file's path) and without comment lines"""
    return [re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", l) for l in device_asm(tree, src).splitlines()
            if not l.lstrip().startswith((";", ".file", ".ident"))]


def kernels_of(tree, src):
    """{kernel symbol: (opcode multiset, figures)} of one kernel file of one tree; none where the tree has no such file"""
    if not os.path.exists(os.path.join(tree, PKG, "csrc", src)):
        return {}
    asm = device_asm(tree, src)
    ops, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = ops.setdefault(m.group(1), collections.Counter())
        elif line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            m = OPCODE.match(line)
            if m:
                cur[m.group(1)] += 1
    figures = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        block = "    .agpr_count:" + block
        name = re.search(r"^    \.name:\s+(\S+)", block, re.M).group(1)   # the kernel's, not an argument's
        figures[name] = {k: int(re.search(r"^\s+" + re.escape(v) + r":\s+(\d+)", block, re.M).group(1))
                         for k, v in FIGURES.items()}
    return {k: (ops[k], figures[k]) for k in figures}


def main():
    text = sys.argv[1:2] == ["--text"]
    argv = sys.argv[2:] if text else sys.argv[1:]
    other = os.path.abspath(argv[0])
    bad = 0
    for src in argv[1:] or DEFAULT:
        if text:
            a, b = text_of(other, src), text_of(ROOT, src)
            bad += a != b
            print(f"{src}: device assembly, {len(b)} lines without .file, .ident and comments: "
                  f"{'identical' if a == b else 'DIFFERS'}")
            continue
        a, b = kernels_of(other, src), kernels_of(ROOT, src)
        differ = [k for k in sorted(set(a) | set(b)) if k not in a or k not in b or a[k][0] != b[k][0] or
                  any(a[k][1][f] != b[k][1][f] for f in FIGURES if f != "sgpr")]
        both = sorted(set(a) & set(b))
        moved = [(a[k][1]["sgpr"], b[k][1]["sgpr"]) for k in both if a[k][1]["sgpr"] != b[k][1]["sgpr"]]
        sg = both or sorted(b)   # a file of this tree alone: its own range
        print(f"{src}: {len(b)} kernels, {sum(sum(v[0].values()) for v in b.values())} counted instructions, "
              f"{len(differ)} differ; SGPRs {min(b[k][1]['sgpr'] for k in sg)}..{max(b[k][1]['sgpr'] for k in sg)}, "
              f"changed in {len(moved)} kernels {sorted(set(moved))}")
        for k in differ:
            bad += 1
            if k in a and k in b:
                d = {op: (a[k][0][op], b[k][0][op]) for op in set(a[k][0]) | set(b[k][0]) if a[k][0][op] != b[k][0][op]}
                f = {f: (a[k][1][f], b[k][1][f]) for f in FIGURES if a[k][1][f] != b[k][1][f]}
                print(f"  DIFFERS {k}: opcodes (other, this) {d}; figures {f}")
            else:
                print(f"  DIFFERS {k}: only in {'the other tree' if k in a else 'this tree'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
