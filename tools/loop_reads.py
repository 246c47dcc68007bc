#!/usr/bin/env python3
"""The fp64 pair-sum step loops as compiled, from the gfx950 ISA and without a GPU: for each kernel, the loop's VALU
instructions and nominal issue cycles (tools/count_valu_slots.py), the kernel's VGPRs, scratch and LDS bytes, how many of
Philox's multiplies carry their constant as first source, and for every ds_read_b128 of the loop the number of VALU
instructions in program order between the read and the s_waitcnt lgkmcnt that covers it (LDS returns in order, so a wait
for lgkmcnt(N) covers all but the N youngest reads; the loop is walked twice, so a read waited for in the next iteration
is measured too).
    python3 tools/loop_reads.py [--against OTHER_TREE]
With --against, the loop's opcode multiset is compared with the same loop of a checkout of another commit."""
import argparse, collections, importlib.util, json, os, re, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"price_f64.hip": ["_ZN5mcamd12price_kernelIdLb0ELb1ELi%dEEE" % vr for vr in range(4)],
           "greeks.hip": ["_ZN5mcamd22greeks_pathwise_kernelIdEE"]}


# v_mad_u64_u32 with a scalar register as FIRST source; the compiler's own form has it second (the first-source form was
# tried for Philox's multiplies and left out: profiles/pairsum_skew_ab.txt)
CONST_FIRST = re.compile(r"v_mad_u64_u32 v\[\d+:\d+\], s\[\d+:\d+\], s\d+, v\d+, 0")


def slots_module(tree=ROOT):
    spec = importlib.util.spec_from_file_location("count_valu_slots_" + str(abs(hash(tree))),
                                                  os.path.join(tree, "tools", "count_valu_slots.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def read_to_wait(ins):
    """VALU instructions between each ds_read_b128 of the loop body and the wait that covers it."""
    pending, dist, valu = [], [], 0
    for rnd in range(2):
        for line in ins:
            op = line.split()[0]
            if op.startswith("v_"):
                valu += 1
            elif op.startswith("ds_read"):
                pending.append((valu, rnd))
            elif op == "s_waitcnt" and "lgkmcnt" in line:
                left = int(re.search(r"lgkmcnt\((\d+)\)", line).group(1))
                while len(pending) > left:
                    at, issued_in = pending.pop(0)
                    if issued_in == 0:
                        dist.append(valu - at)
    return dist, sum(1 for _, r in pending if r == 0)


def figures(asm, symbol):
    block = re.search(r"\.amdhsa_kernel %s\w*\n.*?\.end_amdhsa_kernel" % re.escape(symbol), asm, re.S).group(0)
    get = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, block).group(1))
    return {"vgpr": get("next_free_vgpr"), "scratch": get("private_segment_fixed_size"), "lds": get("group_segment_fixed_size")}


def digest(tree=ROOT):
    """{kernel symbol: figures, loop counts, read-to-wait distances and the loop's opcode multiset}"""
    c = slots_module(tree)
    bmod = c.build_module()
    flags = [f for f in bmod._flags() if f != "-fPIC"]
    out = {}
    for src, symbols in KERNELS.items():
        asm = c.asm_of(src, bmod.hipcc(), flags)
        for sym in symbols:
            ins = c.step_loop(asm, sym)
            dist, never = read_to_wait(ins)
            out[sym] = dict(figures(asm, sym), valu=sum(1 for l in ins if l.startswith("v_")),
                            issue_cycles=sum(c.line_cycles(l) for l in ins), reads=sum(1 for l in ins if l.startswith("ds_read")),
                            valu_between_read_and_wait=dist, reads_never_waited_for=never,
                            philox_mads_constant_first=sum(1 for l in ins if CONST_FIRST.match(l)),
                            opcodes=dict(collections.Counter(l.split()[0] for l in ins if l.startswith(("v_", "ds_")))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", default=None, help="a checkout of the commit to compare the loops' opcodes with")
    args = ap.parse_args()
    here = digest()
    other = digest(os.path.abspath(args.against)) if args.against else {}
    for sym, d in here.items():
        row = {k: v for k, v in d.items() if k != "opcodes"}
        if sym in other:
            a, b = other[sym]["opcodes"], d["opcodes"]
            row["opcodes_other_this"] = {op: (a.get(op, 0), b.get(op, 0)) for op in sorted(set(a) | set(b)) if a.get(op, 0) != b.get(op, 0)}
            row["other"] = {k: v for k, v in other[sym].items() if k != "opcodes"}
        print(json.dumps({"kernel": sym, **row}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
