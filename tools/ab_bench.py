#!/usr/bin/env python3
"""Same-box A/B of two builds of the library on one of the bench tools: the tool runs in alternating fresh processes
(A, B, A, B, ...), each loading ONE library (MCAMD_LIB), and every time the tool's JSON line reports (a key ending in
"_ms", per precision) is gathered per library.  Printed per time: both medians, library A's own min - max spread over
its rounds, and whether B's median is no slower than A's by more than that spread.
    python3 tools/ab_bench.py [--rounds 3] LIB_A LIB_B -- tools/localvol_bench.py [its arguments]     # on an MI355X"""
import argparse, json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def times(node, prefix=""):
    """{dotted key: ms} of every time in a bench tool's JSON line"""
    out = {}
    if isinstance(node, dict):
        tag = f"f{node['precision']}." if "precision" in node else ""
        for k, v in node.items():
            if isinstance(v, (dict, list)):
                out.update(times(v, prefix + tag + (k + "." if isinstance(v, dict) else "")))
            elif k.endswith("_ms") and isinstance(v, (int, float)):
                out[prefix + tag + k] = float(v)
    elif isinstance(node, list):
        for i, v in enumerate(node):   # a list of precisions names its entries itself; any other is numbered
            out.update(times(v, prefix if isinstance(v, dict) and "precision" in v else f"{prefix}{i}."))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("lib_a")
    ap.add_argument("lib_b")
    ap.add_argument("bench", nargs="+", help="the bench tool and its arguments, after --")
    args = ap.parse_args()
    libs = [os.path.abspath(args.lib_a), os.path.abspath(args.lib_b)]
    runs, ids = {lib: [] for lib in libs}, {}
    for _ in range(args.rounds):
        for lib in libs:
            o = subprocess.run([sys.executable, *args.bench], env=dict(os.environ, MCAMD_LIB=lib), cwd=ROOT,
                               capture_output=True, text=True)
            line = [l for l in o.stdout.splitlines() if l.startswith("{")]
            if o.returncode or not line:
                print("bench failed for", lib, o.stderr[-2000:], file=sys.stderr)
                return 1
            doc = json.loads(line[-1])
            ids[lib] = doc.get("build_id")
            runs[lib].append(times(doc))
    med = lambda xs: sorted(xs)[len(xs) // 2]
    ok = True
    for key in runs[libs[0]][0]:
        a, b = [r[key] for r in runs[libs[0]]], [r[key] for r in runs[libs[1]]]
        spread = max(a) - min(a)
        passed = med(b) - med(a) <= spread
        ok = ok and passed
        print(json.dumps({"bench": " ".join(args.bench), "time": key, "a_median": med(a), "b_median": med(b),
                          "a_spread": round(spread, 4), "b_no_slower_within_a_spread": passed, "a": a, "b": b}))
    print(json.dumps({"build_ids": {"a": ids[libs[0]], "b": ids[libs[1]]}, "rounds": args.rounds, "all_within_spread": ok}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
