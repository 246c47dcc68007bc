#!/usr/bin/env python3
"""Digest of a `rocprofv3 --kernel-trace` run of bench.py for the time between consecutive pricing kernels:
    python3 tools/enqueue_trace_digest.py DIR_OR_kernel_trace.csv [--last 20]
Reads the newest *_kernel_trace.csv under DIR, keeps the price_kernel and final_reduce_kernel dispatches, and prints, for
the last N price_kernel dispatches in start order (bench.py's timed steps), each one's duration and the gap from its
predecessor's end to its own start (negative: it started while the predecessor was still running), then the medians, the
span from the first start to the last end, and final_reduce_kernel's times."""
import argparse, csv, glob, os, sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("src")
    ap.add_argument("--last", type=int, default=20)
    args = ap.parse_args()
    path = args.src
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
        if not found:
            print("no *kernel_trace.csv under", path, file=sys.stderr)
            return 1
        path = found[-1]
    price, reduce_ = [], []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            rec = (int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row.get("Queue_Id", "?"), name)
            if "price_kernel" in name:
                price.append(rec)
            elif "final_reduce_kernel" in name:
                reduce_.append(rec)
    price.sort()
    reduce_.sort()
    last = price[-args.last:]
    if len(last) < 2:
        print("fewer than two price_kernel dispatches in", path, file=sys.stderr)
        return 1
    med = lambda xs: sorted(xs)[len(xs) // 2]
    us = lambda ns: ns / 1e3
    print(f"{os.path.basename(path)}: {len(price)} price_kernel and {len(reduce_)} final_reduce_kernel dispatches; the last "
          f"{len(last)} price_kernel dispatches by start:")
    print("   #  queue      duration us   gap from predecessor's end us")
    gaps, durs = [], []
    for i, (s, e, q, _) in enumerate(last):
        durs.append(e - s)
        gap = s - last[i - 1][1] if i else None
        if gap is not None:
            gaps.append(gap)
        print(f"  {i:2d}  {q:>6s}  {us(e - s):12.2f}   " + ("" if gap is None else f"{us(gap):10.2f}"))
    span = last[-1][1] - last[0][0]
    print(f"kernel name: {last[-1][3]}")
    print(f"duration us: median {us(med(durs)):.2f}  min {us(min(durs)):.2f}  max {us(max(durs)):.2f}")
    print(f"gap us: median {us(med(gaps)):.2f}  min {us(min(gaps)):.2f}  max {us(max(gaps)):.2f}; "
          f"started before the predecessor ended: {sum(g < 0 for g in gaps)} of {len(gaps)}")
    print(f"first start to last end: {us(span):.2f} us = {us(span) / len(last):.2f} us per job; "
          f"sum of durations {us(sum(durs)):.2f} us")
    tail = [r for r in reduce_ if r[0] >= last[0][0]]
    if tail:
        d = [e - s for s, e, _, _ in tail]
        print(f"final_reduce_kernel after the first of them: {len(d)} dispatches, duration us median {us(med(d)):.2f}  "
              f"min {us(min(d)):.2f}  max {us(max(d)):.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
