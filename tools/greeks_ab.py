#!/usr/bin/env python3
"""Same-box cost of the in-kernel Greeks: mcamd_price_greeks against mcamd_price_paths on the same jobs, alternating
call by call (A, B, A, B, ...), each timed with the library's own HIP events (kernel_ms); medians are printed as one
JSON line per job.
    python3 tools/greeks_ab.py [--reps 21]          # on an MI355X
Jobs: 10M x 252 window-less, fp64 and fp32, pathwise; 1M x 100 with the reference's bullet window (B = 120, P1 = 10,
P2 = 50), likelihood ratio — at 1M paths mcamd_price_paths also runs one path per thread, so the loops compare like
for like."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    plain, bullet = capi.make_option(), capi.make_option(B=120.0, P1=10, P2=50, use_window=1)
    jobs = [("european f64 10M x 252 pathwise", plain, (10_000_000, 252, capi.F64), capi.GREEKS_PATHWISE),
            ("european f32 10M x 252 pathwise", plain, (10_000_000, 252, capi.F32), capi.GREEKS_PATHWISE),
            ("bullet f64 1M x 100 likelihood ratio", bullet, (1_000_000, 100, capi.F64), capi.GREEKS_LIKELIHOOD_RATIO),
            ("bullet f32 1M x 100 likelihood ratio", bullet, (1_000_000, 100, capi.F32), capi.GREEKS_LIKELIHOOD_RATIO)]
    med = lambda xs: sorted(xs)[len(xs) // 2]
    for _ in range(10):   # warm-up: clocks, code objects, scratch buffers
        ctx.price_paths(plain, capi.make_sim(10_000_000, 252, capi.F64, seed=1))
        ctx.price_greeks(plain, capi.make_sim(10_000_000, 252, capi.F64, seed=1))
    for name, opt, (n, steps, prec), method in jobs:
        price_ms, greeks_ms = [], []
        for r in range(args.reps):
            sim = capi.make_sim(n, steps, prec, seed=100 + r)
            price_ms.append(ctx.price_paths(opt, sim).kernel_ms)
            g = ctx.price_greeks(opt, sim, method)
            greeks_ms.append(g.kernel_ms)
        a, b = med(price_ms), med(greeks_ms)
        print(json.dumps({"job": name, "price_paths_ms": round(a, 4), "price_greeks_ms": round(b, 4),
                          "ratio": round(b / a, 4), "greeks_grid": g.grid, "reps": args.reps,
                          "build_id": capi.build_id()}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
