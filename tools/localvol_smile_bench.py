#!/usr/bin/env python3
"""Cost of mcamd_price_localvol_smile on one box, from the library's own HIP events: medians of --reps calls per job,
one process alternating call by call between
    mcamd_price_localvol without a barrier (one strike, one expiry: the single call a smile replaces n_e n_K of),
    mcamd_price_localvol_smile at (n_e, n_K) = (1, 1), (12, 41) and (32, 64), the last expiry at n_steps, the others
    spread evenly below it, strikes from 50 to 200,
all at --paths x --steps (10M x 252) on a skewed 4 x 65 surface, S0 = 100, r = 0.1, q = 0.03, T = 1, in fp64 and fp32.
Printed as ONE JSON line; no time is asserted anywhere.
    python3 tools/localvol_smile_bench.py [--reps 7] [--out profiles/localvol_smile_bench.json]     # on an MI355X
smile_over_single is the path kernel of the smile over the single call's kernel; total_over_single takes the smile's
total (with the sum of the per-wavefront records); per_node divides that by n_e n_K: the share of a single call one node
of the smile costs."""
import argparse
import importlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 1), (12, 41), (32, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--paths", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=252)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    base = dict(S0=100.0, K=100.0, r=0.1, v=0.0, T=1.0)
    q = 0.03
    opt = capi.make_option(**base)
    xs = [-1.5 + 3.0 * k / 64 for k in range(65)]
    surface = ctx.localvol_surface((4, 65, -1.5, 1.5),
                                   [[(0.18 + 0.04 * j) * (1.0 + 0.5 * math.exp(-x)) / 1.5 for x in xs] for j in range(4)])
    plain = capi.make_localvol(capi.PAYOFF_CALL, q=q)
    med = lambda v: sorted(v)[len(v) // 2]
    smiles = {}
    for n_e, n_K in SHAPES:
        steps = [max(1, (m + 1) * args.steps // n_e) for m in range(n_e)]
        strikes = [100.0] if n_K == 1 else [50.0 + 150.0 * k / (n_K - 1) for k in range(n_K)]
        smiles[(n_e, n_K)] = (capi.make_smile(n_e, n_K, capi.PAYOFF_CALL, q), steps, strikes)
    out = {"tool": "localvol_smile_bench", "device": ctx.device_info().name.decode(), "n_paths": args.paths,
           "n_steps": args.steps, "reps": args.reps, "S0": 100.0, "r": 0.1, "q": q, "T": 1.0, "surface": "skew 4 x 65",
           "jobs": []}
    for prec in (capi.F64, capi.F32):
        sim = capi.make_sim(args.paths, args.steps, prec, seed=1234)
        calls = {"single": lambda: ctx.price_localvol(opt, sim, plain, surface)}
        for shape, (smile, steps, strikes) in smiles.items():
            calls[shape] = (lambda smile=smile, steps=steps, strikes=strikes:
                            ctx.price_localvol_smile(opt, sim, smile, steps, strikes, surface)[3])
        for call in calls.values():
            call()   # warm-up: code objects, scratch
        kernel, total, last = {name: [] for name in calls}, {name: [] for name in calls}, {}
        for _ in range(args.reps):
            for name, call in calls.items():
                last[name] = call()
                kernel[name].append(last[name].kernel_ms)
                total[name].append(last[name].total_ms)
        single = med(kernel["single"])
        job = {"precision": prec, "single_ms": round(single, 3), "single_grid": last["single"].grid, "smiles": []}
        for n_e, n_K in SHAPES:
            k_ms, t_ms = med(kernel[(n_e, n_K)]), med(total[(n_e, n_K)])
            job["smiles"].append({"n_expiries": n_e, "n_strikes": n_K, "kernel_ms": round(k_ms, 3),
                                  "total_ms": round(t_ms, 3), "grid": last[(n_e, n_K)].grid,
                                  "smile_over_single": round(k_ms / single, 3),
                                  "total_over_single": round(t_ms / single, 3),
                                  "per_node": round(t_ms / single / (n_e * n_K), 5),
                                  "last_node_price": last[(n_e, n_K)].price})
        job["single_price"] = last["single"].price
        out["jobs"].append(job)
    out["build_id"] = capi.build_id()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    surface.close()
    ctx.close()


if __name__ == "__main__":
    main()
