#!/usr/bin/env python3
"""Cost of mcamd_price_basket on one box, from the library's own HIP events: medians of --reps calls per job after one
warm-up call each, one process alternating call by call, for d in {1, 2, 4, 8} in fp64 and in fp32, in two shapes:
    terminal:   arithmetic call, w_j = 1 / d, K = 100, at --terminal-paths x 1 step (10M x 1),
    monitored:  worst-of knock-in put on the performances, K = 1, B = 0.8, at --paths x --steps (1M x 252),
on S0_j = 80 + 10 j, v_j = 0.15 + 0.05 j, corr_jk = 0.6^|j - k|, r = 0.05, T = 1.  Beside the d = 1 figures, in the same
run, mcamd_price_barrier's discrete DOWN_IN put of the monitored shape on the first asset alone (S0 = K = 80, B = 64),
with the ratio.  Printed as ONE JSON line; no time is asserted anywhere.
    python3 tools/basket_bench.py [--reps 7] [--out profiles/basket_bench.json]     # on an MI355X"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--terminal-paths", type=int, default=10_000_000)
    ap.add_argument("--paths", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=252)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    r, T = 0.05, 1.0
    med = lambda xs: sorted(xs)[len(xs) // 2]

    def assets(d):
        S0 = [80.0 + 10.0 * j for j in range(d)]
        v = [0.15 + 0.05 * j for j in range(d)]
        return S0, v, [[0.6 ** abs(j - k) for k in range(d)] for j in range(d)]

    out = {"tool": "basket_bench", "terminal_paths": args.terminal_paths, "paths": args.paths, "steps": args.steps,
           "reps": args.reps, "r": r, "T": T, "jobs": []}
    for prec in (capi.F64, capi.F32):
        term_sim = capi.make_sim(args.terminal_paths, 1, prec, seed=1234)
        mon_sim = capi.make_sim(args.paths, args.steps, prec, seed=1234)
        calls = {}
        for d in (1, 2, 4, 8):
            S0, v, corr = assets(d)
            arith = capi.make_basket(S0, v, [1.0 / d] * d, corr, capi.BASKET_ARITHMETIC, capi.PAYOFF_CALL)
            worst = capi.make_basket(S0, v, [1.0 / s for s in S0], corr, capi.BASKET_WORST_OF, capi.PAYOFF_PUT,
                                     capi.BASKET_DOWN_IN)
            calls["terminal", d] = (lambda b=arith: ctx.price_basket(capi.make_option(K=100.0, r=r, T=T), term_sim, b))
            calls["monitored", d] = (lambda b=worst: ctx.price_basket(capi.make_option(K=1.0, r=r, T=T, B=0.8), mon_sim, b))
        single = capi.make_option(S0=80.0, K=80.0, B=64.0, r=r, v=0.15, T=T)
        knock_in = capi.make_barrier(capi.BARRIER_DOWN_IN, capi.PAYOFF_PUT, capi.MONITOR_DISCRETE)
        calls["barrier", 1] = lambda: ctx.price_barrier(single, mon_sim, knock_in)
        for call in calls.values():
            call()   # warm-up: code objects, scratch
        times = {key: [] for key in calls}
        last = {}
        for _ in range(args.reps):
            for key, call in calls.items():
                last[key] = call()
                times[key].append(last[key].kernel_ms)
        job = {"precision": prec, "barrier_knock_in_ms": round(med(times["barrier", 1]), 3),
               "barrier_knock_in_price": last["barrier", 1].price}
        for d in (1, 2, 4, 8):
            t, m = med(times["terminal", d]), med(times["monitored", d])
            job[f"d{d}"] = {
                "terminal_ms": round(t, 3), "monitored_ms": round(m, 3),
                "terminal_paths_per_s": args.terminal_paths / (t * 1e-3),
                "monitored_asset_steps_per_s": args.paths * args.steps * d / (m * 1e-3),
                "terminal_price": last["terminal", d].price, "terminal_std_err": last["terminal", d].std_err,
                "monitored_price": last["monitored", d].price, "monitored_std_err": last["monitored", d].std_err,
                "live_over_work": round(last["monitored", d].live_steps / last["monitored", d].work_steps, 4),
                "grid": last["monitored", d].grid}
        job["d1_monitored_over_barrier"] = round(med(times["monitored", 1]) / med(times["barrier", 1]), 3)
        for d in (2, 4, 8):
            job[f"d{d}_monitored_over_d1"] = round(med(times["monitored", d]) / med(times["monitored", 1]), 3)
            job[f"d{d}_terminal_over_d1"] = round(med(times["terminal", d]) / med(times["terminal", 1]), 3)
        out["jobs"].append(job)
    out["build_id"] = capi.build_id()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
