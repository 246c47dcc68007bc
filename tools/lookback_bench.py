#!/usr/bin/env python3
"""Cost of mcamd_price_lookback on one box, from the library's own HIP events: medians of --reps calls per job, one
process alternating call by call between
    mcamd_price_lookback, fixed-strike call, discrete monitoring,
    mcamd_price_lookback, fixed-strike call, continuous monitoring,
    mcamd_price_barrier, DOWN_IN call, discrete monitoring (a kernel of the same shape that also runs to maturity),
all at --paths x --steps (10M x 252) on S0 = K = 100, B = 90, r = 0.1, v = 0.2, T = 1, in fp64 and in fp32.
Printed as ONE JSON line; no time is asserted anywhere.
    python3 tools/lookback_bench.py [--reps 7] [--out profiles/lookback_bench.json]     # on an MI355X
live_over_work is live_steps / work_steps of the continuous job: the share of lane-steps whose bridge extremum was
formed (q < Q); the kernel predicates it per lane, so the share says how much of that work was kept, not skipped."""
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
    ap.add_argument("--paths", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=252)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    base = dict(S0=100.0, K=100.0, B=90.0, r=0.1, v=0.2, T=1.0)
    opt = capi.make_option(**base)
    disc = capi.make_lookback(capi.LOOKBACK_FIXED, capi.PAYOFF_CALL, capi.MONITOR_DISCRETE)
    cont = capi.make_lookback(capi.LOOKBACK_FIXED, capi.PAYOFF_CALL, capi.MONITOR_CONTINUOUS)
    knock_in = capi.make_barrier(capi.BARRIER_DOWN_IN, capi.PAYOFF_CALL, capi.MONITOR_DISCRETE)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    out = {"tool": "lookback_bench", "n_paths": args.paths, "n_steps": args.steps, "reps": args.reps, **base, "jobs": []}
    for prec in (capi.F64, capi.F32):
        sim = capi.make_sim(args.paths, args.steps, prec, seed=1234)
        for call in (lambda: ctx.price_lookback(opt, sim, disc), lambda: ctx.price_lookback(opt, sim, cont),
                     lambda: ctx.price_barrier(opt, sim, knock_in)):
            call()   # warm-up: code objects, scratch
        t_d, t_c, t_b = [], [], []
        for _ in range(args.reps):
            d = ctx.price_lookback(opt, sim, disc)
            c = ctx.price_lookback(opt, sim, cont)
            b = ctx.price_barrier(opt, sim, knock_in)
            t_d.append(d.kernel_ms)
            t_c.append(c.kernel_ms)
            t_b.append(b.kernel_ms)
        steps = args.paths * args.steps
        out["jobs"].append({
            "precision": prec, "discrete_ms": round(med(t_d), 3), "continuous_ms": round(med(t_c), 3),
            "barrier_knock_in_ms": round(med(t_b), 3), "discrete_over_barrier": round(med(t_d) / med(t_b), 3),
            "continuous_over_barrier": round(med(t_c) / med(t_b), 3),
            "continuous_over_discrete": round(med(t_c) / med(t_d), 3),
            "live_over_work": round(c.live_steps / c.work_steps, 4),
            "work_over_full": round(c.work_steps / (64 * -(-args.paths // 64) * args.steps), 4),
            "discrete_path_steps_per_s": steps / (med(t_d) * 1e-3),
            "continuous_path_steps_per_s": steps / (med(t_c) * 1e-3),
            "discrete_price": d.price, "discrete_std_err": d.std_err,
            "continuous_price": c.price, "continuous_std_err": c.std_err,
            "closed_form_continuous": capi.lookback_price_f64(base["S0"], base["K"], base["T"], base["r"], base["v"],
                                                              capi.LOOKBACK_FIXED, capi.PAYOFF_CALL),
            "barrier_knock_in_price": b.price, "grid": d.grid, "barrier_grid": b.grid})
    out["build_id"] = capi.build_id()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
