#!/usr/bin/env python3
"""Cost of mcamd_price_barrier on one box, from the library's own HIP events: medians of --reps calls per job, one
process alternating call by call between
    mcamd_price_barrier, DOWN_OUT call, discrete monitoring,
    mcamd_price_barrier, DOWN_OUT call, continuous monitoring,
    mcamd_price_paths with use_window = 1, P1 = P2 = 0 (the bullet job that pays the same discrete samples),
all at --paths x --steps (10M x 252) on S0 = K = 100, B = 90, r = 0.1, v = 0.2, T = 1, in fp64 and in fp32.
Printed as ONE JSON line; no time is asserted anywhere.
    python3 tools/barrier_bench.py [--reps 7] [--out profiles/barrier_bench.json]     # on an MI355X
live_over_work is live_steps / work_steps of the knock-out: how full its wavefronts ran (the bullet job of this size
runs the lane-compacting kernel; the barrier kernel does not compact)."""
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
    bullet = capi.make_option(**base, P1=0, P2=0, use_window=1)
    disc = capi.make_barrier(capi.BARRIER_DOWN_OUT, capi.PAYOFF_CALL, capi.MONITOR_DISCRETE)
    cont = capi.make_barrier(capi.BARRIER_DOWN_OUT, capi.PAYOFF_CALL, capi.MONITOR_CONTINUOUS)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    out = {"tool": "barrier_bench", "n_paths": args.paths, "n_steps": args.steps, "reps": args.reps, **base, "jobs": []}
    for prec in (capi.F64, capi.F32):
        sim = capi.make_sim(args.paths, args.steps, prec, seed=1234)
        for call in (lambda: ctx.price_barrier(opt, sim, disc), lambda: ctx.price_barrier(opt, sim, cont),
                     lambda: ctx.price_paths(bullet, sim)):
            call()   # warm-up: code objects, scratch
        t_d, t_c, t_b = [], [], []
        for _ in range(args.reps):
            d = ctx.price_barrier(opt, sim, disc)
            c = ctx.price_barrier(opt, sim, cont)
            b = ctx.price_paths(bullet, sim)
            t_d.append(d.kernel_ms)
            t_c.append(c.kernel_ms)
            t_b.append(b.kernel_ms)
        steps = args.paths * args.steps
        out["jobs"].append({
            "precision": prec, "discrete_ms": round(med(t_d), 3), "continuous_ms": round(med(t_c), 3),
            "bullet_ms": round(med(t_b), 3), "discrete_over_bullet": round(med(t_d) / med(t_b), 3),
            "continuous_over_discrete": round(med(t_c) / med(t_d), 3),
            "live_over_work": round(d.live_steps / d.work_steps, 4),
            "live_over_work_continuous": round(c.live_steps / c.work_steps, 4),
            "work_over_full": round(d.work_steps / (64 * -(-args.paths // 64) * args.steps), 4),
            "discrete_path_steps_per_s": steps / (med(t_d) * 1e-3), "bullet_path_steps_per_s": steps / (med(t_b) * 1e-3),
            "discrete_price": d.price, "discrete_std_err": d.std_err, "bullet_price": b.price,
            "continuous_price": c.price, "continuous_std_err": c.std_err,
            "closed_form_continuous": capi.barrier_price_f64(base["S0"], base["K"], base["B"], base["T"], base["r"],
                                                             base["v"], capi.BARRIER_DOWN_OUT, capi.PAYOFF_CALL),
            "grid": d.grid, "bullet_grid": b.grid})
    out["build_id"] = capi.build_id()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
