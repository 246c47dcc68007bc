#!/usr/bin/env python3
"""Cost of mcamd_price_asian on one box, from the library's own HIP events: medians of --reps calls per job, one
process alternating call by call between
    mcamd_price_asian, geometric average, fixed-strike call,
    mcamd_price_asian, arithmetic average, fixed-strike call,
    mcamd_price_asian, arithmetic average with the geometric control variate, fixed-strike call,
    mcamd_price_lookback, fixed-strike call, discrete monitoring (a kernel of the same shape: the yardstick),
all at --paths x --steps (10M x 252) on S0 = K = 100, r = 0.1, v = 0.2, T = 1, without the spot, in fp64 and in fp32.
Printed as ONE JSON line; no time is asserted anywhere.
    python3 tools/asian_bench.py [--reps 7] [--out profiles/asian_bench.json]     # on an MI355X
se_ratio is the plain arithmetic job's standard error over the controlled one's: what the control variate buys."""
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
    base = dict(S0=100.0, K=100.0, r=0.1, v=0.2, T=1.0)
    opt = capi.make_option(**base)
    geo = capi.make_asian(capi.ASIAN_GEOMETRIC, capi.ASIAN_FIXED, capi.PAYOFF_CALL)
    ari = capi.make_asian(capi.ASIAN_ARITHMETIC, capi.ASIAN_FIXED, capi.PAYOFF_CALL)
    cv = capi.make_asian(capi.ASIAN_ARITHMETIC, capi.ASIAN_FIXED, capi.PAYOFF_CALL, control=capi.ASIAN_CONTROL_GEOMETRIC)
    look = capi.make_lookback(capi.LOOKBACK_FIXED, capi.PAYOFF_CALL, capi.MONITOR_DISCRETE)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    out = {"tool": "asian_bench", "n_paths": args.paths, "n_steps": args.steps, "reps": args.reps, **base, "jobs": []}
    for prec in (capi.F64, capi.F32):
        sim = capi.make_sim(args.paths, args.steps, prec, seed=1234)
        calls = (lambda: ctx.price_asian(opt, sim, geo), lambda: ctx.price_asian(opt, sim, ari),
                 lambda: ctx.price_asian(opt, sim, cv), lambda: ctx.price_lookback(opt, sim, look))
        for call in calls:
            call()   # warm-up: code objects, scratch
        times = [[] for _ in calls]
        for _ in range(args.reps):
            last = [call() for call in calls]
            for t, res in zip(times, last):
                t.append(res.kernel_ms)
        g, a, c, lb = last
        t_g, t_a, t_c, t_l = (med(t) for t in times)
        steps = args.paths * args.steps
        out["jobs"].append({
            "precision": prec, "geometric_ms": round(t_g, 3), "arithmetic_ms": round(t_a, 3),
            "controlled_ms": round(t_c, 3), "lookback_discrete_ms": round(t_l, 3),
            "geometric_over_lookback": round(t_g / t_l, 3), "arithmetic_over_lookback": round(t_a / t_l, 3),
            "controlled_over_lookback": round(t_c / t_l, 3), "controlled_over_arithmetic": round(t_c / t_a, 3),
            "geometric_path_steps_per_s": steps / (t_g * 1e-3), "arithmetic_path_steps_per_s": steps / (t_a * 1e-3),
            "controlled_path_steps_per_s": steps / (t_c * 1e-3),
            "geometric_price": g.price, "geometric_std_err": g.std_err,
            "closed_form_geometric": capi.asian_geometric_price_f64(base["S0"], base["K"], base["T"], base["r"],
                                                                    base["v"], args.steps),
            "arithmetic_price": a.price, "arithmetic_std_err": a.std_err,
            "controlled_price": c.price, "controlled_std_err": c.std_err, "cv_beta": c.cv_beta, "cv_rho": c.cv_rho,
            "se_ratio": round(a.std_err / c.std_err, 2), "grid": g.grid, "lookback_grid": lb.grid})
    out["build_id"] = capi.build_id()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
