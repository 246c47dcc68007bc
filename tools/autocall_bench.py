#!/usr/bin/env python3
"""Cost of mcamd_price_autocall on one box, from the library's own HIP events: medians of --reps calls per job after one
warm-up call each, one process alternating call by call, in fp64 and in fp32.  The job is a 3-asset quarterly 5-year
note: --paths x --steps (1M x 1260, 252 steps a year), an observation every 63 steps (20 dates), autocall level 1,
coupon 0.02 a date, knock-in at 0.6 monitored at every step or at maturity, on v_j = 0.15 + 0.05 j,
corr_jk = 0.6^|j - k|, r = 0.05, T = 5.  Beside it, in the same run, mcamd_price_basket's worst-of knock-in put of the
same assets, steps and level — the same step without the observation test and with no early exit — and the ratio.
Reports kernel ms and live_steps / work_steps (how full the wavefronts ran) and work_steps over the full count (how much
of the loop the early exit saved).  Printed as ONE JSON line; no time is asserted anywhere.
    python3 tools/autocall_bench.py [--reps 7] [--out profiles/autocall_bench.json]     # on an MI355X"""
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
    ap.add_argument("--paths", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=1260)
    ap.add_argument("--observe-every", type=int, default=63)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    r, T, d, ki_level = 0.05, 5.0, 3, 0.6
    med = lambda xs: sorted(xs)[len(xs) // 2]
    v = [0.15 + 0.05 * j for j in range(d)]
    corr = [[0.6 ** abs(j - k) for k in range(d)] for j in range(d)]
    full = 64 * -(-args.paths // 64) * args.steps

    out = {"tool": "autocall_bench", "paths": args.paths, "steps": args.steps, "observe_every": args.observe_every,
           "assets": d, "reps": args.reps, "r": r, "T": T, "jobs": []}
    for prec in (capi.F64, capi.F32):
        sim = capi.make_sim(args.paths, args.steps, prec, seed=1234)
        opt = capi.make_option(S0=0.0, v=0.0, K=0.0, r=r, T=T)
        calls = {}
        for name, ki in (("ki_every_step", capi.AUTOCALL_KI_EVERY_STEP), ("ki_at_maturity", capi.AUTOCALL_KI_AT_MATURITY)):
            note = capi.make_autocall(v, corr, args.observe_every, 1.0, 0.02, ki_level, ki)
            calls[name] = lambda a=note: ctx.price_autocall(opt, sim, a)
        worst = capi.make_basket([1.0] * d, v, [1.0] * d, corr, capi.BASKET_WORST_OF, capi.PAYOFF_PUT, capi.BASKET_DOWN_IN)
        calls["basket_knock_in_put"] = lambda: ctx.price_basket(capi.make_option(K=1.0, r=r, T=T, B=ki_level), sim, worst)
        for call in calls.values():
            call()   # warm-up: code objects, scratch
        times = {key: [] for key in calls}
        last = {}
        for _ in range(args.reps):
            for key, call in calls.items():
                last[key] = call()
                times[key].append(last[key].kernel_ms)
        job = {"precision": prec, "basket_knock_in_put_ms": round(med(times["basket_knock_in_put"]), 3)}
        for name in ("ki_every_step", "ki_at_maturity"):
            t, res = med(times[name]), last[name]
            job[name] = {
                "kernel_ms": round(t, 3), "price": res.price, "std_err": res.std_err,
                "called": res.n_called / args.paths, "mean_call_time": res.sum_t_call / max(res.n_called, 1),
                "knocked_in": res.n_knocked_in / args.paths,
                "live_over_work": round(res.live_steps / res.work_steps, 4),
                "work_over_full": round(res.work_steps / full, 4),
                "asset_steps_per_s": res.work_steps * d / (t * 1e-3),
                "over_basket_knock_in_put": round(t / med(times["basket_knock_in_put"]), 3), "grid": res.grid}
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
