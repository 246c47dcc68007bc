#!/usr/bin/env python3
"""Cost of mcamd_price_heston_barrier on one box, from the library's own HIP events: medians of --reps calls per job,
one process alternating call by call between
    mcamd_price_heston, European call on input F (the kernel the barrier kernels are built around: the baseline),
    mcamd_price_heston_barrier on the same input, down-and-out and down-and-in at B = 90, each monitored at the step
    ends and continuously,
at --paths x --steps (10M x 252), S0 = K = 100, r = 0.03, q = 0.01, T = 1, in fp64 and in fp32.  Beside each median:
the ratio to the European kernel and live_steps / work_steps (the share of the lane-steps the wavefronts ran that a
live path took: what lane compaction of knocked paths would start from).  Printed as ONE JSON line; no time is asserted
anywhere, and the spread between runs is not measured.
    python3 tools/heston_barrier_bench.py [--reps 7] [--out profiles/heston_barrier_bench.json]     # on an MI355X"""
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
    ap.add_argument("--level", type=float, default=90.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    base = dict(S0=100.0, K=100.0, r=0.03, v=0.2, T=1.0, B=args.level)
    model = dict(q=0.01, v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
    opt = capi.make_option(**base)
    heston = capi.make_heston(capi.PAYOFF_CALL, **model)
    down = args.level < base["S0"]
    kinds = {"out": capi.BARRIER_DOWN_OUT if down else capi.BARRIER_UP_OUT,
             "in": capi.BARRIER_DOWN_IN if down else capi.BARRIER_UP_IN}
    monitorings = {"discrete": capi.MONITOR_DISCRETE, "continuous": capi.MONITOR_CONTINUOUS}
    barriers = {f"{k}_{m}": capi.make_barrier(kind, capi.PAYOFF_CALL, mon)
                for k, kind in kinds.items() for m, mon in monitorings.items()}
    med = lambda xs: sorted(xs)[len(xs) // 2]
    out = {"tool": "heston_barrier_bench", "device": ctx.device_info().name.decode(), "n_paths": args.paths,
           "n_steps": args.steps, "reps": args.reps, **{k: base[k] for k in ("S0", "K", "r", "T", "B")}, **model,
           "side": "down" if down else "up", "run_to_run_spread": "not measured", "jobs": []}
    for prec in (capi.F64, capi.F32):
        sim = capi.make_sim(args.paths, args.steps, prec, seed=1234)
        calls = {"european": lambda: ctx.price_heston(opt, sim, heston)}
        for name, bar in barriers.items():
            calls[name] = lambda bar=bar: ctx.price_heston_barrier(opt, sim, heston, bar)
        for call in calls.values():
            call()   # warm-up: code objects, scratch
        ms = {name: [] for name in calls}
        last = {}
        for _ in range(args.reps):
            for name, call in calls.items():
                last[name] = call()
                ms[name].append(last[name].kernel_ms)
        m = {name: med(v) for name, v in ms.items()}
        job = {"precision": prec, "european_ms": round(m["european"], 3), "european_price": last["european"].price,
               "european_path_steps_per_s": args.paths * args.steps / (m["european"] * 1e-3), "grid": last["european"].grid}
        for name in barriers:
            r = last[name]
            job[name] = {"ms": round(m[name], 3), "over_european": round(m[name] / m["european"], 3),
                         "min_ms": round(min(ms[name]), 3), "max_ms": round(max(ms[name]), 3),
                         "live_over_work": round(r.live_steps / r.work_steps, 4),
                         "work_over_full": round(r.work_steps / last["european"].work_steps, 4),
                         "price": r.price, "std_err": r.std_err,
                         "truncated_share": r.truncated_steps / max(r.live_steps if name.startswith("out") else
                                                                    args.paths * args.steps, 1.0),
                         "mean_variance": r.mean_variance}
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
