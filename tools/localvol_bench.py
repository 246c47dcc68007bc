#!/usr/bin/env python3
"""Cost of mcamd_price_localvol on one box, from the library's own HIP events: medians of --reps calls per job, one
process alternating call by call between
    mcamd_price_localvol on a flat 1 x 2 surface (sigma = 0.2),  without a barrier and with a discrete DOWN_OUT call,
    mcamd_price_localvol on a 16 x 128 surface (the largest table: 2048 nodes), the same two jobs,
    mcamd_price_barrier, DOWN_OUT call, discrete monitoring, v = 0.2 (the job the flat surface restates),
all at --paths x --steps (10M x 252) on S0 = K = 100, B = 90, r = 0.1, q = 0, T = 1, in fp64 and in fp32.
Printed as ONE JSON line; no time is asserted anywhere.
    python3 tools/localvol_bench.py [--reps 7] [--out profiles/localvol_bench.json]     # on an MI355X
flat_over_barrier is what the per-step table lookup and the unscaled normals cost on the job both kernels price;
full_over_flat is what the size of the LDS table costs (occupancy: 32 KiB more per workgroup in fp64)."""
import argparse
import importlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--paths", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=252)
    ap.add_argument("--monitoring", choices=("discrete", "continuous"), default="discrete",
                    help="of the three DOWN_OUT jobs (continuous: the kernels with the bridge factor)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    base = dict(S0=100.0, K=100.0, B=90.0, r=0.1, v=0.2, T=1.0)
    opt = capi.make_option(**base)
    flat = ctx.localvol_surface((1, 2, -1.5, 1.5), [[0.2, 0.2]])
    xs = [-1.5 + 3.0 * k / 127 for k in range(128)]
    full = ctx.localvol_surface((16, 128, -1.5, 1.5),
                                [[(0.15 + 0.01 * j) * (1.0 + 0.5 * math.exp(-x)) / 1.5 for x in xs] for j in range(16)])
    plain = capi.make_localvol(capi.PAYOFF_CALL)
    mon = capi.MONITOR_CONTINUOUS if args.monitoring == "continuous" else capi.MONITOR_DISCRETE
    knock = capi.make_localvol(capi.PAYOFF_CALL, capi.BARRIER_DOWN_OUT, mon)
    bar = capi.make_barrier(capi.BARRIER_DOWN_OUT, capi.PAYOFF_CALL, mon)
    med = lambda xs_: sorted(xs_)[len(xs_) // 2]
    out = {"tool": "localvol_bench", "device": ctx.device_info().name.decode(), "n_paths": args.paths,
           "n_steps": args.steps, "reps": args.reps, "monitoring": args.monitoring, **base, "q": 0.0, "jobs": []}
    for prec in (capi.F64, capi.F32):
        sim = capi.make_sim(args.paths, args.steps, prec, seed=1234)
        calls = {
            "flat_european": lambda: ctx.price_localvol(opt, sim, plain, flat),
            "flat_down_out": lambda: ctx.price_localvol(opt, sim, knock, flat),
            "full_european": lambda: ctx.price_localvol(opt, sim, plain, full),
            "full_down_out": lambda: ctx.price_localvol(opt, sim, knock, full),
            "barrier_down_out": lambda: ctx.price_barrier(opt, sim, bar),
        }
        for call in calls.values():
            call()   # warm-up: code objects, scratch
        ms = {name: [] for name in calls}
        last = {}
        for _ in range(args.reps):
            for name, call in calls.items():
                last[name] = call()
                ms[name].append(last[name].kernel_ms)
        m = {name: med(v) for name, v in ms.items()}
        steps = args.paths * args.steps
        job = {"precision": prec, **{name + "_ms": round(v, 3) for name, v in m.items()},
               "flat_over_barrier": round(m["flat_down_out"] / m["barrier_down_out"], 3),
               "flat_european_over_barrier": round(m["flat_european"] / m["barrier_down_out"], 3),
               "full_over_flat_european": round(m["full_european"] / m["flat_european"], 3),
               "full_over_flat_down_out": round(m["full_down_out"] / m["flat_down_out"], 3),
               "flat_european_path_steps_per_s": steps / (m["flat_european"] * 1e-3),
               "work_over_full": round(last["flat_down_out"].work_steps / (64 * -(-args.paths // 64) * args.steps), 4),
               "flat_down_out_price": last["flat_down_out"].price, "barrier_down_out_price": last["barrier_down_out"].price,
               "flat_european_price": last["flat_european"].price,
               "bs_price": capi.bs_price_f64(base["S0"], base["K"], base["T"], base["r"], 0.0, base["v"]),
               "full_european_price": last["full_european"].price, "grid": last["flat_european"].grid}
        out["jobs"].append(job)
    out["build_id"] = capi.build_id()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    full.close()
    flat.close()
    ctx.close()


if __name__ == "__main__":
    main()
