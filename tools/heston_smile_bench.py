#!/usr/bin/env python3
"""Cost of mcamd_price_heston_smile on one box, from the library's own HIP events: medians of --reps calls per job, one
process alternating call by call between
    mcamd_price_heston, one European call at K = 100 on the same sim (the paths the smile walks, one strike, one expiry),
    mcamd_price_heston_smile, calls at --expiries evenly spaced expiry steps x --strikes strikes (12 monthly x 21),
on input F (v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7) at --paths x --steps (1M x 252), S0 = 100, r = 0.03,
q = 0.01, T = 1, in fp64 and in fp32.  Printed as ONE JSON line; no time is asserted anywhere.
    python3 tools/heston_smile_bench.py [--reps 7] [--out profiles/heston_smile_bench.json]     # on an MI355X
smile_over_single is the price of the strike phase and of the expiry tests: the smile call's path kernel over one
mcamd_price_heston kernel.  nodes_over_smile is what the call buys: n_e n_K single prices over one smile call.
The spread is (max - min) / median of each job's --reps kernel times."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--paths", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=252)
    ap.add_argument("--expiries", type=int, default=12)
    ap.add_argument("--strikes", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    base = dict(S0=100.0, K=100.0, r=0.03, v=0.2, T=1.0)
    model = dict(q=0.01, v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
    opt = capi.make_option(**base)
    heston = capi.make_heston(capi.PAYOFF_CALL, **model)
    steps = [args.steps * (m + 1) // args.expiries for m in range(args.expiries)]
    strikes = [float(k) for k in np.linspace(70.0, 130.0, args.strikes)]
    nodes = len(steps) * len(strikes)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    spread = lambda xs: (max(xs) - min(xs)) / med(xs)
    out = {"tool": "heston_smile_bench", "device": ctx.device_info().name.decode(), "n_paths": args.paths,
           "n_steps": args.steps, "reps": args.reps, "expiry_steps": steps, "strikes": strikes,
           **{k: base[k] for k in ("S0", "r", "T")}, **model, "jobs": []}
    for prec in (capi.F64, capi.F32):
        sim = capi.make_sim(args.paths, args.steps, prec, seed=1234)
        calls = {"single": lambda: ctx.price_heston(opt, sim, heston),
                 "smile": lambda: ctx.price_heston_smile(opt, sim, heston, steps, strikes)[3]}
        for call in calls.values():
            call()   # warm-up: code objects, scratch
        ms = {name: [] for name in calls}
        last = {}
        for _ in range(args.reps):
            for name, call in calls.items():
                last[name] = call()
                ms[name].append(last[name].kernel_ms)
        m = {name: med(v) for name, v in ms.items()}
        out["jobs"].append({
            "precision": prec, **{name + "_ms": round(v, 3) for name, v in m.items()},
            **{name + "_spread": round(spread(v), 3) for name, v in ms.items()},
            "smile_total_ms": round(last["smile"].total_ms, 3),
            "smile_over_single": round(m["smile"] / m["single"], 3),
            "nodes_over_smile": round(nodes * m["single"] / m["smile"], 1),
            "single_price": last["single"].price, "smile_last_node_price": last["smile"].price,
            "single_grid": last["single"].grid, "smile_grid": last["smile"].grid})
    out["build_id"] = capi.build_id()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
