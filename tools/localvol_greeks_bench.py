#!/usr/bin/env python3
"""Cost of mcamd_price_localvol_greeks on one box, from the library's own HIP events: kernel medians of --reps calls
per job, one process alternating call by call between
    mcamd_price_localvol without a barrier (the price alone: what every bump-and-reprice launch costs),
    mcamd_price_localvol_greeks plain (price, delta, vega, rho, rho_q),  + gamma (gamma_bump = 0.01, two more walks),
    + 8 vega buckets,  and both,
all at --paths x --steps (10M x 252) on the 4 x 65 skew surface on [-1.47, 1.53], S0 = K = 100, r = 0.1, q = 0.03,
T = 1, in fp64 and in fp32.  Printed as ONE JSON line; no time is asserted anywhere.
    python3 tools/localvol_greeks_bench.py [--reps 7] [--out profiles/localvol_greeks_bench.json]     # on an MI355X
<job>_over_price is what the tangents cost over the price alone; launches_replaced is the count of
mcamd_price_localvol launches a central bump-and-reprice needs for the same numbers: 2 (4 + B) — delta, vega, rho,
rho_q and B buckets — plus one for the price (gamma by a second difference reuses delta's two)."""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    base = dict(S0=100.0, K=100.0, r=0.1, v=0.0, T=1.0)
    q, eta, n_b = 0.03, 0.01, 8
    opt = capi.make_option(**base)
    xs = [-1.47 + 3.0 * k / 64 for k in range(65)]
    surface = ctx.localvol_surface((4, 65, -1.47, 1.53),
                                   [[(0.18 + 0.04 * j) * (1.0 + 0.5 * math.exp(-x)) / 1.5 for x in xs] for j in range(4)])
    G = capi.make_localvol_greeks_job
    jobs = {"plain": G(capi.PAYOFF_CALL, 0, q, 0.0), "gamma": G(capi.PAYOFF_CALL, 0, q, eta),
            "buckets": G(capi.PAYOFF_CALL, n_b, q, 0.0), "gamma_buckets": G(capi.PAYOFF_CALL, n_b, q, eta)}
    price_job = capi.make_localvol(capi.PAYOFF_CALL, q=q)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"tool": "localvol_greeks_bench", "device": ctx.device_info().name.decode(), "n_paths": args.paths,
           "n_steps": args.steps, "reps": args.reps, **base, "q": q, "gamma_bump": eta, "n_vega_buckets": n_b,
           "launches_replaced": {name: 2 * (4 + j.n_vega_buckets) + 1 for name, j in jobs.items()}, "jobs": []}
    for prec in (capi.F64, capi.F32):
        sim = capi.make_sim(args.paths, args.steps, prec, seed=1234)
        calls = {"price": lambda: ctx.price_localvol(opt, sim, price_job, surface)}
        for name, j in jobs.items():
            calls[name] = lambda j=j: ctx.price_localvol_greeks(opt, sim, j, surface)
        for call in calls.values():
            call()   # warm-up: code objects, scratch
        ms, last = {name: [] for name in calls}, {}
        for _ in range(args.reps):
            for name, call in calls.items():
                last[name] = call()
                ms[name].append(last[name].kernel_ms)
        m = {name: med(v) for name, v in ms.items()}
        g = last["gamma_buckets"]
        job = {"precision": prec, **{name + "_ms": round(v, 3) for name, v in m.items()},
               **{name + "_over_price": round(m[name] / m["price"], 3) for name in jobs},
               **{name + "_over_bump_and_reprice": round(m[name] / (out["launches_replaced"][name] * m["price"]), 4)
                  for name in jobs},
               "price": last["price"].price, "greeks_price": g.value[0], "delta": g.value[1], "gamma": g.value[2],
               "vega": g.value[3], "rho": g.value[4], "rho_q": g.value[5], "bucket_vega": list(g.bucket_value),
               "std_err": list(g.std_err), "grid": g.grid}
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
