#!/usr/bin/env python3
"""Cost of mcamd_price_heston_greeks on one box, from the library's own HIP events: medians of --reps calls per job, one
process alternating call by call between
    mcamd_price_heston on input F (v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7): ONE call of the pricer, whose
        kernel this change does not touch,
    mcamd_price_heston_greeks with P = 0 (price, delta, gamma, rho, rho_q from the base walk alone),
    mcamd_price_heston_greeks with P = 5 (all five parameter bumps: eleven walks on shared draws),
at --paths x --steps (10M x 252), S0 = K = 100, r = 0.03, q = 0.01, T = 1, gamma_eta = 0.01, bumps 0.005 (v0, theta) and
0.05 (kappa, xi, rho), in fp64 and in fp32.  Each Greeks job is reported as a ratio to ONE mcamd_price_heston call and
to the 1 + 2 P such calls it replaces.  --runs > 1 repeats the whole measurement in the same process and reports the
spread of the medians between runs; with the default of one run the spread is not measured, and the line says so.
Printed as ONE JSON line; no time is asserted anywhere.
    python3 tools/heston_greeks_bench.py [--reps 7] [--runs 1] [--out profiles/heston_greeks_bench.json]   # on an MI355X"""
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
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--paths", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=252)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("monte-carlo-project-cuda_amd")
    capi, hg = pkg.capi, pkg.heston_greeks
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    base = dict(S0=100.0, K=100.0, r=0.03, v=0.2, T=1.0)
    model = dict(q=0.01, v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
    bumps = dict(v0=0.005, kappa=0.05, theta=0.005, xi=0.05, rho=0.05)
    eta = 0.01
    opt = capi.make_option(**base)
    heston = capi.make_heston(capi.PAYOFF_CALL, **model)
    jobs = {0: hg.make_job(eta), 5: hg.make_job(eta, **bumps)}
    med = lambda xs: sorted(xs)[len(xs) // 2]
    out = {"tool": "heston_greeks_bench", "device": ctx.device_info().name.decode(), "n_paths": args.paths,
           "n_steps": args.steps, "reps": args.reps, "runs": args.runs, **{k: base[k] for k in ("S0", "K", "r", "T")},
           **model, "gamma_eta": eta, "bumps": bumps, "jobs": []}
    for prec in (capi.F64, capi.F32):
        sim = capi.make_sim(args.paths, args.steps, prec, seed=1234)
        calls = {"heston": lambda: ctx.price_heston(opt, sim, heston),
                 "greeks_p0": lambda: ctx.price_heston_greeks(opt, sim, heston, jobs[0]),
                 "greeks_p5": lambda: ctx.price_heston_greeks(opt, sim, heston, jobs[5])}
        for call in calls.values():
            call()   # warm-up: code objects, scratch
        medians = {name: [] for name in calls}
        last = {}
        for _ in range(args.runs):
            ms = {name: [] for name in calls}
            for _ in range(args.reps):
                for name, call in calls.items():
                    last[name] = call()
                    ms[name].append(last[name].kernel_ms)
            for name, v in ms.items():
                medians[name].append(med(v))
        m = {name: med(v) for name, v in medians.items()}
        job = {"precision": prec, **{name + "_ms": round(v, 3) for name, v in m.items()}}
        for P, name in ((0, "greeks_p0"), (5, "greeks_p5")):
            job[name + "_over_one_heston_call"] = round(m[name] / m["heston"], 3)
            job[name + "_over_the_calls_it_replaces"] = round(m[name] / ((1 + 2 * P) * m["heston"]), 3)
            job[name + "_calls_replaced"] = 1 + 2 * P
        job["spread_between_runs"] = ({name: round((max(v) - min(v)) / m[name], 4) for name, v in medians.items()}
                                      if args.runs > 1 else "not measured: one run")
        job["heston_price"] = last["heston"].price
        job["greeks_p5"] = {k: [round(x, 6) for x in v] for k, v in last["greeks_p5"].as_dict().items()}
        job["closed_form"] = [round(x, 6) for x in hg.greeks_closed_form(
            base["S0"], base["K"], base["T"], base["r"], model["q"], model["v0"], model["kappa"], model["theta"],
            model["xi"], model["rho"], capi.PAYOFF_CALL, eta, [bumps[p] for p in hg.PARAMS])]
        job["grid"] = last["greeks_p5"].grid
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
