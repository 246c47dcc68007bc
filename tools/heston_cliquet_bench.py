#!/usr/bin/env python3
"""Cost of mcamd_price_heston_cliquet on one box, from the library's own HIP events: medians of --reps calls per job, one
process alternating call by call between
    mcamd_price_heston, European call on input F (v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7): the walk alone,
    mcamd_price_heston_cliquet on the same input with monthly resets (reset_every = 21): the additive cliquet (SUM,
    local bounds -0.03 / 0.05), the compounding one (COMPOUND, same bounds) and the realized variance (VARIANCE),
    and the additive cliquet with a reset at every step (reset_every = 1): an exponential per step,
at --paths x --steps (10M x 252), r = 0.03, q = 0.01, T = 1, in fp64 and in fp32.  Printed as ONE JSON line; no time
is asserted anywhere.
    python3 tools/heston_cliquet_bench.py [--reps 7] [--out profiles/heston_cliquet_bench.json]     # on an MI355X
<job>_over_european is what the reset test, the period rule and the two extra record slots cost per job."""
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
    ap.add_argument("--reset-every", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    base = dict(S0=100.0, K=100.0, r=0.03, v=0.2, T=1.0)
    model = dict(q=0.01, v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
    floor, cap = -0.03, 0.05
    opt = capi.make_option(**base)
    heston = capi.make_heston(capi.PAYOFF_CALL, **model)
    every = args.reset_every
    jobs = {"sum": capi.make_cliquet(capi.CLIQUET_SUM, every, 1, floor, cap, q=model["q"]),
            "compound": capi.make_cliquet(capi.CLIQUET_COMPOUND, every, 1, floor, cap, q=model["q"]),
            "variance": capi.make_cliquet(capi.CLIQUET_VARIANCE, every, 1, q=model["q"]),
            "sum_every_step": capi.make_cliquet(capi.CLIQUET_SUM, 1, 1, floor, cap, q=model["q"])}
    periods = args.steps // every
    m_args = (base["T"], base["r"], model["q"], model["v0"], model["kappa"], model["theta"], model["xi"], model["rho"])
    closed = {"sum": capi.heston_cliquet_price(capi.CLIQUET_SUM, *m_args, periods, 1, floor, cap),
              "variance": capi.heston_cliquet_price(capi.CLIQUET_VARIANCE, *m_args, periods),
              "sum_every_step": capi.heston_cliquet_price(capi.CLIQUET_SUM, *m_args, args.steps, 1, floor, cap)}
    med = lambda xs: sorted(xs)[len(xs) // 2]
    out = {"tool": "heston_cliquet_bench", "device": ctx.device_info().name.decode(), "n_paths": args.paths,
           "n_steps": args.steps, "reset_every": every, "reps": args.reps, "r": base["r"], "T": base["T"], **model,
           "local_floor": floor, "local_cap": cap, "closed_form": closed, "jobs": []}
    for prec in (capi.F64, capi.F32):
        sim = capi.make_sim(args.paths, args.steps, prec, seed=1234)
        calls = {"european": lambda: ctx.price_heston(opt, sim, heston)}
        for name, cq in jobs.items():
            calls[name] = lambda cq=cq: ctx.price_heston_cliquet(opt, sim, heston, cq)
        for call in calls.values():
            call()   # warm-up: code objects, scratch
        ms = {name: [] for name in calls}
        last = {}
        for _ in range(args.reps):
            for name in jobs:   # each cliquet job beside a European call of its own, alternating
                for which in ("european", name):
                    last[which] = calls[which]()
                    ms[which].append(last[which].kernel_ms)
        m = {name: med(v) for name, v in ms.items()}
        out["jobs"].append({
            "precision": prec, **{name + "_ms": round(v, 3) for name, v in m.items()},
            **{name + "_over_european": round(m[name] / m["european"], 3) for name in jobs},
            **{name + "_path_steps_per_s": args.paths * args.steps / (v * 1e-3) for name, v in m.items()},
            **{name + "_price": last[name].price for name in calls},
            **{name + "_std_err": last[name].std_err for name in jobs},
            "truncated_share": last["sum"].truncated_steps / (args.paths * args.steps),
            "mean_variance": last["sum"].mean_variance, "grid": last["sum"].grid})
    out["build_id"] = capi.build_id()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
