#!/usr/bin/env python3
"""Cost of mcamd_american_upper_bound on one box: the store of the outer paths, the continuation kernel and the scan,
from the library's own HIP events, medians of --reps calls per job, alternating call by call with
mcamd_price_american on the same option and with the product-form European pricer (mcamd_price_paths,
MCAMD_FLAG_PRODUCT_FORM) as the yardstick of a path-step.  Printed as ONE JSON line.
    python3 tools/american_dual_bench.py [--reps 7] [--out profiles/american_dual_bench.json]     # on an MI355X
Jobs: the Bermudan put of Longstaff-Schwartz (S0 = 36, K = 40, r = 0.06, v = 0.2, T = 1), 50 dates of one step, rule
fitted on 200 000 paths, 4096 outer paths x 256 continuation paths per point, fp64 and fp32.  Path-steps per second
of the continuation kernel count the steps its wavefronts ran (work_steps: idle lanes included) and, beside that, the
steps of paths that had not stopped yet (live_steps)."""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    opt = capi.make_option(S0=36.0, K=40.0, r=0.06, v=0.2, T=1.0)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    n_steps, k, n_outer, n_inner, n_euro = 50, 1, 4096, 256, 10_000_000
    out = {"tool": "american_dual_bench", "n_train": 200_000, "n_outer": n_outer, "n_inner": n_inner,
           "n_steps": n_steps, "k": k, "reps": args.reps, "jobs": []}
    for prec in (capi.F64, capi.F32):
        am = capi.make_american(exercise_every=k, n_train=200_000, train_seed=11)
        low_sim = capi.make_sim(2_000_000, n_steps, prec, seed=12)
        low_work = torch.empty(capi.american_workspace_bytes(am, low_sim), dtype=torch.uint8, device="cuda")
        dual = capi.make_american_dual(n_inner=n_inner, inner_seed=14)
        sim = capi.make_sim(n_outer, n_steps, prec, seed=13)
        work = torch.empty(capi.american_dual_workspace_bytes(am, sim, dual), dtype=torch.uint8, device="cuda")
        euro = capi.make_sim(n_euro, n_steps, prec, seed=12, flags=capi.FLAG_PRODUCT_FORM)
        low, coeffs = ctx.price_american(opt, low_sim, am, low_work, coeffs=True)   # warm-up: code objects, scratch
        ctx.american_upper_bound(opt, sim, am, dual, coeffs, work)
        ctx.price_paths(opt, euro)
        outer, inner, scan, total, lower, eu = [], [], [], [], [], []
        for _ in range(args.reps):
            r = ctx.american_upper_bound(opt, sim, am, dual, coeffs, work)
            outer.append(r.outer_ms)
            inner.append(r.inner_ms)
            scan.append(r.scan_ms)
            total.append(r.total_ms)
            lower.append(ctx.price_american(opt, low_sim, am, low_work).total_ms)
            eu.append(ctx.price_paths(opt, euro).kernel_ms)
        out["jobs"].append({
            "precision": prec, "M": n_steps // k, "outer_ms": round(med(outer), 3), "inner_ms": round(med(inner), 3),
            "scan_ms": round(med(scan), 3), "total_ms": round(med(total), 3),
            "price_american_total_ms": round(med(lower), 3), "european_product_form_ms": round(med(eu), 3),
            "cont_work_steps_per_s": r.work_steps / (med(inner) * 1e-3),
            "cont_live_steps_per_s": r.live_steps / (med(inner) * 1e-3),
            "european_steps_per_s": n_euro * n_steps / (med(eu) * 1e-3),
            "live_over_work": round(r.live_steps / r.work_steps, 4),
            "upper": r.upper, "upper_std_err": r.std_err, "lower": low.price, "lower_std_err": low.std_err,
            "q0_mean": r.sum_q0 / r.n, "grid": r.grid})
        del work, low_work
    out["build_id"] = capi.build_id()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
