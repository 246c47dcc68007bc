#!/usr/bin/env python3
"""Cost of mcamd_price_american on one box: training (trajectory store + backward sweep) and the pricing kernel, from
the library's own HIP events, medians of --reps calls per job, printed as ONE JSON line.  Beside them, the
product-form European pricer (mcamd_price_paths, MCAMD_FLAG_PRODUCT_FORM) on the priced job, alternating call by
call, as the yardstick of the pricing pass.
    python3 tools/american_bench.py [--reps 7]          # on an MI355X
Jobs: 1M training paths x 10M priced paths of 250 steps with M = 50 (k = 5) and of 252 steps with M = 252 (k = 1),
fp64 and fp32; the Bermudan put of Longstaff-Schwartz (S0 = 36, K = 40, r = 0.06, v = 0.2, T = 1)."""
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
    args = ap.parse_args()
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    opt = capi.make_option(S0=36.0, K=40.0, r=0.06, v=0.2, T=1.0)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    jobs = [(250, 5), (252, 1)]
    out = {"tool": "american_bench", "n_train": 1_000_000, "n_paths": 10_000_000, "reps": args.reps, "jobs": []}
    for prec in (capi.F64, capi.F32):
        for n_steps, k in jobs:
            am = capi.make_american(exercise_every=k, n_train=1_000_000, train_seed=11)
            sim = capi.make_sim(10_000_000, n_steps, prec, seed=12)
            work = torch.empty(capi.american_workspace_bytes(am, sim), dtype=torch.uint8, device="cuda")
            euro = capi.make_sim(10_000_000, n_steps, prec, seed=12, flags=capi.FLAG_PRODUCT_FORM)
            ctx.price_american(opt, sim, am, work)   # warm-up: code objects, scratch
            ctx.price_paths(opt, euro)
            train, price, total, eu = [], [], [], []
            for _ in range(args.reps):
                r = ctx.price_american(opt, sim, am, work)
                train.append(r.train_ms)
                price.append(r.price_ms)
                total.append(r.total_ms)
                eu.append(ctx.price_paths(opt, euro).kernel_ms)
            out["jobs"].append({"precision": prec, "n_steps": n_steps, "k": k, "M": n_steps // k,
                                "train_ms": round(med(train), 3), "price_ms": round(med(price), 3),
                                "total_ms": round(med(total), 3), "european_product_form_ms": round(med(eu), 3),
                                "price_over_european": round(med(price) / med(eu), 3),
                                "price": r.price, "std_err": r.std_err, "in_sample_price": r.in_sample_price,
                                "n_early": r.n_early, "n_regressed": r.n_regressed, "grid": r.grid,
                                "train_grid": r.train_grid})
            del work
    out["build_id"] = capi.build_id()
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
