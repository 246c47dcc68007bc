#!/usr/bin/env python3
"""Cost of mcamd_price_cliquet on one box, from the library's own HIP events: medians of --reps calls per job, one
process alternating call by call between
    mcamd_price_localvol, European call, no barrier (the kernel the cliquet kernels are modelled on),
    mcamd_price_cliquet, MCAMD_CLIQUET_SUM, COMPOUND and VARIANCE, each at reset_every = 1 and 21,
all on the 4 x 65 skewed surface of the tests at --paths x --steps (2^22 x 252), r = 0.1, q = 0.03, T = 1, local bounds
-3 % / +5 % and global bounds 0 / 25 % (none for VARIANCE), in fp64 and in fp32.  Printed as ONE JSON line; no time is
asserted anywhere.
    python3 tools/cliquet_bench.py [--reps 7] [--out profiles/cliquet_bench.json]     # on an MI355X
<kind>_<reset_every>_over_european is what the reset test and the period's arithmetic cost per job: one exponential per
reset for SUM, a subtract, two min / max and an add for COMPOUND, a subtract and a fused multiply-add for VARIANCE."""
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
    ap.add_argument("--paths", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=252)
    ap.add_argument("--resets", type=int, nargs="+", default=[1, 21])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    base = dict(S0=100.0, K=100.0, r=0.1, v=0.2, T=1.0)
    q = 0.03
    opt = capi.make_option(**base)
    xs = [-1.5 + 3.0 * k / 64 for k in range(65)]
    skew = ctx.localvol_surface((4, 65, -1.5, 1.5),
                                [[(0.18 + 0.04 * j) * (1.0 + 0.5 * math.exp(-x)) / 1.5 for x in xs] for j in range(4)])
    european = capi.make_localvol(capi.PAYOFF_CALL, q=q)
    kinds = {"sum": capi.CLIQUET_SUM, "compound": capi.CLIQUET_COMPOUND, "variance": capi.CLIQUET_VARIANCE}
    bounds = dict(local_floor=-0.03, local_cap=0.05, global_floor=0.0, global_cap=0.25)
    med = lambda xs_: sorted(xs_)[len(xs_) // 2]
    out = {"tool": "cliquet_bench", "device": ctx.device_info().name.decode(), "n_paths": args.paths,
           "n_steps": args.steps, "reps": args.reps, "resets": args.resets, "r": base["r"], "T": base["T"], "q": q,
           **bounds, "jobs": []}
    for prec in (capi.F64, capi.F32):
        sim = capi.make_sim(args.paths, args.steps, prec, seed=1234)
        calls = {"european": lambda: ctx.price_localvol(opt, sim, european, skew)}
        for name, kind in kinds.items():
            for every in args.resets:
                kw = {} if kind == capi.CLIQUET_VARIANCE else bounds
                cq = capi.make_cliquet(kind, every, 1, q=q, **kw)
                calls[f"{name}_{every}"] = lambda cq=cq: ctx.price_cliquet(opt, sim, cq, skew)
        for call in calls.values():
            call()   # warm-up: code objects, scratch
        ms = {name: [] for name in calls}
        last = {}
        for _ in range(args.reps):
            for name, call in calls.items():
                last[name] = call()
                ms[name].append(last[name].kernel_ms)
        m = {name: med(v) for name, v in ms.items()}
        job = {"precision": prec, **{name + "_ms": round(v, 3) for name, v in m.items()},
               **{name + "_over_european": round(v / m["european"], 3) for name, v in m.items() if name != "european"},
               "european_path_steps_per_s": args.paths * args.steps / (m["european"] * 1e-3),
               **{name + "_price": last[name].price for name in calls}, "grid": last["european"].grid}
        out["jobs"].append(job)
    out["build_id"] = capi.build_id()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    skew.close()
    ctx.close()


if __name__ == "__main__":
    main()
