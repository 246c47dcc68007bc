#!/usr/bin/env python3
"""Cost of mcamd_price_autocall_localvol on one box, from the library's own HIP events: medians of --reps calls per job
after one warm-up call each, one process alternating call by call, in fp64 and in fp32.  The job is the note of
tools/autocall_bench.py: 3 assets, --paths x --steps (1M x 1260, 252 steps a year), an observation every 63 steps (20
dates), autocall level 1, coupon 0.02 a date, knock-in at 0.6 monitored at every step, corr_jk = 0.6^|j - k|, r = 0.05,
T = 5.  It runs
    on flat 1 x 2 surfaces at sigma_j = v_j = 0.15 + 0.05 j, q = 0   (the constant-volatility note, looked up),
    on skewed 4 x 65 surfaces  sigma_j(t, x) = v_j (0.9 + 0.07 t) (1 + 0.5 e^{-x}) / 1.5  with q = (0, 0.03, 0.01),
and beside them, in the same run, mcamd_price_autocall on the same note at v_j — the yardstick: the same loop without
the D lookups per step — and the ratios.  Reports kernel ms, live_steps / work_steps (how full the wavefronts ran) and
work_steps over the full count (how much of the loop the early exit saved).  --assets and --skew-nx run other widths
(8 assets need --skew-nx 33 or less: the tables of all assets share 2048 nodes).  Printed as ONE JSON line; no time is
asserted anywhere.
    python3 tools/autocall_localvol_bench.py [--reps 7] [--out profiles/autocall_localvol_bench.json]     # on an MI355X"""
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
    ap.add_argument("--paths", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=1260)
    ap.add_argument("--observe-every", type=int, default=63)
    ap.add_argument("--assets", type=int, default=3, help="1..8; beyond 3, q_j repeats and v_j keeps growing")
    ap.add_argument("--skew-nx", type=int, default=65, help="nodes per slice of the skewed surfaces (4 slices each)")
    ap.add_argument("--ki", choices=("every-step", "maturity"), default="every-step", help="the knock-in's monitoring")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    r, T, d, ki_level = 0.05, 5.0, args.assets, 0.6
    ki = capi.AUTOCALL_KI_EVERY_STEP if args.ki == "every-step" else capi.AUTOCALL_KI_AT_MATURITY
    med = lambda xs: sorted(xs)[len(xs) // 2]
    v = [0.15 + 0.05 * j for j in range(d)]
    q = [(0.0, 0.03, 0.01)[j % 3] for j in range(d)]
    corr = [[0.6 ** abs(j - k) for k in range(d)] for j in range(d)]
    full = 64 * -(-args.paths // 64) * args.steps
    n_t, n_x, x_min, x_max = 4, args.skew_nx, -1.5, 1.5
    xs = [x_min + k * (x_max - x_min) / (n_x - 1) for k in range(n_x)]
    flat = [ctx.localvol_surface((1, 2, x_min, x_max), [[v[j], v[j]]]) for j in range(d)]
    skew = [ctx.localvol_surface((n_t, n_x, x_min, x_max),
                                 [[v[j] * (0.9 + 0.07 * t) * (1.0 + 0.5 * math.exp(-x)) / 1.5 for x in xs] for t in range(n_t)])
            for j in range(d)]

    out = {"tool": "autocall_localvol_bench", "device": ctx.device_info().name.decode(), "paths": args.paths,
           "steps": args.steps, "observe_every": args.observe_every, "assets": d, "ki": args.ki, "reps": args.reps, "r": r, "T": T,
           "skewed_grid": [n_t, n_x, x_min, x_max], "q_skewed": q, "jobs": []}
    for prec in (capi.F64, capi.F32):
        sim = capi.make_sim(args.paths, args.steps, prec, seed=1234)
        opt = capi.make_option(S0=0.0, v=0.0, K=0.0, r=r, T=T)
        gbm = capi.make_autocall(v, corr, args.observe_every, 1.0, 0.02, ki_level, ki)
        lv0 = capi.make_autocall_localvol([0.0] * d, corr, args.observe_every, 1.0, 0.02, ki_level, ki)
        lvq = capi.make_autocall_localvol(q, corr, args.observe_every, 1.0, 0.02, ki_level, ki)
        calls = {"autocall": lambda: ctx.price_autocall(opt, sim, gbm),
                 "flat": lambda: ctx.price_autocall_localvol(opt, sim, lv0, flat),
                 "skewed": lambda: ctx.price_autocall_localvol(opt, sim, lvq, skew)}
        for call in calls.values():
            call()   # warm-up: code objects, scratch
        times = {key: [] for key in calls}
        last = {}
        for _ in range(args.reps):
            for key, call in calls.items():
                last[key] = call()
                times[key].append(last[key].kernel_ms)
        job = {"precision": prec}
        for name in calls:
            t, res = med(times[name]), last[name]
            job[name] = {
                "kernel_ms": round(t, 3), "price": res.price, "std_err": res.std_err,
                "called": res.n_called / args.paths, "mean_call_time": res.sum_t_call / max(res.n_called, 1),
                "knocked_in": res.n_knocked_in / args.paths,
                "live_over_work": round(res.live_steps / res.work_steps, 4),
                "work_over_full": round(res.work_steps / full, 4),
                "asset_steps_per_s": res.work_steps * d / (t * 1e-3),
                "ms_per_work_gstep": round(t / (res.work_steps * 1e-9), 4),
                "over_autocall": round(t / med(times["autocall"]), 3), "grid": res.grid}
        out["jobs"].append(job)
    out["build_id"] = capi.build_id()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for s in flat + skew:
        s.close()
    ctx.close()


if __name__ == "__main__":
    main()
