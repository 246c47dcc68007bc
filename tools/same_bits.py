#!/usr/bin/env python3
"""Do two builds of the library compute the same bits?  One fresh worker process per library (MCAMD_LIB) runs a fixed
list of small jobs on the kernels that walk a local-volatility surface — mcamd_price_localvol, mcamd_price_localvol_smile,
mcamd_price_autocall_localvol, mcamd_price_cliquet, mcamd_price_localvol_greeks — on mcamd_price_heston (a put and a
call, with the samples and the final state) and mcamd_price_heston_smile (1 x 1 and 3 x 63 nodes, expiries at step 1 and
at the last step, with the spots and variances at every expiry), mcamd_price_heston_cliquet (three kinds over the
periods) and mcamd_price_heston_barrier (every kind x monitoring x payoff, with the samples and the final state), and on
the one-path-per-thread kernels of constant volatility — mcamd_price_barrier, mcamd_price_lookback, mcamd_price_asian, the likelihood-ratio and pathwise
mcamd_price_greeks, mcamd_price_american, mcamd_american_upper_bound, and on d = 1..8 correlated assets
mcamd_price_basket and mcamd_price_autocall — and prints a SHA-256 per job over the per-path
outputs where the call has them (samples, spots, continuation values, coefficients) and the result record without its
timings; this process compares the lines.
    python3 tools/same_bits.py LIB_A LIB_B          # on an MI355X; exit status 1 on any difference
Every job is 1000 paths (four workgroups, a partial last wavefront) of a 2^40-path job, from path 5003 and from path
2^33 + 5003, in both precisions.  Step counts 1, 2, 3, 5, 7 and 13 leave every remainder of a Philox block of 2 and of
4 normals; the one-path-per-thread kernels also take 4 and 8, a path of whole blocks only in fp32 too; where a product
ties the count to a period (reset_every, exercise_every) the counts still leave no whole block, no remainder and a
remainder.  The surfaces are a
flat 1 x 2, a skewed 3 x 5 (n_t divides no step count but 3), a 16 x 5 (more rows than steps), the full 16 x 128 table
and an axis so narrow that the paths clamp on both sides.  The baskets take every kind x payoff, and best-of / worst-of
with every barrier, at d = 1..8 over the step counts of the one-path-per-thread kernels: a group of G = NB / gcd(d, NB)
steps is 1, 2 or 4 steps, so they leave every remainder, no whole group, and whole groups only; the constant-volatility
autocallable takes d = 1..8 and the three knock-in modes over the (n_steps, period) pairs.  Some jobs make whole
wavefronts leave the step loop after a whole block or group, and their names carry the proof: a knock-out barrier beside
the spot on 100 000 paths, under constant volatility and under Heston, and a worst-of knock-out basket with the barrier
beside the aggregate (d = 3 and 8; their work_steps fall short of the full count — for the Heston barrier and the
baskets the worker refuses to go on otherwise); an American put so deep in the money
(K = 10 S0) that every priced path is exercised at the first date, step 4 of 48, so that every wavefront of the
pricing kernel leaves 44 steps early; and a 3-asset note with a call level of 0.01 under mcamd_price_autocall and under
mcamd_price_autocall_localvol, every path called at the first date, step 4 of 48, after 4 wave-steps per wavefront —
the worker refuses to go on otherwise there too."""
import hashlib, importlib, json, math, os, struct, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, OFFSETS, STEPS = 1000, (5003, 2 ** 33 + 5003), (1, 2, 3, 5, 7, 13)
STEPS_WALK = (1, 2, 3, 4, 5, 7, 8, 13)   # of the one-path-per-thread kernels: 4 and 8 are whole blocks in fp32 as well
# (n_steps, period): reset_every of a cliquet, exercise_every of an American option
PERIODS = ((1, 1), (2, 1), (2, 2), (3, 1), (3, 3), (4, 2), (5, 1), (7, 7), (8, 1), (8, 4), (13, 1), (13, 13))


def surfaces(ctx):
    def skew(n_t, n_x, lo, hi, v=0.2):
        xs = [lo + k * (hi - lo) / (n_x - 1) for k in range(n_x)]
        return ctx.localvol_surface((n_t, n_x, lo, hi),
                                    [[v * (0.9 + 0.05 * t) * (1.0 + 0.5 * math.exp(-x)) / 1.5 for x in xs] for t in range(n_t)])
    return {"flat": ctx.localvol_surface((1, 2, -1.5, 1.5), [[0.2, 0.2]]), "skew3x5": skew(3, 5, -1.0, 1.0),
            "rows16x5": skew(16, 5, -1.0, 1.0, 0.3), "full16x128": skew(16, 128, -1.5, 1.5),
            "narrow": skew(2, 4, -0.01, 0.01, 0.4)}


def worker():
    sys.path.insert(0, ROOT)
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0, stream.cuda_stream)
    surf = surfaces(ctx)
    dtype = {capi.F32: torch.float32, capi.F64: torch.float64}

    def emit(name, res, *arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(a.cpu().numpy().tobytes() if hasattr(a, "cpu") else a.tobytes())
        for key, _ in res._fields_:   # the record without its timings; an array field value by value
            if not key.endswith("_ms"):
                value = getattr(res, key)
                for v in (value if hasattr(value, "__len__") else (value,)):
                    h.update(struct.pack("<d", float(v)))
        print(json.dumps({"job": name, "sha256": h.hexdigest()}))

    def sim(n_steps, prec, off, n=N):
        return capi.make_sim(2 ** 40, n_steps, prec, seed=77, path_offset=off, n_paths_local=n)

    for prec in (capi.F32, capi.F64):
        for off in OFFSETS:
            tag = f"f{prec} @{off}"
            out = torch.empty(N, dtype=dtype[prec], device="cuda")
            # mcamd_price_localvol: no barrier, and every kind x monitoring x payoff, on every surface and step count
            kinds = [(capi.LOCALVOL_NO_BARRIER, capi.MONITOR_DISCRETE, capi.PAYOFF_CALL)] + [
                (kind, mon, pay) for kind in range(4) for mon in (capi.MONITOR_DISCRETE, capi.MONITOR_CONTINUOUS)
                for pay in (capi.PAYOFF_CALL, capi.PAYOFF_PUT)]
            for sname, s in surf.items():
                for n_steps in STEPS_WALK:
                    for kind, mon, pay in kinds:
                        up = kind in (capi.BARRIER_UP_OUT, capi.BARRIER_UP_IN)
                        opt = capi.make_option(S0=100.0, K=100.0, B=110.0 if up else 90.0, r=0.05, v=0.0, T=1.0)
                        res = ctx.price_localvol(opt, sim(n_steps, prec, off), capi.make_localvol(pay, kind, mon, q=0.02), s,
                                                 out.zero_())
                        emit(f"localvol {tag} {sname} n={n_steps} kind={kind} mon={mon} pay={pay}", res, out)
            # mcamd_price_localvol_smile: expiries on different slots of a Philox block and in the remainder block
            opt = capi.make_option(S0=100.0, K=0.0, r=0.05, v=0.0, T=1.0)
            for sname in ("skew3x5", "full16x128", "narrow"):
                for n_K in (1, 64):
                    strikes = [60.0 + 80.0 * k / max(n_K - 1, 1) for k in range(n_K)]
                    spots = torch.zeros(3 * N, dtype=dtype[prec], device="cuda")
                    _, _, stats, res = ctx.price_localvol_smile(opt, sim(13, prec, off), capi.make_smile(3, n_K, q=0.02),
                                                                (5, 6, 13), strikes, surf[sname], spots)
                    emit(f"smile {tag} {sname} n_K={n_K}", res, spots, stats)
            # two trips: 32 x 64 nodes cap the grid at 512 workgroups, so 150 000 paths make wavefronts add to their record
            n2, strikes = 150_000, [60.0 + 80.0 * k / 63 for k in range(64)]
            spots = torch.zeros(32 * n2, dtype=dtype[prec], device="cuda")
            _, _, stats, res = ctx.price_localvol_smile(opt, sim(32, prec, off, n2), capi.make_smile(32, 64, capi.PAYOFF_PUT),
                                                        range(1, 33), strikes, surf["skew3x5"], spots)
            emit(f"smile {tag} two trips grid={res.grid}", res, spots, stats)
            # mcamd_price_autocall_localvol: every width and knock-in mode, a surface per asset, and one shared by three
            opt = capi.make_option(S0=0.0, K=0.0, r=0.03, v=0.0, T=3.0)
            cycle = ["skew3x5", "flat", "rows16x5", "narrow"]
            notes = [(d, [cycle[j % 4] for j in range(d)]) for d in range(1, 9)]
            notes += [(1, ["full16x128"]), (3, ["skew3x5"] * 3)]
            for d, names in notes:
                ss = [surf[name] for name in names]
                corr = [[0.5 ** abs(j - k) for k in range(d)] for j in range(d)]
                q = [0.01 * (j % 3) for j in range(d)]
                for ki in (capi.AUTOCALL_KI_NONE, capi.AUTOCALL_KI_AT_MATURITY, capi.AUTOCALL_KI_EVERY_STEP):
                    ac = capi.make_autocall_localvol(q, corr, 3, 1.0, 0.02, 0.8 if ki else 0.0, ki, call_step_down=0.01)
                    res = ctx.price_autocall_localvol(opt, sim(12, prec, off), ac, ss, out.zero_())
                    emit(f"autocall {tag} d={d} on {'+'.join(names)} ki={ki}", res, out)
            # mcamd_price_cliquet: every kind, resets inside a block, at its end and at the path's end only
            opt = capi.make_option(S0=100.0, K=0.0, r=0.05, v=0.0, T=1.0)
            for sname in ("skew3x5", "full16x128"):
                for n_steps, every in PERIODS:
                    for kind in (capi.CLIQUET_SUM, capi.CLIQUET_COMPOUND, capi.CLIQUET_VARIANCE):
                        local = {} if kind == capi.CLIQUET_VARIANCE else dict(local_floor=-0.03, local_cap=0.05)
                        cq = capi.make_cliquet(kind, every, 1 + (n_steps // every) // 3, global_floor=0.0, global_cap=0.2,
                                               q=0.02, **local)
                        res = ctx.price_cliquet(opt, sim(n_steps, prec, off), cq, surf[sname], out.zero_())
                        emit(f"cliquet {tag} {sname} n={n_steps} every={every} kind={kind}", res, out)
            # mcamd_price_localvol_greeks: with and without gamma's two bumped walks and the vega buckets
            opt = capi.make_option(S0=100.0, K=100.0, r=0.05, v=0.0, T=1.0)
            for sname in ("skew3x5", "full16x128"):
                for n_steps in STEPS_WALK:
                    for n_b, bump in ((0, 0.0), (0, 0.01), (3, 0.0), (8, 0.01)):
                        each = torch.zeros((6 + n_b) * N, dtype=torch.float64, device="cuda")
                        job = capi.make_localvol_greeks_job(capi.PAYOFF_PUT if n_b == 3 else capi.PAYOFF_CALL, n_b, 0.02, bump)
                        res = ctx.price_localvol_greeks(opt, sim(n_steps, prec, off), job, surf[sname], each)
                        emit(f"localvol greeks {tag} {sname} n={n_steps} buckets={n_b} bump={bump}", res, each)
            # mcamd_price_heston: a put and a call; xi = 1 against kappa theta = 0.08 sends variances below zero
            opt = capi.make_option(S0=100.0, K=100.0, r=0.05, v=0.0, T=1.0)
            state = torch.empty(2 * N, dtype=dtype[prec], device="cuda")
            for n_steps in STEPS_WALK:
                for pay in (capi.PAYOFF_CALL, capi.PAYOFF_PUT):
                    hs = capi.make_heston(pay, q=0.02, v0=0.04, kappa=2.0, theta=0.04, xi=1.0, rho=-0.7)
                    res = ctx.price_heston(opt, sim(n_steps, prec, off), hs, out.zero_(), state.zero_())
                    emit(f"heston {tag} n={n_steps} pay={pay}", res, out, state)
            # mcamd_price_heston_smile on the same model: one node at step 1 and one at the last step, and 3 x 63 nodes
            # with expiries at step 1, half way and at the last step (1 or 2 expiries where n_steps < 3 holds no more);
            # the spots and raw variances are hashed with the sums
            for n_steps in STEPS_WALK:
                ends = sorted({1, (n_steps + 1) // 2, n_steps})
                for pay, steps, n_K in [(capi.PAYOFF_CALL, (s,), 1) for s in sorted({1, n_steps})] + [(capi.PAYOFF_PUT, ends, 63)]:
                    strikes = [60.0 + 80.0 * k / max(n_K - 1, 1) for k in range(n_K)]
                    hs = capi.make_heston(pay, q=0.02, v0=0.04, kappa=2.0, theta=0.04, xi=1.0, rho=-0.7)
                    state = torch.zeros(2 * len(steps) * N, dtype=dtype[prec], device="cuda")
                    _, _, stats, res = ctx.price_heston_smile(opt, sim(n_steps, prec, off), hs, steps, strikes, state)
                    emit(f"heston smile {tag} n={n_steps} expiries={list(steps)} n_K={n_K}", res, state, stats)
            # mcamd_price_heston_cliquet on the same model: every kind, resets inside a block, at its end and at the
            # path's end only
            opt = capi.make_option(S0=100.0, K=0.0, r=0.05, v=0.0, T=1.0)
            hs = capi.make_heston(capi.PAYOFF_CALL, q=0.02, v0=0.04, kappa=2.0, theta=0.04, xi=1.0, rho=-0.7)
            for n_steps, every in PERIODS:
                for kind in (capi.CLIQUET_SUM, capi.CLIQUET_COMPOUND, capi.CLIQUET_VARIANCE):
                    local = {} if kind == capi.CLIQUET_VARIANCE else dict(local_floor=-0.03, local_cap=0.05)
                    cq = capi.make_cliquet(kind, every, 1 + (n_steps // every) // 3, global_floor=0.0, global_cap=0.2,
                                           q=0.02, **local)
                    res = ctx.price_heston_cliquet(opt, sim(n_steps, prec, off), hs, cq, out.zero_())
                    emit(f"heston cliquet {tag} n={n_steps} every={every} kind={kind}", res, out)
            # mcamd_price_heston_barrier on the same model: every kind, monitoring and payoff, with S_T, the variance
            # and the survival weight of every path
            state = torch.empty(3 * N, dtype=dtype[prec], device="cuda")
            for n_steps in STEPS_WALK:
                for kind in range(4):
                    up = kind in (capi.BARRIER_UP_OUT, capi.BARRIER_UP_IN)
                    opt = capi.make_option(S0=100.0, K=100.0, B=110.0 if up else 90.0, r=0.05, v=0.0, T=1.0)
                    for mon in (capi.MONITOR_DISCRETE, capi.MONITOR_CONTINUOUS):
                        for pay in (capi.PAYOFF_CALL, capi.PAYOFF_PUT):
                            hs = capi.make_heston(pay, q=0.02, v0=0.04, kappa=2.0, theta=0.04, xi=1.0, rho=-0.7)
                            res = ctx.price_heston_barrier(opt, sim(n_steps, prec, off), hs, capi.make_barrier(kind, pay, mon),
                                                           out.zero_(), state.zero_())
                            emit(f"heston barrier {tag} n={n_steps} kind={kind} mon={mon} pay={pay}", res, out, state)
            # ... and a knock-out with the barrier beside the spot under a drift of -0.5: whole wavefronts leave after a
            # whole block
            n_ko = 100_000
            opt = capi.make_option(S0=100.0, K=100.0, B=99.9, r=0.0, v=0.0, T=1.0)
            hs = capi.make_heston(capi.PAYOFF_CALL, q=0.5, v0=0.16, kappa=2.0, theta=0.16, xi=1.0, rho=-0.7)
            many, state = (torch.empty(k * n_ko, dtype=dtype[prec], device="cuda") for k in (1, 3))
            res = ctx.price_heston_barrier(opt, sim(51, prec, off, n_ko), hs,
                                           capi.make_barrier(capi.BARRIER_DOWN_OUT, capi.PAYOFF_CALL, capi.MONITOR_CONTINUOUS),
                                           many.zero_(), state.zero_())
            full = 64.0 * 51 * ((n_ko + 63) // 64)
            if not res.work_steps < full:
                raise SystemExit(f"heston barrier {tag}: no wavefront left the loop early ({res.work_steps} of {full})")
            emit(f"heston barrier {tag} early exit work={res.work_steps:.0f} of {full:.0f}", res, many, state)
            # mcamd_price_barrier: every kind, monitoring and payoff
            for n_steps in STEPS_WALK:
                for kind in range(4):
                    up = kind in (capi.BARRIER_UP_OUT, capi.BARRIER_UP_IN)
                    opt = capi.make_option(S0=100.0, K=100.0, B=110.0 if up else 90.0, r=0.05, v=0.2, T=1.0)
                    for mon in (capi.MONITOR_DISCRETE, capi.MONITOR_CONTINUOUS):
                        for pay in (capi.PAYOFF_CALL, capi.PAYOFF_PUT):
                            res = ctx.price_barrier(opt, sim(n_steps, prec, off), capi.make_barrier(kind, pay, mon), out.zero_())
                            emit(f"barrier {tag} n={n_steps} kind={kind} mon={mon} pay={pay}", res, out)
            # ... and a knock-out with the barrier beside the spot: whole wavefronts leave after a whole block
            n_ko = 100_000
            opt = capi.make_option(S0=100.0, K=100.0, B=99.9, r=0.0, v=0.4, T=1.0)
            many = torch.empty(n_ko, dtype=dtype[prec], device="cuda")
            for mon in (capi.MONITOR_DISCRETE, capi.MONITOR_CONTINUOUS):
                res = ctx.price_barrier(opt, sim(51, prec, off, n_ko), capi.make_barrier(capi.BARRIER_DOWN_OUT, capi.PAYOFF_CALL, mon),
                                        many.zero_())
                emit(f"barrier {tag} early exit mon={mon} work={res.work_steps:.0f} of {64.0 * 51 * ((n_ko + 63) // 64):.0f}",
                     res, many)
            # mcamd_price_lookback: both monitorings, strikes and payoffs
            opt = capi.make_option(S0=100.0, K=105.0, r=0.05, v=0.25, T=1.0)
            for n_steps in STEPS_WALK:
                for mon in (capi.MONITOR_DISCRETE, capi.MONITOR_CONTINUOUS):
                    for strike in (capi.LOOKBACK_FLOATING, capi.LOOKBACK_FIXED):
                        for pay in (capi.PAYOFF_CALL, capi.PAYOFF_PUT):
                            res = ctx.price_lookback(opt, sim(n_steps, prec, off), capi.make_lookback(strike, pay, mon), out.zero_())
                            emit(f"lookback {tag} n={n_steps} mon={mon} strike={strike} pay={pay}", res, out)
            # mcamd_price_asian: arithmetic, geometric, and arithmetic with the geometric control
            for n_steps in STEPS_WALK:
                for avg, control in ((capi.ASIAN_ARITHMETIC, capi.ASIAN_CONTROL_NONE), (capi.ASIAN_GEOMETRIC, capi.ASIAN_CONTROL_NONE),
                                     (capi.ASIAN_ARITHMETIC, capi.ASIAN_CONTROL_GEOMETRIC)):
                    for strike in (capi.ASIAN_FIXED, capi.ASIAN_FLOATING):
                        for pay in (capi.PAYOFF_CALL, capi.PAYOFF_PUT):
                            asian = capi.make_asian(avg, strike, pay, include_spot=(n_steps + pay) % 2, control=control)
                            res = ctx.price_asian(opt, sim(n_steps, prec, off), asian, out.zero_())
                            emit(f"asian {tag} n={n_steps} avg={avg} control={control} strike={strike} pay={pay}", res, out)
            # mcamd_price_greeks: likelihood ratio without and with the bullet window (it closes: P2 = 1), and pathwise
            for n_steps in STEPS_WALK:
                plain = capi.make_option(S0=100.0, K=100.0, r=0.05, v=0.2, T=1.0)
                window = capi.make_option(S0=100.0, K=100.0, B=101.0, P1=0, P2=1, use_window=1, r=0.05, v=0.2, T=1.0)
                for name, opt, method in (("lr", plain, capi.GREEKS_LIKELIHOOD_RATIO), ("lr window", window, capi.GREEKS_LIKELIHOOD_RATIO),
                                          ("pathwise", plain, capi.GREEKS_PATHWISE)):
                    emit(f"greeks {tag} {name} n={n_steps}", ctx.price_greeks(opt, sim(n_steps, prec, off), method))
            # mcamd_price_american and mcamd_american_upper_bound on its rule; K = 1000 at 48 steps: so deep in the money
            # that every path is exercised at the first date, so every wavefront leaves after the block that holds step 4
            for n_steps, every in PERIODS + ((48, 4),):
                for K in (100.0, 1000.0):
                    if K == 1000.0 and n_steps != 48:
                        continue
                    opt = capi.make_option(S0=100.0, K=K, r=0.06, v=0.3, T=1.0)
                    s, am = sim(n_steps, prec, off), capi.make_american(capi.PAYOFF_PUT, every, n_train=4096, train_seed=99)
                    work = torch.empty(capi.american_workspace_bytes(am, s), dtype=torch.uint8, device="cuda")
                    res, rule = ctx.price_american(opt, s, am, work, coeffs=True)
                    note = ""
                    if K == 1000.0:
                        t_first = every * opt.T / n_steps
                        if res.n_early != N or abs(res.sum_t_exercise - N * t_first) > 1e-9 * N:
                            raise SystemExit(f"american {tag}: {res.n_early} of {N} paths exercised early, mean date "
                                             f"{res.sum_t_exercise / max(res.n_early, 1)}: not all at the first, {t_first}")
                        note = f" early exit: all {res.n_early} paths exercised at step {every}"
                    emit(f"american {tag} n={n_steps} every={every} K={K}{note}", res, rule)
                    dual = capi.make_american_dual(n_inner=96, inner_seed=55)
                    work = torch.empty(capi.american_dual_workspace_bytes(am, s, dual), dtype=torch.uint8, device="cuda")
                    cont = torch.zeros((n_steps // every) * N, dtype=torch.float64, device="cuda")
                    res = ctx.american_upper_bound(opt, s, am, dual, rule, work, cont)
                    emit(f"american dual {tag} n={n_steps} every={every} K={K} work={res.work_steps:.0f}", res, cont)
            # mcamd_price_basket: every width, kind and payoff, and best-of / worst-of with every barrier
            extreme = (capi.BASKET_BEST_OF, capi.BASKET_WORST_OF)
            for d in range(1, 9):
                corr = [[0.5 ** abs(j - k) for k in range(d)] for j in range(d)]
                S0, v = [100.0 + j for j in range(d)], [0.2 + 0.02 * j for j in range(d)]
                for n_steps in STEPS_WALK:
                    for kind in range(4):
                        w = [1.0] * d if kind in extreme else [1.0 / d] * d
                        for barrier in range(5 if kind in extreme else 1):
                            up = barrier in (capi.BASKET_UP_OUT, capi.BASKET_UP_IN)
                            opt = capi.make_option(S0=0.0, K=100.0, B=115.0 if up else 90.0, r=0.05, v=0.0, T=1.0)
                            for pay in (capi.PAYOFF_CALL, capi.PAYOFF_PUT):
                                res = ctx.price_basket(opt, sim(n_steps, prec, off), capi.make_basket(S0, v, w, corr, kind, pay, barrier),
                                                       out.zero_())
                                emit(f"basket {tag} d={d} n={n_steps} kind={kind} barrier={barrier} pay={pay}", res, out)
            # ... and a worst-of knock-out with the barrier beside the aggregate: whole wavefronts leave after a whole group
            opt = capi.make_option(S0=0.0, K=100.0, B=99.9, r=0.0, v=0.0, T=1.0)
            for d in (3, 8):
                corr = [[0.5 ** abs(j - k) for k in range(d)] for j in range(d)]
                bk = capi.make_basket([100.0] * d, [0.4] * d, [1.0] * d, corr, capi.BASKET_WORST_OF, capi.PAYOFF_CALL,
                                      capi.BASKET_DOWN_OUT)
                res = ctx.price_basket(opt, sim(51, prec, off, n_ko), bk, many.zero_())
                full = 64.0 * 51 * ((n_ko + 63) // 64)
                if not res.work_steps < full:
                    raise SystemExit(f"basket {tag} d={d}: no wavefront left the loop early ({res.work_steps} of {full})")
                emit(f"basket {tag} d={d} early exit work={res.work_steps:.0f} of {full:.0f}", res, many)
            # mcamd_price_autocall: every width, the three knock-in modes, dates inside a group, at its end and at maturity only
            opt = capi.make_option(S0=0.0, K=0.0, r=0.03, v=0.0, T=3.0)
            for d in range(1, 9):
                corr = [[0.5 ** abs(j - k) for k in range(d)] for j in range(d)]
                v = [0.2 + 0.02 * j for j in range(d)]
                for n_steps, every in PERIODS:
                    for ki in (capi.AUTOCALL_KI_NONE, capi.AUTOCALL_KI_AT_MATURITY, capi.AUTOCALL_KI_EVERY_STEP):
                        ac = capi.make_autocall(v, corr, every, 1.0, 0.02, 0.8 if ki else 0.0, ki, call_step_down=0.01)
                        res = ctx.price_autocall(opt, sim(n_steps, prec, off), ac, out.zero_())
                        emit(f"autocall const {tag} d={d} n={n_steps} every={every} ki={ki}", res, out)
            # ... and, under constant volatilities and under surfaces, a note with a call level so low (0.01) that every path
            # is called at the first date, step 4 of 48: every wavefront leaves after the group that holds step 4
            d, every, n_steps = 3, 4, 48
            corr = [[0.5 ** abs(j - k) for k in range(d)] for j in range(d)]
            t_first, early = every * opt.T / n_steps, 64.0 * every * ((N + 63) // 64)
            for name, run in (("autocall const", lambda: ctx.price_autocall(
                                  opt, sim(n_steps, prec, off), capi.make_autocall([0.2, 0.22, 0.24], corr, every, 0.01, 0.02), out.zero_())),
                              ("autocall", lambda: ctx.price_autocall_localvol(
                                  opt, sim(n_steps, prec, off), capi.make_autocall_localvol([0.0, 0.01, 0.02], corr, every, 0.01, 0.02),
                                  [surf["skew3x5"], surf["flat"], surf["rows16x5"]], out.zero_()))):
                res = run()
                if res.n_called != N or abs(res.sum_t_call - N * t_first) > 1e-9 * N or res.work_steps != early:
                    raise SystemExit(f"{name} {tag}: {res.n_called} of {N} paths called, mean date "
                                     f"{res.sum_t_call / max(res.n_called, 1)}, {res.work_steps} wave-steps: not all called at "
                                     f"the first date, {t_first}, after {early} wave-steps")
                emit(f"{name} {tag} d={d} early exit: all {res.n_called} paths called at step {every}, work={res.work_steps:.0f}",
                     res, out)
    print(json.dumps({"build_id": capi.build_id()}))
    for s in surf.values():
        s.close()
    ctx.close()


def main():
    if sys.argv[1:] == ["--worker"]:
        return worker()
    if len(sys.argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    runs = []
    n_lines = []
    for lib in sys.argv[1:]:
        env = dict(os.environ, MCAMD_LIB=os.path.abspath(lib))
        o = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=env, capture_output=True, text=True)
        lines = [json.loads(l) for l in o.stdout.splitlines() if l.startswith("{")]
        if o.returncode or not lines or "build_id" not in lines[-1]:
            print(f"worker failed for {lib} (exit status {o.returncode}):", o.stderr[-2000:], file=sys.stderr)
            return 1
        runs.append((lines[-1]["build_id"], {l["job"]: l["sha256"] for l in lines[:-1]}))
        n_lines.append(len(lines) - 1)
    (id_a, a), (id_b, b) = runs
    differ = sorted(job for job in set(a) | set(b) if a.get(job) != b.get(job))
    for job in differ:
        print("DIFFERS", job)
    for job in sorted(a):   # the jobs whose names carry what shows that wavefronts did leave early
        if "early exit" in job:
            print("ran", job)
    print(f"same_bits: {len(a)} jobs, {len(differ)} differ; builds {id_a} and {id_b}")
    if n_lines != [len(a), len(b)]:
        print("same_bits: two jobs share a name", file=sys.stderr)
        return 1
    return 1 if differ or not a else 0


if __name__ == "__main__":
    sys.exit(main())
