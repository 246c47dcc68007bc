"""GPU tests of the Andersen-Broadie dual bound (mcamd_american_upper_bound).  Run with -m gpu on an MI355X.

  * exact: the continuation values of chosen points against inner paths obtained independently of the new kernel —
    the trajectory store restarted at (S_{p,j}, s_j) on the point's own Philox subsequences — with the rule applied
    in numpy; the scan against numpy on the engine's stored outer rows and its own continuation values; one date;
    repeatability, shards, d_cont = NULL; a never-exercise rule.  fp64 sums to 1e-11, decisions through
    american_restate.decide (tests/american_dual_restate.py).
  * statistical: the fitted rule's upper estimate and the lower estimate of the same rule bracket a CRR tree that
    exercises at the same dates (Longstaff-Schwartz Table 1); the fitted rule's bound lies well below the
    never-exercise rule's; an American call without dividends is bounded by the European value."""
import importlib
import math

import numpy as np
import pytest

import american_dual_restate as adr
import american_restate as ar

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

LS = dict(K=40.0, r=0.06)
TORCH_T = {capi.F64: torch.float64, capi.F32: torch.float32}
RTOL = 1e-11


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    import os
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    c = capi.Context(0, stream.cuda_stream)
    yield c
    c.close()
    torch.cuda.set_stream(torch.cuda.default_stream())


def fit_rule(ctx, opt, n_steps, prec, am):
    """(lower-bound result, coefficient table) of mcamd_price_american on 2 000 000 fresh paths"""
    sim = capi.make_sim(2_000_000, n_steps, prec, seed=32)
    work = torch.empty(capi.american_workspace_bytes(am, sim), dtype=torch.uint8, device="cuda")
    return ctx.price_american(opt, sim, am, work, coeffs=True)


def bound(ctx, opt, sim, am, dual, coeffs, cont=True):
    """(result, Q [M, n_local] or None)"""
    M = sim.n_steps // am.exercise_every
    work = torch.empty(capi.american_dual_workspace_bytes(am, sim, dual), dtype=torch.uint8, device="cuda")
    q = torch.full((M * sim.n_paths_local,), float("nan"), dtype=torch.float64, device="cuda") if cont else None
    res = ctx.american_upper_bound(opt, sim, am, dual, coeffs, work, cont=q)
    return res, (q.view(M, sim.n_paths_local).cpu().numpy() if cont else None)


def stored_rows(ctx, opt, n, n_steps, prec, seed, path_offset=0, n_local=None, n_sim=None):
    n_local = n if n_local is None else n_local
    n_sim = n_steps if n_sim is None else n_sim
    traj = torch.empty(n_local * n_sim, dtype=TORCH_T[prec], device="cuda")
    ctx.simulate_trajectories(opt, capi.make_sim(n, n_steps, prec, seed=seed, flags=capi.FLAG_PRODUCT_FORM,
                                                 path_offset=path_offset, n_paths_local=n_local), traj)
    return traj.view(n_sim, n_local).cpu().numpy().astype(np.float64)


def unpack(coeffs):
    return coeffs[:, :-1], coeffs[:, -1] != 0


def small_rule(ctx, opt, n_steps, prec, k, m, drop=()):
    """A fitted rule of a small job; drop: dates whose rule is taken out (flag 0, NaN coefficients)"""
    am = capi.make_american(exercise_every=k, n_basis=m, n_train=60_000, train_seed=1000 + n_steps)
    sim = capi.make_sim(1000, n_steps, prec, seed=5)
    work = torch.empty(capi.american_workspace_bytes(am, sim), dtype=torch.uint8, device="cuda")
    _, coeffs = ctx.price_american(opt, sim, am, work, coeffs=True)
    for j in drop:
        coeffs[j - 1, :-1] = np.nan
        coeffs[j - 1, -1] = 0.0
    return am, coeffs


# (precision, exercise_every, n_basis, n_steps, dates without a rule): fp64 (2 steps per Philox block) and fp32 (4) with
# remaining step counts of every remainder, k = 1 and k > 1, a rule with holes
CONT_CASES = [(capi.F64, 1, 3, 21, ()), (capi.F32, 3, 3, 63, ()), (capi.F64, 7, 4, 49, (2, 3)), (capi.F32, 1, 2, 50, (1, 7, 8, 30)),
              (capi.F64, 1, 3, 50, (49,))]


@pytest.mark.parametrize("prec,k,m,n_steps,drop", CONT_CASES)
def test_continuation_values_against_restarted_store_paths(ctx, prec, k, m, n_steps, drop):
    opt = capi.make_option(S0=37.0, T=1.0, v=0.3, **LS)
    am, coeffs = small_rule(ctx, opt, n_steps, prec, k, m, drop)
    beta, flags = unpack(coeffs)
    M, t, disc = ar.dates(opt.T, opt.r, n_steps, k)
    assert flags[:-1].sum() >= 3 and not flags[np.array(drop, dtype=int) - 1].any()
    n, offset, n_local, n_inner, outer_seed, inner_seed = 5000, 1003, 300, 300, 91, 92   # n_inner: a ragged second pass
    sim = capi.make_sim(n, n_steps, prec, seed=outer_seed, path_offset=offset, n_paths_local=n_local)
    dual = capi.make_american_dual(n_inner=n_inner, inner_seed=inner_seed)
    res, Q = bound(ctx, opt, sim, am, dual, coeffs)
    assert np.isfinite(Q).all() and res.n == n_local and res.n_dates == M and res.block == 256
    assert res.grid == min(M * n_local, 8192)
    rows = stored_rows(ctx, opt, n, n_steps, prec, outer_seed, offset, n_local)
    rng = np.random.default_rng(n_steps)
    worst, stops, n_points = 0.0, set(), 0
    mid = [j for j in range(2, M - 1)]
    for j in sorted({0, 1, M - 1, *rng.choice(mid, size=min(3, len(mid)), replace=False)}):
        if j == 0:
            paths = [0, n_local - 1]   # every path starts at S0: two of them show two subsequence bases
        else:
            order = np.argsort(rows[j * k - 1])   # deepest in the money, deepest out, at the money, and some others
            atm = int(np.argmin(np.abs(rows[j * k - 1] - opt.K)))
            paths = sorted({int(order[0]), int(order[1]), int(order[-1]), atm, *map(int, rng.choice(n_local, 6))})
        for p in paths:
            S = opt.S0 if j == 0 else float(rows[j * k - 1, p])
            restart = capi.make_option(S0=opt.S0, T=opt.T, v=opt.v, Sk=0.0 if j == 0 else S, Tk=j * k, **LS)
            base = adr.subsequence_base(offset + p, j, M, n_inner)
            inner = stored_rows(ctx, restart, base + n_inner, n_steps, prec, inner_seed, base, n_inner,
                                n_sim=n_steps - j * k)
            y, stop = adr.follow(inner, j, opt.K, am.payoff == capi.PAYOFF_PUT, k, disc, beta, flags)
            want = y.sum() / n_inner
            err = abs(Q[j, p] - want) / max(abs(want), 1e-300) if want != 0.0 else abs(Q[j, p])
            worst = max(worst, err)
            stops.update(stop.tolist())
            n_points += 1
    print(f"{n_points} points, worst relative deviation {worst:.2e}, stop dates {len(stops)}")
    assert worst <= RTOL, worst
    assert not any(s in drop for s in stops) and len(stops) >= min(M, 6) // 2 and M in stops
    # every wavefront ran at least what its live lanes needed, and no more than every remaining step of every pass
    NB = 2 if prec == capi.F64 else 4
    cap = sum(n_local * -(-n_inner // 64) * 64 * (-(-(M - j) * k // NB) * NB) for j in range(M))
    assert 0 < res.live_steps <= res.work_steps <= cap, (res.live_steps, res.work_steps, cap)
    assert res.work_steps % 64 == 0 and res.live_steps % k == 0


@pytest.mark.parametrize("prec,k,m,n_steps,drop", [(capi.F64, 1, 3, 50, ()), (capi.F32, 3, 4, 63, (5,)),
                                                   (capi.F64, 5, 2, 50, (3, 4))])
def test_scan_against_numpy_on_the_stored_rows(ctx, prec, k, m, n_steps, drop):
    opt = capi.make_option(S0=37.0, T=1.0, v=0.3, **LS)
    am, coeffs = small_rule(ctx, opt, n_steps, prec, k, m, drop)
    beta, flags = unpack(coeffs)
    M, t, disc = ar.dates(opt.T, opt.r, n_steps, k)
    n, offset, n_local = 9000, 777, 3001   # twelve workgroups, the last one ragged
    sim = capi.make_sim(n, n_steps, prec, seed=191, path_offset=offset, n_paths_local=n_local)
    dual = capi.make_american_dual(n_inner=64, inner_seed=192)
    res, Q = bound(ctx, opt, sim, am, dual, coeffs)
    rows = stored_rows(ctx, opt, n, n_steps, prec, 191, offset, n_local)
    u = adr.scan(rows, Q, opt.K, True, k, disc, beta, flags)
    print(f"sum {res.sum!r} numpy {u.sum()!r}; sumsq {res.sumsq!r} numpy {(u * u).sum()!r}; sum_q0 {res.sum_q0!r} "
          f"numpy {Q[0].sum()!r}")
    assert math.isclose(res.sum, u.sum(), rel_tol=RTOL) and math.isclose(res.sumsq, (u * u).sum(), rel_tol=RTOL)
    assert math.isclose(res.sum_q0, Q[0].sum(), rel_tol=RTOL)
    assert math.isclose(res.upper, u.mean(), rel_tol=RTOL)
    assert math.isclose(res.std_err, u.std(ddof=1) / math.sqrt(n_local), rel_tol=1e-7)
    assert math.isclose(res.ci_hi, res.upper + 1.959963984540054 * res.std_err, rel_tol=1e-15)
    assert res.immediate_exercise == 0 and res.outer_ms > 0 and res.inner_ms > 0 and res.scan_ms > 0
    assert res.total_ms >= res.inner_ms
    # each u_p: a shard of one path returns it as its sum
    for p in (0, 1, 255, 256, 1500, n_local - 1):
        one, q1 = bound(ctx, opt, capi.make_sim(n, n_steps, prec, seed=191, path_offset=offset + p, n_paths_local=1),
                        am, dual, coeffs)
        assert np.array_equal(q1[:, 0], Q[:, p])
        assert math.isclose(one.sum, u[p], rel_tol=RTOL, abs_tol=1e-300), (p, one.sum, u[p])
        assert one.n == 1 and one.std_err == 0.0


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_one_date_is_the_european_value(ctx, prec):
    n_steps = 50
    opt = capi.make_option(S0=40.0, T=1.0, v=0.2, **LS)   # at the money: h(S0) = 0
    am = capi.make_american(exercise_every=n_steps, n_train=0)
    coeffs = np.full((1, 4), np.nan)
    coeffs[0, -1] = 0.0
    dual = capi.make_american_dual(n_inner=256, inner_seed=52)
    res, Q = bound(ctx, opt, capi.make_sim(4096, n_steps, prec, seed=51), am, dual, coeffs)
    assert Q.shape == (1, 4096) and res.n_dates == 1
    assert math.isclose(res.sum, Q[0].sum(), rel_tol=RTOL)
    assert res.sum == res.sum_q0   # bit for bit
    parity = capi.bs_call_f64(40.0, 40.0, 1.0, 0.06, 0.2) - 40.0 + 40.0 * math.exp(-0.06)
    print(f"upper {res.upper:.5f} se {res.std_err:.5f} parity put {parity:.5f}")
    assert res.std_err > 0 and abs(res.upper - parity) <= 4 * res.std_err, (res.upper, res.std_err, parity)


def test_repeatable_shardable_and_d_cont_optional(ctx):
    n_steps, k, prec = 50, 1, capi.F64
    opt = capi.make_option(S0=36.0, T=1.0, v=0.2, **LS)
    am, coeffs = small_rule(ctx, opt, n_steps, prec, k, 3)
    n = 2003
    dual = capi.make_american_dual(n_inner=100, inner_seed=7)
    whole, Q = bound(ctx, opt, capi.make_sim(n, n_steps, prec, seed=6), am, dual, coeffs)
    again, Q2 = bound(ctx, opt, capi.make_sim(n, n_steps, prec, seed=6), am, dual, coeffs)
    fields = ("sum", "sumsq", "sum_q0", "n", "upper", "std_err", "ci_hi", "work_steps", "live_steps", "n_dates", "grid")
    for f in fields:
        assert getattr(whole, f) == getattr(again, f), f
    assert Q.tobytes() == Q2.tobytes()
    without, none = bound(ctx, opt, capi.make_sim(n, n_steps, prec, seed=6), am, dual, coeffs, cont=False)
    assert none is None
    for f in fields:
        assert getattr(whole, f) == getattr(without, f), f
    for cuts in ((0, 800, n), (0, 123, 1301, n)):
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            r, q = bound(ctx, opt, capi.make_sim(n, n_steps, prec, seed=6, path_offset=lo, n_paths_local=hi - lo), am,
                         dual, coeffs)
            assert q.tobytes() == np.ascontiguousarray(Q[:, lo:hi]).tobytes()   # the same streams as the whole job
            parts.append(r)
        for f in ("sum", "sumsq", "sum_q0", "work_steps", "live_steps"):
            assert math.isclose(sum(getattr(p, f) for p in parts), getattr(whole, f), rel_tol=RTOL), f
        assert sum(p.n for p in parts) == n
    empty, _ = bound(ctx, opt, capi.make_sim(n, n_steps, prec, seed=6, n_paths_local=0), am, dual, coeffs, cont=False)
    assert empty.n == 0 and empty.sum == 0.0 and empty.upper == 0.0 and empty.grid == 0 and empty.total_ms == 0.0


def test_never_exercise_rule_gives_european_continuation_values(ctx):
    n_steps, k, n = 20, 2, 4096
    opt = capi.make_option(S0=38.0, T=1.0, v=0.25, **LS)
    am = capi.make_american(exercise_every=k, n_train=0)
    M, t, disc = ar.dates(opt.T, opt.r, n_steps, k)
    coeffs = np.full((M, 4), np.nan)
    coeffs[:, -1] = 0.0
    dual = capi.make_american_dual(n_inner=512, inner_seed=12)
    res, Q = bound(ctx, opt, capi.make_sim(n, n_steps, capi.F64, seed=11), am, dual, coeffs)
    rows = stored_rows(ctx, opt, n, n_steps, capi.F64, 11)
    # nobody stops early: every lane is live for every step its wavefront runs
    assert res.live_steps == res.work_steps == sum(n * 512 * (M - j) * k for j in range(M))
    for j in range(M):
        S = np.full(n, opt.S0) if j == 0 else rows[j * k - 1]
        d = 1.0 if j == 0 else disc[j - 1]
        dev = Q[j] - d * adr.bs_put(S, opt.K, opt.r, opt.v, opt.T - (0.0 if j == 0 else t[j - 1]))
        se = dev.std(ddof=1) / math.sqrt(n)
        assert abs(dev.mean()) <= 5 * se, (j, dev.mean(), se)
    u = adr.scan(rows, Q, opt.K, True, k, disc, coeffs[:, :-1], np.zeros(M, dtype=bool))
    assert math.isclose(res.sum, u.sum(), rel_tol=RTOL)


# ---- statistical -----------------------------------------------------------------------------------------------------

LS_TABLE = [(S0, v, T) for S0 in (36.0, 40.0, 44.0) for v in (0.2, 0.4) for T in (1.0, 2.0)]
N_OUTER, N_INNER = 4096, 256


@pytest.mark.parametrize("S0,v,T", LS_TABLE)
def test_bounds_bracket_the_tree(ctx, S0, v, T):
    n_steps = int(50 * T)   # 50 exercise dates per year
    opt = capi.make_option(S0=S0, T=T, v=v, **LS)
    am = capi.make_american(exercise_every=1, n_train=200_000, train_seed=31)
    low, coeffs = fit_rule(ctx, opt, n_steps, capi.F64, am)
    dual = capi.make_american_dual(n_inner=N_INNER, inner_seed=34)
    up, _ = bound(ctx, opt, capi.make_sim(N_OUTER, n_steps, capi.F64, seed=33), am, dual, coeffs, cont=False)
    tree = ar.crr_bermudan(S0, opt.K, opt.r, v, T, n_steps, per_date=200)
    print(f"BRACKET S0={S0} v={v} T={T} tree={tree:.4f} lower={low.price:.4f} se_low={low.std_err:.4f} "
          f"upper={up.upper:.4f} se_up={up.std_err:.4f} upper-tree={up.upper - tree:.4f} "
          f"upper-lower={up.upper - low.price:.4f} q0={up.sum_q0 / up.n:.4f} n_outer={N_OUTER} n_inner={N_INNER} "
          f"live/work={up.live_steps / up.work_steps:.3f} inner_ms={up.inner_ms:.1f}")
    assert up.upper + 4 * up.std_err >= tree, (up.upper, up.std_err, tree)
    assert low.price - 4 * low.std_err <= up.upper + 4 * up.std_err, (low.price, low.std_err, up.upper, up.std_err)
    assert up.immediate_exercise == 0 and up.n == N_OUTER


def test_the_fitted_rule_tightens_the_bound(ctx):
    n_steps = 50
    opt = capi.make_option(S0=36.0, T=1.0, v=0.2, **LS)
    am = capi.make_american(exercise_every=1, n_train=200_000, train_seed=31)
    _, coeffs = fit_rule(ctx, opt, n_steps, capi.F64, am)
    never = np.full_like(coeffs, np.nan)
    never[:, -1] = 0.0
    dual = capi.make_american_dual(n_inner=N_INNER, inner_seed=34)
    sim = capi.make_sim(N_OUTER, n_steps, capi.F64, seed=33)
    fitted, _ = bound(ctx, opt, sim, am, dual, coeffs, cont=False)
    european, _ = bound(ctx, opt, sim, am, dual, never, cont=False)
    gap = european.upper - fitted.upper
    se = math.hypot(european.std_err, fitted.std_err)
    print(f"RULE fitted={fitted.upper:.4f} ({fitted.std_err:.4f}) never={european.upper:.4f} ({european.std_err:.4f}) "
          f"gap={gap:.4f} = {gap / se:.1f} combined SE")
    assert gap > 4 * se, (fitted.upper, european.upper, se)


# Inner sample of the call test, from the size of the inner-noise bias, not from a run.  The price is the European one and
# the best rule never stops early, so u_p is about Q_0 + max(0, max_j (Z_j - Q_j - eps_j)) with eps_j the sampling error
# of Q_j: the dual estimate exceeds the price by the expected positive part of the noise over the time value
# g_j = Q_j - Z_j.  In the money, g_j ~ K (1 - e^{-r tau}) ~ 2.4 tau and sd(eps_j) ~ S v sqrt(tau / n_inner) ~
# 8 sqrt(tau / n_inner) (tau = T - t_j): their ratio 0.3 sqrt(tau n_inner) is smallest at the last dates.  A normal
# eps has E[(eps - g)+] = sd (phi(x) - x (1 - Phi(x))), x = g / sd.  n_inner = 256: tau = 0.02 gives x = 0.68,
# sd = 0.071, 0.010; tau = 0.04 gives x = 0.96, sd = 0.10, 0.009; tau = 0.06: 0.007 .. — a few cents in all once the
# maximum runs over the last ten dates, several times the 0.2 % (0.009) the bound allows.  n_inner = 2048: x = 1.92,
# sd = 0.025, 0.0003; x = 2.7, 0.00004 ..: below 0.001 in all, a ninth of the allowance.
N_INNER_CALL = 2048


def test_american_call_without_dividends_is_bounded_by_the_european_value(ctx):
    opt = capi.make_option(S0=40.0, T=1.0, v=0.2, **LS)
    am = capi.make_american(payoff=capi.PAYOFF_CALL, exercise_every=1, n_train=200_000, train_seed=41)
    _, coeffs = fit_rule(ctx, opt, 50, capi.F64, am)
    dual = capi.make_american_dual(n_inner=N_INNER_CALL, inner_seed=44)
    up, _ = bound(ctx, opt, capi.make_sim(N_OUTER, 50, capi.F64, seed=43), am, dual, coeffs, cont=False)
    bs = capi.bs_call_f64(40.0, 40.0, 1.0, 0.06, 0.2)
    print(f"CALL upper={up.upper:.4f} se={up.std_err:.4f} bs={bs:.4f} n_inner={N_INNER_CALL}")
    assert abs(up.upper - bs) <= 4 * up.std_err + 0.002 * bs, (up.upper, up.std_err, bs)
