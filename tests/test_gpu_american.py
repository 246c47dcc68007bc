"""GPU tests of the least-squares Monte Carlo pricer (mcamd_price_american).  Run with -m gpu on an MI355X.

  * restatement: the engine's stored trajectories (mcamd_simulate_trajectories, same Philox stream and product form)
    run through the numpy restatement of tests/american_restate.py: numpy's own regression reproduces the engine's
    continuation values (1e-9 of their scale), the same dates are regressed, and applying the engine's coefficients
    gives its in-sample and out-of-sample sums (1e-12 relative) and its early-exercise count exactly — at the
    flagship shape, over a matrix of payoff x exercise_every x n_basis x precision x step-count remainders, on jobs
    larger than the capped grids (the grid-stride loops stride), and on jobs where only some dates are regressed
    (by the count rule, by the pivot rule);
  * structure: the same paths in both passes give the same estimate; shards add up; two calls are bit-identical;
  * accuracy: the Bermudan put of Longstaff-Schwartz Table 1 against a CRR tree exercising at the same dates, and
    the known limits (American call without dividends, European exercise, deep out of the money, fp32 vs fp64)."""
import importlib
import math

import numpy as np
import pytest

import american_restate as ar

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

LS = dict(K=40.0, r=0.06)
TORCH_T = {capi.F64: torch.float64, capi.F32: torch.float32}


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


def run(ctx, opt, sim, am, coeffs=True):
    work = torch.empty(capi.american_workspace_bytes(am, sim), dtype=torch.uint8, device="cuda")
    return ctx.price_american(opt, sim, am, work, coeffs=coeffs)


def stored_rows(ctx, opt, n, n_steps, prec, seed, path_offset=0, n_local=None):
    n_local = n if n_local is None else n_local
    traj = torch.empty(n_local * n_steps, dtype=TORCH_T[prec], device="cuda")
    ctx.simulate_trajectories(opt, capi.make_sim(n, n_steps, prec, seed=seed, flags=capi.FLAG_PRODUCT_FORM,
                                                 path_offset=path_offset, n_paths_local=n_local), traj)
    return traj.view(n_steps, n_local).cpu().numpy().astype(np.float64)


def unpack(coeffs):
    return coeffs[:, :-1], coeffs[:, -1] != 0


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_sweep_and_pricing_restate_exactly(ctx, prec):
    n_steps, k, m = 50, 1, 3
    opt = capi.make_option(S0=38.0, T=1.0, v=0.25, **LS)
    am = capi.make_american(exercise_every=k, n_train=200_000, train_seed=777)
    sim = capi.make_sim(150_001, n_steps, prec, seed=778)
    res, coeffs = run(ctx, opt, sim, am)
    beta, flags = unpack(coeffs)
    M, t, disc = ar.dates(opt.T, opt.r, n_steps, k)
    assert res.n_dates == M == 50 and coeffs.shape == (M, m + 1) and not flags[-1]
    assert np.isnan(beta[~flags]).all() and np.isfinite(beta[flags]).all()
    assert res.n_regressed == flags[:-1].sum() == M - 1 and res.n_train == 200_000 and res.n == 150_001

    # 1. the sweep: numpy's own regression at every date, given the engine's decisions at later dates
    rows = stored_rows(ctx, opt, am.n_train, n_steps, prec, am.train_seed)
    V, per_date = ar.sweep(rows, opt.K, True, k, m, disc, beta, flags)
    for j, ok, itm, c_np, c_gpu in per_date:
        assert ok == flags[j - 1], j
        if ok:
            scale = np.abs(c_gpu).max()
            assert np.abs(c_np - c_gpu).max() <= 1e-9 * scale, (j, np.abs(c_np - c_gpu).max(), scale)
    assert math.isclose(res.in_sample_sum, V.sum(), rel_tol=1e-12), (res.in_sample_sum, V.sum())
    assert math.isclose(res.in_sample_sumsq, (V * V).sum(), rel_tol=1e-12)
    assert math.isclose(res.in_sample_price, V.mean(), rel_tol=1e-12)

    # 2. the pricing pass: the engine's rule applied to the job's own stored paths
    rows = stored_rows(ctx, opt, sim.n_paths, n_steps, prec, sim.seed)
    y, ex_date, t_ex, margin = ar.forward(rows, opt.K, True, k, m, disc, t, beta, flags)
    assert margin > 1e-12, margin   # no decision within rounding of its boundary: the counts must then agree
    assert math.isclose(res.sum, y.sum(), rel_tol=1e-12) and math.isclose(res.sumsq, (y * y).sum(), rel_tol=1e-12)
    assert res.n_early == int((ex_date > 0).sum()) > 0
    assert math.isclose(res.sum_t_exercise, t_ex.sum(), rel_tol=1e-12)
    assert math.isclose(res.price, y.mean(), rel_tol=1e-12)
    assert math.isclose(res.std_err, y.std(ddof=1) / math.sqrt(y.size), rel_tol=1e-8)
    assert res.ci_lo < res.price < res.ci_hi and res.immediate_exercise == 0
    assert res.train_ms > 0 and res.price_ms > 0 and res.total_ms >= res.price_ms and res.block == 256
    # low-biased out of sample, high-biased in sample: the two bracket each other within a few SE
    assert abs(res.price - res.in_sample_price) < 5 * (res.std_err + res.in_sample_std_err)


def restate(ctx, opt, sim, am):
    """The assertions of test_sweep_and_pricing_restate_exactly for any job: the engine's table and sums against the
    restatement of its own stored paths.  A date is expected regressed when |I_j| >= 4m and the exact smallest scaled
    pivot of its restated record is above the threshold; a date whose exact pivot lies in ar.BAND (the engine's own
    pivot is a rounded one) may go either way and is counted.  Coefficients: 1e-9 of the scale of the continuation
    values, and C 2^-53 / pivot where that is larger (pivots below 2e-6; the bound of the solver's accuracy ladder,
    tests/test_gpu_american_solver.py).  Returns what the callers assert their preconditions on."""
    n_steps, prec, k = sim.n_steps, sim.precision, am.exercise_every
    m, put = am.n_basis or 3, am.payoff == capi.PAYOFF_PUT
    res, coeffs = run(ctx, opt, sim, am)
    beta, flags = unpack(coeffs)
    M, t, disc = ar.dates(opt.T, opt.r, n_steps, k)
    assert res.n_dates == M == n_steps // k and coeffs.shape == (M, m + 1) and not flags[-1]
    assert np.isnan(beta[~flags]).all() and np.isfinite(beta[flags]).all()
    assert res.n_regressed == flags[:-1].sum() and res.n_train == am.n_train and res.n == sim.n_paths_local
    assert res.grid == min(-(-sim.n_paths_local // 256), 8192) and res.train_grid == min(-(-am.n_train // 256), 8192)

    rows = stored_rows(ctx, opt, am.n_train, n_steps, prec, am.train_seed)
    pivots, band = {}, []
    V, per_date = ar.sweep(rows, opt.K, put, k, m, disc, beta, flags, pivots)
    for j, ok, itm, c_np, c_gpu in per_date:
        n_itm, piv = pivots[j]
        if piv is not None and ar.BAND[0] <= piv <= ar.BAND[1]:
            band.append(j)
            continue
        assert ok == flags[j - 1], (j, n_itm, piv, flags[j - 1])
        if ok:
            scale = np.abs(c_gpu).max()
            tol = max(1e-9, ar.C_DEVICE * ar.EPS / piv)
            assert np.abs(c_np - c_gpu).max() <= tol * scale, (j, piv, np.abs(c_np - c_gpu).max(), scale)
    assert math.isclose(res.in_sample_sum, V.sum(), rel_tol=1e-12), (res.in_sample_sum, V.sum())
    assert math.isclose(res.in_sample_sumsq, (V * V).sum(), rel_tol=1e-12)

    rows = stored_rows(ctx, opt, sim.n_paths, n_steps, prec, sim.seed, sim.path_offset, sim.n_paths_local)
    y, ex_date, t_ex, margin = ar.forward(rows, opt.K, put, k, m, disc, t, beta, flags)
    assert margin > 1e-12, margin   # no decision within rounding of its boundary: the counts must then agree
    assert math.isclose(res.sum, y.sum(), rel_tol=1e-12), (res.sum, y.sum())
    assert math.isclose(res.sumsq, (y * y).sum(), rel_tol=1e-12)
    assert res.n_early == int((ex_date > 0).sum())
    assert math.isclose(res.sum_t_exercise, t_ex.sum(), rel_tol=1e-12, abs_tol=0.0 if res.n_early else 1e-300)
    assert flags[ex_date[ex_date > 0] - 1].all()   # nobody exercises at a date that is not regressed
    return dict(res=res, flags=flags, pivots=pivots, band=band, ex_date=ex_date, y=y)


PUT, CALL = capi.PAYOFF_PUT, capi.PAYOFF_CALL
assert (capi.F64, capi.F32) == (64, 32)
# what the matrix covers is checked on every CPU run (tests/test_american_solver_cpu.py)
SHAPES = [(PUT if put else CALL, k, m, prec, n_steps) for put, k, m, prec, n_steps in ar.SHAPES]


@pytest.mark.parametrize("payoff,k,m,prec,n_steps", SHAPES)
def test_shape_matrix_restates_exactly(ctx, payoff, k, m, prec, n_steps):
    # in the money either way, so that most dates are regressed and paths do stop early
    opt = capi.make_option(S0=37.0 if payoff == PUT else 43.0, T=1.0, v=0.3, **LS)
    am = capi.make_american(payoff=payoff, exercise_every=k, n_basis=m, n_train=60_000, train_seed=1000 + n_steps)
    out = restate(ctx, opt, capi.make_sim(50_001, n_steps, prec, seed=2000 + n_steps), am)
    assert out["flags"][:-1].all() and not out["band"]
    if payoff == PUT:
        assert out["res"].n_early > 0.2 * out["res"].n
        assert len(np.unique(out["ex_date"])) > min(n_steps // k, 8) // 2   # exercise spread over the dates


@pytest.mark.parametrize("prec,k", [(capi.F64, 1), (capi.F32, 3)])
def test_grids_that_stride_restate_exactly(ctx, prec, k):
    # both capped grids (8192 workgroups of 256) loop: a second, ragged trip in the sweep and in the pricing pass
    n_train, n_local, offset = 2_300_017, 4_200_011, 1_000_003
    assert min(n_train, n_local) > 8192 * 256 and all(n % 256 and n % 64 for n in (n_train, n_local))
    opt = capi.make_option(S0=38.0, T=1.0, v=0.25, **LS)
    am = capi.make_american(exercise_every=k, n_train=n_train, train_seed=91)
    sim = capi.make_sim(offset + n_local + 12_345, 12, prec, seed=92, path_offset=offset, n_paths_local=n_local)
    assert capi.american_workspace_bytes(am, sim) < 300e6
    out = restate(ctx, opt, sim, am)
    assert out["res"].grid == out["res"].train_grid == 8192
    assert out["flags"][:-1].all() and out["res"].n_early > 0.1 * n_local
    # the second trip's paths exercise like the first's
    early = out["ex_date"] > 0
    assert abs(early[8192 * 256:].mean() - early[:8192 * 256].mean()) < 0.01


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_count_rule_leaves_some_dates_out(ctx, prec):
    """An out-of-the-money put: the first dates have no or few training paths in the money.  Dates with fewer than 4m
    are not regressed and the pricing pass walks past them; the first regressed ones fit a dozen points."""
    m = 3
    opt = capi.make_option(S0=50.0, T=1.0, v=0.2, **LS)
    am = capi.make_american(exercise_every=1, n_basis=m, n_train=100_000, train_seed=301)
    out = restate(ctx, opt, capi.make_sim(400_003, 100, prec, seed=302), am)
    counts = {j: n for j, (n, _) in out["pivots"].items()}
    few = [j for j, n in counts.items() if 0 < n < 4 * m]
    small = [j for j, n in counts.items() if 4 * m <= n < 100]
    assert few and small and any(n == 0 for n in counts.values()), sorted(counts.items())[:20]
    assert not out["flags"][np.array(few) - 1].any() and out["flags"][np.array(small) - 1].all()
    assert not out["band"] and 0 < out["res"].n_early and out["res"].immediate_exercise == 0
    assert out["res"].n_regressed == sum(n >= 4 * m for n in counts.values())


# v places the j^3 ladder of pivots with dates 1 and 2 below the band, date 3 in it and date 4 above (numpy paths of
# the same law give 4.2e-12, 3.3e-11, 1.1e-10, 2.8e-10 at dates 1..4; the test asserts what the engine's paths give)
PIVOT_JOB = dict(S0=30.0, v=0.0443, n_steps=200, n_train=50_000)


def test_pivot_rule_leaves_some_dates_out(ctx):
    """A deep in-the-money, low-volatility put with 200 dates and four basis functions: every training path is in the
    money at every date, and at the first dates the prices sit so close together (u = -0.25 +- a few 1e-3, some 50 000 of them) that the
    scaled pivot is below the threshold.  The smallest pivot grows like j^3 from date to date, by less than the
    band's factor 4 from the second date on, so no choice of volatility or seed keeps every date out of the band
    [0.5, 2] x threshold and has two dates below it: dates in the band may go either way (as in the solver's ladder),
    and at most 2 % of the dates may lie there."""
    m, n_steps = 4, PIVOT_JOB["n_steps"]
    opt = capi.make_option(S0=PIVOT_JOB["S0"], T=1.0, v=PIVOT_JOB["v"], **LS)
    am = capi.make_american(exercise_every=1, n_basis=m, n_train=PIVOT_JOB["n_train"], train_seed=401)
    out = restate(ctx, opt, capi.make_sim(100_003, n_steps, capi.F64, seed=402), am)
    piv = out["pivots"]
    assert all(n == am.n_train for n, _ in piv.values())   # the count rule plays no part
    below = [j for j, (_, p) in piv.items() if p < ar.BAND[0]]
    above = [j for j, (_, p) in piv.items() if p > ar.BAND[1]]
    assert len(below) >= 2 and len(above) >= 20 and len(out["band"]) <= 0.02 * (n_steps - 1), \
        (len(below), len(above), out["band"])
    assert not out["flags"][np.array(below) - 1].any() and out["flags"][np.array(above) - 1].all()
    # some regressed dates are close enough to the threshold for the accuracy bound to be the one that is applied
    assert sum(piv[j][1] < 2e-6 for j in above) >= 3
    # a threshold ten times higher would be noticed: it would leave out a date that is regressed here
    assert sum(piv[j][1] < 0.5e-9 for j in above) >= 1, sorted(piv.items())[:8]
    res = out["res"]
    assert res.immediate_exercise == 1 and res.price == 10.0
    # whole wavefronts stop at the first regressed date, long before the last Philox block
    assert res.n_early > 0.9 * res.n and np.median(out["ex_date"]) < n_steps // 4


@pytest.mark.parametrize("prec,k,payoff", [(capi.F64, 1, capi.PAYOFF_PUT), (capi.F32, 5, capi.PAYOFF_PUT),
                                           (capi.F64, 4, capi.PAYOFF_CALL)])
def test_same_paths_give_the_in_sample_estimate(ctx, prec, k, payoff):
    n = 300_007
    opt = capi.make_option(S0=40.0, T=1.0, v=0.3, **LS)
    am = capi.make_american(payoff=payoff, exercise_every=k, n_train=n, train_seed=2024)
    res, _ = run(ctx, opt, capi.make_sim(n, 100, prec, seed=2024), am)
    assert math.isclose(res.sum, res.in_sample_sum, rel_tol=1e-12), (res.sum, res.in_sample_sum)
    assert math.isclose(res.sumsq, res.in_sample_sumsq, rel_tol=1e-12)
    assert math.isclose(res.price, res.in_sample_price, rel_tol=1e-12)


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_shards_add_up_to_the_whole_job(ctx, prec):
    n, n_steps = 1_000_003, 50
    opt = capi.make_option(S0=36.0, T=1.0, v=0.2, **LS)
    am = capi.make_american(exercise_every=1, n_train=100_000, train_seed=5)
    whole, c0 = run(ctx, opt, capi.make_sim(n, n_steps, prec, seed=6), am)
    for cuts in ((0, 400_000, n), (0, 123_457, 777_777, n)):
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            r, c = run(ctx, opt, capi.make_sim(n, n_steps, prec, seed=6, path_offset=lo, n_paths_local=hi - lo), am)
            assert np.array_equal(c, c0, equal_nan=True)   # every shard trains identically
            parts.append(r)
        assert math.isclose(sum(p.sum for p in parts), whole.sum, rel_tol=1e-12)
        assert math.isclose(sum(p.sumsq for p in parts), whole.sumsq, rel_tol=1e-12)
        assert math.isclose(sum(p.sum_t_exercise for p in parts), whole.sum_t_exercise, rel_tol=1e-12)
        assert sum(p.n_early for p in parts) == whole.n_early and sum(p.n for p in parts) == n
    empty, c = run(ctx, opt, capi.make_sim(n, n_steps, prec, seed=6, n_paths_local=0), am)
    assert empty.n == 0 and empty.sum == 0.0 and empty.price == 0.0 and empty.grid == 0
    assert empty.in_sample_sum == whole.in_sample_sum and np.array_equal(c, c0, equal_nan=True)


def test_two_calls_are_bit_identical(ctx):
    opt = capi.make_option(S0=40.0, T=2.0, v=0.4, **LS)
    am = capi.make_american(exercise_every=2, n_basis=4, n_train=250_000, train_seed=9)
    sim = capi.make_sim(2_000_000, 100, capi.F64, seed=10)
    a, ca = run(ctx, opt, sim, am)
    b, cb = run(ctx, opt, sim, am)
    for f in ("sum", "sumsq", "n_early", "sum_t_exercise", "in_sample_sum", "in_sample_sumsq", "n_regressed", "price"):
        assert getattr(a, f) == getattr(b, f), f
    assert ca.shape == (50, 5) and ca.tobytes() == cb.tobytes()


LS_TABLE = [(S0, v, T) for S0 in (36.0, 40.0, 44.0) for v in (0.2, 0.4) for T in (1.0, 2.0)]


@pytest.mark.parametrize("S0,v,T", LS_TABLE)
def test_bermudan_put_against_a_tree(ctx, S0, v, T):
    n_steps = int(50 * T)   # 50 exercise dates per year
    opt = capi.make_option(S0=S0, T=T, v=v, **LS)
    am = capi.make_american(exercise_every=1, n_train=200_000, train_seed=31)
    res = run(ctx, opt, capi.make_sim(2_000_000, n_steps, capi.F64, seed=32), am, coeffs=False)
    tree = ar.crr_bermudan(S0, opt.K, opt.r, v, T, n_steps, per_date=200)
    assert res.price <= tree + 4 * res.std_err + 2e-3, (res.price, res.std_err, tree)
    assert res.price >= tree - 4 * res.std_err - 0.005 * tree, (res.price, res.std_err, tree)
    assert res.n_early > 0 and res.immediate_exercise == 0


def test_american_call_without_dividends_is_european(ctx):
    opt = capi.make_option(S0=40.0, T=1.0, v=0.2, **LS)
    am = capi.make_american(payoff=capi.PAYOFF_CALL, exercise_every=1, n_train=200_000, train_seed=41)
    res = run(ctx, opt, capi.make_sim(2_000_000, 50, capi.F64, seed=42), am, coeffs=False)
    bs = capi.bs_call_f64(40.0, 40.0, 1.0, 0.06, 0.2)
    assert abs(res.price - bs) <= 4 * res.std_err + 0.002 * bs, (res.price, res.std_err, bs)
    assert res.n_early < 0.1 * res.n, res.n_early


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_european_exercise_is_the_parity_put(ctx, prec):
    # at the money: h(S0) = 0, so the t = 0 rule leaves the European value alone (S0 = 36 would report h(S0) = 4 > 3.84)
    opt = capi.make_option(S0=40.0, T=1.0, v=0.2, **LS)
    am = capi.make_american(exercise_every=50, n_train=50_000, train_seed=51)
    res, coeffs = run(ctx, opt, capi.make_sim(2_000_000, 50, prec, seed=52), am)
    parity = capi.bs_call_f64(40.0, 40.0, 1.0, 0.06, 0.2) - 40.0 + 40.0 * math.exp(-0.06)
    assert abs(res.price - parity) <= 4 * res.std_err, (res.price, res.std_err, parity)
    assert res.n_dates == 1 and res.n_regressed == 0 and res.n_early == 0 and coeffs.shape == (1, 4)
    assert res.immediate_exercise == 0 and res.std_err > 0
    assert coeffs[0, -1] == 0 and np.isnan(coeffs[0, :-1]).all()


def test_deep_out_of_the_money_put_has_nothing_to_regress(ctx):
    opt = capi.make_option(S0=200.0, T=1.0, v=0.2, **LS)
    am = capi.make_american(exercise_every=1, n_train=100_000, train_seed=61)
    res, coeffs = run(ctx, opt, capi.make_sim(1_000_000, 50, capi.F64, seed=62), am)
    assert res.n_regressed == 0 and (coeffs[:, -1] == 0).all() and np.isnan(coeffs[:, :-1]).all()
    assert res.price < 1e-9 and res.in_sample_price < 1e-9 and res.n_early == 0


def test_immediate_exercise_of_a_deep_in_the_money_put(ctx):
    opt = capi.make_option(S0=10.0, T=1.0, v=0.2, **LS)
    am = capi.make_american(exercise_every=5, n_train=100_000, train_seed=71)
    res = run(ctx, opt, capi.make_sim(500_000, 50, capi.F64, seed=72), am, coeffs=False)
    assert res.immediate_exercise == 1
    assert res.price == 30.0 and res.std_err == 0.0 and res.ci_lo == res.ci_hi == 30.0
    assert res.in_sample_price == 30.0 and res.in_sample_std_err == 0.0
    assert res.sum < 30.0 * res.n   # the raw sums stay the shard's, for adding shards


def test_fp32_and_fp64_agree(ctx):
    opt = capi.make_option(S0=36.0, T=1.0, v=0.2, **LS)
    am = capi.make_american(exercise_every=1, n_train=200_000, train_seed=81)
    sim = dict(n_paths=2_000_000, n_steps=50, seed=82)
    a = run(ctx, opt, capi.make_sim(precision=capi.F64, **sim), am, coeffs=False)
    b = run(ctx, opt, capi.make_sim(precision=capi.F32, **sim), am, coeffs=False)
    assert abs(a.price - b.price) <= 4 * math.hypot(a.std_err, b.std_err), (a.price, b.price)
