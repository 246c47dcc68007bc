"""GPU tests of the least-squares Monte Carlo pricer (mcamd_price_american).  Run with -m gpu on an MI355X.

  * restatement: the engine's stored trajectories (mcamd_simulate_trajectories, same Philox stream and product form)
    run through the numpy restatement of tests/american_restate.py: numpy's own regression reproduces the engine's
    continuation values (1e-9 of their scale), the same dates are regressed, and applying the engine's coefficients
    gives its in-sample and out-of-sample sums (1e-12 relative) and its early-exercise count exactly;
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


def stored_rows(ctx, opt, n, n_steps, prec, seed):
    traj = torch.empty(n * n_steps, dtype=TORCH_T[prec], device="cuda")
    ctx.simulate_trajectories(opt, capi.make_sim(n, n_steps, prec, seed=seed, flags=capi.FLAG_PRODUCT_FORM), traj)
    return traj.view(n_steps, n).cpu().numpy().astype(np.float64)


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
