"""GPU tests of the lookback pricer (mcamd_price_lookback).  Run with -m gpu on an MI355X.

  1. samples, elementwise through d_samples, against the numpy restatement (tests/lookback_restate.py) on normals and
     uniforms drawn from the oracle's rocRAND-exact generator for (seed, global path id, block / 2^63 + block): 50, 1, 3
     and 5 steps on 4096 paths at global ids 5003.. under seed 77, and 7 steps on the deep inputs, ids 2^33 + 5003.. of
     a job of 2^40 paths under seed 2^40 + 77.  The last, partial Philox block of a path is a branch of its own in the
     kernel, with its own block of uniforms: these step counts leave 2, 1, 3, 1 and 3 of its 4 steps in fp32 and 0, 1,
     1, 1 and 1 of its 2 in fp64;
  2. per-path identities on the GPU's own samples;  3. continuous monitoring against the closed form within 4 SE at
  n_steps 1, 12 and 252;  4. one discrete step is the European call struck at the spot;  5. shards;
  6. repeatability and the enqueue form;  7. the work counters;  8. flags and the empty shard.

Tolerance of 1 (compare / elementwise_tolerance below; it comes from the restatement alone, computed on the CPU): four
times the largest elementwise difference between the float64 and longdouble restatements (fp64 kernels), or between
the float32 and float64 restatements (fp32 kernels), over all 16 strike x payoff x monitoring x K cases on the test's
own inputs — S0 = 100, r = 0.1, v = 0.2, T = 1, K = 100 and, for the fixed strike, also 95 and 105; 50 steps, 4096
paths at global ids 5003.., seed 77 — floored at 1e-11 of the sample (fp64) and 2e-3 absolute (fp32).  Measured on an
x86-64 CPU (80-bit longdouble): 4 x 7.06e-14 = 2.8e-13 absolute for fp64; 4 x 5.06e-5 = 2.0e-4 for fp32, i.e. the
2e-3 floor decides there.  The sample is continuous in every input, so NO path is left out.  The tolerance is still
taken from the 50-step inputs alone.  On the other inputs of test 1 (MORE_INPUTS) the restatements differ by less — at most
6.4e-14 (fp64) and 4.5e-5 (fp32) — and disagree on no live count, which test_added_inputs_stay_under_the_spreads asserts
(it runs no kernel, but lives in this module and so runs with -m gpu).

The live counter (test 1 too): the kernel's lane-steps with q < Q against the restated count.  q is a product of two
differences, and a step whose q lies within rounding of Q can fall on either side; the restatements of two dtypes
(both with the kernel precision's Q) disagree on none of the 204 800 lane-steps of any case here, float64 against
longdouble and float32 against float64 alike.  The bound is four times the largest such disagreement over the cases of
the precision — the factor of the values — floored at 4 lane-steps, because no disagreement among 204 800 does not
exclude one."""
import importlib
import itertools
import math

import numpy as np
import pytest

import lookback_restate as lr
from deep_inputs import DEEP, SHALLOW, check_deep_draws_differ

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

NP_T = {capi.F64: np.float64, capi.F32: np.float32}
SUM_RTOL = {capi.F64: 1e-11, capi.F32: 2e-5}
BASE = dict(S0=100.0, r=0.1, v=0.2, T=1.0)
N_JOB, OFFSET, N_LOCAL, N_STEPS, SEED = 20_000, 5003, 4096, 50, 77
assert SHALLOW == (SEED, OFFSET, N_JOB)   # (seed, first path, paths of the job); DEEP: tests/deep_inputs.py
MORE_INPUTS = ((1, SHALLOW), (3, SHALLOW), (5, SHALLOW), (7, DEEP))          # (n_steps, where) beside (N_STEPS, SHALLOW)
PRECS = (capi.F64, capi.F32)


def option(K=100.0, **kw):
    return capi.make_option(**dict(BASE, K=K, **kw))


_draws = {}


def draws(prec, seed, first, n, n_steps):
    """([n_steps, n] normals, [n_steps, n] uniforms) of global paths first..first+n-1, as the kernels draw them (as
    float64 values): the normals from Philox blocks 0, 1, .., the uniforms from blocks 2^63, 2^63 + 1, .."""
    from oracle import pyoracle as o
    key = (prec, seed, first, n, n_steps)
    if key not in _draws:
        per, draw = (2, o.normal2_f64) if prec == capi.F64 else (4, o.normal4_f32)
        blocks = -(-n_steps // per)
        z = np.empty((blocks * per, n))
        u = np.empty((blocks * per, n))
        for p in range(n):
            for k in range(blocks):
                z[k * per:(k + 1) * per, p] = draw(seed, first + p, k)
                w = o.philox(seed, first + p, 2 ** 63 + k)
                if prec == capi.F64:
                    x, y, zz, ww = (int(v) for v in w)
                    u[2 * k, p] = ((x ^ (y << 21)) + 1) * 2.0 ** -53      # exact: at most 53 bits
                    u[2 * k + 1, p] = ((zz ^ (ww << 21)) + 1) * 2.0 ** -53
                else:   # float(word) 2^-32 is exact, so the sum rounds once, as the fused multiply-add does
                    u[4 * k:4 * k + 4, p] = w.astype(np.float32) * np.float32(2.0 ** -32) + np.float32(2.0 ** -32)
        _draws[key] = (z[:n_steps], u[:n_steps])
    return _draws[key]


def restate(prec, strike, payoff, monitoring, K, z, u, dtype=None):
    dtype = dtype or NP_T[prec]   # whatever the dtype, Q is the kernel precision's
    return lr.samples(z, u, BASE["S0"], K, BASE["T"], BASE["r"], BASE["v"], strike, payoff, monitoring, dtype,
                      lr.Q_CUT[np.dtype(NP_T[prec])])


def compare(prec, strike, payoff, monitoring, K, z, u):
    """(restated samples to compare with, restatement in the kernel's precision, largest difference between the two
    restatements the tolerance is taken from, lane-steps on whose q < Q the two restatements disagree) — CPU only"""
    own = restate(prec, strike, payoff, monitoring, K, z, u)
    other = restate(prec, strike, payoff, monitoring, K, z, u, np.longdouble if prec == capi.F64 else np.float64)
    spread = float(np.abs(own["y"] - other["y"]).max())
    flips = int(np.abs(own["live"] - other["live"]).sum())
    # an fp64 kernel is compared with the float64 restatement, an fp32 kernel with the float64 one too
    want = own["y"] if prec == capi.F64 else other["y"]
    return np.asarray(want, dtype=np.float64), own, spread, flips


PRODUCT_CASES = [(strike, payoff, monitoring, K)
                 for (strike, payoff), monitoring in itertools.product(lr.PRODUCTS, (lr.DISCRETE, lr.CONTINUOUS))
                 for K in ((100.0, 95.0, 105.0) if strike == lr.FIXED else (100.0,))]
CASES = [(prec,) + c for prec in PRECS for c in PRODUCT_CASES]


def _name(case, n_steps, where):
    return "-".join(str(x) for x in case) + f"-{n_steps}" + ("-deep" if where == DEEP else "")


# the ids of the 50-step cases are those pytest gave them before there were others
SAMPLE_CASES = [pytest.param(*c, N_STEPS, SHALLOW, id="-".join(str(x) for x in c)) for c in CASES] + \
               [pytest.param(*c, n_steps, where, id=_name(c, n_steps, where)) for n_steps, where in MORE_INPUTS for c in CASES]

_spread = {}


def measured(prec):
    """(largest restatement difference, largest disagreement on the live count) over the cases of test 1's inputs"""
    if prec not in _spread:
        z, u = draws(prec, SEED, OFFSET, N_LOCAL, N_STEPS)
        rows = [compare(prec, *case, z, u)[2:] for case in PRODUCT_CASES]
        _spread[prec] = (max(r[0] for r in rows), max(r[1] for r in rows))
    return _spread[prec]


def elementwise_tolerance(prec, want):
    """Absolute tolerance per element: 4 x the largest restatement difference over the cases of test 1's inputs,
    floored at 1e-11 of the sample (fp64) / 2e-3 (fp32).  From the restatement alone."""
    spread = measured(prec)[0]
    if prec == capi.F64:
        return np.maximum(4.0 * spread, 1e-11 * np.abs(want))
    return np.full(want.shape, max(4.0 * spread, 2e-3))


def live_tolerance(prec):
    return max(4 * measured(prec)[1], 4)


def test_restatement_spreads():
    """no kernel runs: prints what the tolerances of test 1 are made of"""
    for prec in PRECS:
        spread, flips = measured(prec)
        print(f"prec {prec}: largest restatement difference {spread:.3e}, largest live-count disagreement {flips}")
        assert spread > 0 and flips <= 64


def test_added_inputs_stay_under_the_spreads():
    """no kernel runs: on MORE_INPUTS the two restatements differ by no more than on the inputs the tolerance is taken
    from, and four times their disagreement on a live count stays within the bound on the kernel's"""
    for n_steps, where in MORE_INPUTS:
        worst = {}
        for prec, *case in CASES:
            z, u = draws(prec, where[0], where[1], N_LOCAL, n_steps)
            want, own, spread, flips = compare(prec, *case, z, u)
            assert np.isfinite(want).all() and spread <= measured(prec)[0], (n_steps, where, prec, case, spread)
            assert 4 * flips <= live_tolerance(prec), (n_steps, where, prec, case, flips)
            worst[prec] = max(worst.get(prec, (0.0, 0)), (spread, flips))
        print(f"n_steps {n_steps} first path {where[1]}: largest restatement difference and live-count disagreement "
              f"{worst[capi.F64]} (fp64; the tolerance's {measured(capi.F64)}) {worst[capi.F32]} (fp32; {measured(capi.F32)})")


@pytest.mark.parametrize("prec", PRECS)
def test_deep_draws_are_those_of_neither_shallow_word(prec):
    """no kernel runs.  What makes the deep cases worth running: the deep normals and uniforms share nothing with the
    streams a dropped high word of the path id or of the seed lands on (tests/deep_inputs.py)."""
    check_deep_draws_differ(lambda seed, first: draws(prec, seed, first, 64, 7))


torch = pytest.importorskip("torch")
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


def run(ctx, opt, sim, lb, want_samples=True):
    """(result, samples as float64 numpy or None)"""
    s = None
    if want_samples:
        s = torch.full((max(sim.n_paths_local, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    res = ctx.price_lookback(opt, sim, lb, s)
    torch.cuda.synchronize()
    return res, (s[:sim.n_paths_local].cpu().numpy().astype(np.float64) if want_samples else None)


def full_work(n, n_steps):
    return 64 * -(-n // 64) * n_steps


def terminal_prices(ctx, sim, K=100.0):
    """(S_T, (S_T - K)+) per path from mcamd_simulate_trajectories (the product-form store kernel), as float64"""
    n, steps = sim.n_paths_local, sim.n_steps
    traj = torch.empty(n * steps, dtype=TORCH_T[sim.precision], device="cuda")
    cnt = torch.empty(n * steps, dtype=torch.int32, device="cuda")
    pay = torch.empty(n, dtype=TORCH_T[sim.precision], device="cuda")
    ctx.simulate_trajectories(option(K), sim, traj, cnt, pay)
    torch.cuda.synchronize()
    return (traj.view(steps, n)[-1].cpu().numpy().astype(np.float64), pay.cpu().numpy().astype(np.float64))


# ---- 1. samples against the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec,strike,payoff,monitoring,K,n_steps,where", SAMPLE_CASES)
def test_samples_against_the_restatement(ctx, prec, strike, payoff, monitoring, K, n_steps, where):
    seed, first, n_job = where
    z, u = draws(prec, seed, first, N_LOCAL, n_steps)
    want, own, spread, flips = compare(prec, strike, payoff, monitoring, K, z, u)
    tol = elementwise_tolerance(prec, want)
    sim = capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=N_LOCAL)
    res, got = run(ctx, option(K), sim, capi.make_lookback(strike, payoff, monitoring))
    assert np.isfinite(got).all() and res.n == N_LOCAL and res.block == 256 and res.grid == N_LOCAL // 256
    err = np.abs(got - want)
    k = int(np.argmax(err - tol))
    want_live = int(own["live"].sum())
    print(f"prec {prec} strike {strike} payoff {payoff} monitoring {monitoring} K {K} n_steps {n_steps} first path {first}: "
          f"restatement spread {spread:.3e}, "
          f"tolerance {tol.min():.3e}..{tol.max():.3e}, worst deviation {err.max():.3e}, "
          f"nonzero samples {(want != 0).mean():.3f}, live {res.live_steps:.0f} restated {want_live} "
          f"(restatements disagree on {flips}, bound {live_tolerance(prec)})")
    assert (err <= tol).all(), (k, got[k], want[k], tol[k])   # every path: nothing is left out
    # not a vacuous comparison (the restatement's own samples).  One discrete step of the fixed put struck at 95 pays
    # where S_1 < 95 only, with probability N((ln 0.95 - 0.08) / 0.2) = 0.256: 0.2 is 8 standard errors of 4096 paths below
    assert (0.3 if n_steps > 1 else 0.2) < (want != 0).mean()
    ref = np.asarray(own["y"], dtype=np.float64)
    rt = SUM_RTOL[prec]
    assert abs(res.sum - ref.sum()) <= rt * abs(ref.sum()), (res.sum, ref.sum())
    assert abs(res.sumsq - (ref * ref).sum()) <= rt * (ref * ref).sum()
    fin = capi.finalize(res.sum, res.sumsq, res.n, BASE["r"], BASE["T"])
    assert (res.price, res.std_err, res.ci_lo, res.ci_hi) == (fin.price, fin.std_err, fin.ci_lo, fin.ci_hi)
    assert res.sum_c == res.sum_cc == res.sum_yc == res.cv_beta == res.cv_rho == 0.0
    # 7 (the half that needs the restatement): the counters
    assert res.work_steps == full_work(N_LOCAL, n_steps)
    if monitoring == lr.DISCRETE:
        assert res.live_steps == 0.0
    else:
        # the first step has q = 0 (E_0 = X_0, so one of the two distances is 0): every lane forms its bridge extremum
        assert 0 < want_live and (want_live < N_LOCAL * n_steps) == (n_steps > 1)
        assert abs(res.live_steps - want_live) <= live_tolerance(prec)


# ---- 2. identities on the GPU's own samples ----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("monitoring", [lr.DISCRETE, lr.CONTINUOUS])
def test_per_path_identities(ctx, prec, monitoring):
    """Tolerances: each sample is an fp64 difference of two path-precision prices rounded once to the path precision,
    and S_T comes from the store kernel, which multiplies step factors where the lookback kernel adds exponents: the
    project's agreement between those two forms, 1e-11 of the price (fp64) / 2e-3 absolute (fp32)."""
    n, n_steps = 50_000, 50
    sim = capi.make_sim(n, n_steps, prec, seed=21)
    S0 = BASE["S0"]
    S_T, _ = terminal_prices(ctx, sim)
    tol = 1e-11 * np.maximum(S_T, S0) if prec == capi.F64 else np.full(n, 2e-3)
    _, flo_put = run(ctx, option(), sim, capi.make_lookback(lr.FLOATING, lr.PUT, monitoring))
    _, flo_call = run(ctx, option(), sim, capi.make_lookback(lr.FLOATING, lr.CALL, monitoring))
    assert (flo_put >= 0).all() and (flo_call >= 0).all() and (flo_put > 0).any() and (flo_call > 0).any()
    for K in (100.0, 90.0):      # K <= S0: S_max >= K on every path
        _, fix_call = run(ctx, option(K), sim, capi.make_lookback(lr.FIXED, lr.CALL, monitoring))
        assert (np.abs(fix_call - flo_put - (S_T - K)) <= 2 * tol).all()
    for K in (100.0, 115.0):     # K >= S0: S_min <= K on every path
        _, fix_put = run(ctx, option(K), sim, capi.make_lookback(lr.FIXED, lr.PUT, monitoring))
        assert (np.abs(fix_put - flo_call - (K - S_T)) <= 2 * tol).all()
    # S_max = floating put + S_T >= max(S0, S_T) and S_min <= min(S0, S_T): exactly so in the kernel's own arithmetic
    # (a fixed strike at the spot pays S_max - S0 >= 0 and S0 - S_min >= 0), to tolerance through the store kernel's S_T
    _, up = run(ctx, option(S0), sim, capi.make_lookback(lr.FIXED, lr.CALL, monitoring))
    _, down = run(ctx, option(S0), sim, capi.make_lookback(lr.FIXED, lr.PUT, monitoring))
    assert (up >= 0).all() and (down >= 0).all()
    assert (up + S0 >= S_T - tol).all() and (S0 - down <= S_T + tol).all()
    if monitoring == lr.CONTINUOUS:
        # continuous S_max >= discrete S_max, continuous S_min <= discrete S_min, sample for sample
        for strike, payoff in lr.PRODUCTS:
            _, c = run(ctx, option(), sim, capi.make_lookback(strike, payoff, lr.CONTINUOUS))
            _, d = run(ctx, option(), sim, capi.make_lookback(strike, payoff, lr.DISCRETE))
            assert (c >= d).all() and (c > d).mean() > 0.5


# ---- 3. the closed form ------------------------------------------------------------------------------------------------------

CLOSED = [(prec, strike, payoff, K, n_steps) for prec in PRECS for strike, payoff in lr.PRODUCTS
          for K in (90.0, 100.0, 110.0) for n_steps in (1, 12, 252)]


@pytest.mark.parametrize("prec,strike,payoff,K,n_steps", CLOSED)
def test_continuous_monitoring_against_the_closed_form(ctx, prec, strike, payoff, K, n_steps):
    n = 4_000_000
    sim = capi.make_sim(n, n_steps, prec, seed=2024 + n_steps)
    res, _ = run(ctx, option(K), sim, capi.make_lookback(strike, payoff, lr.CONTINUOUS), False)
    want = capi.lookback_price_f64(BASE["S0"], K, BASE["T"], BASE["r"], BASE["v"], strike, payoff)
    print(f"LOOKBACK prec {prec} strike {strike} payoff {payoff} K {K} n_steps {n_steps}: closed {want:.6f} "
          f"price {res.price:.6f} SE {res.std_err:.6f} ({(res.price - want) / res.std_err:+.2f} SE) live/work "
          f"{res.live_steps / res.work_steps:.4f} kernel {res.kernel_ms:.3f} ms")
    assert res.std_err > 0 and abs(res.price - want) <= 4.0 * res.std_err, (res.price, want, res.std_err)


# ---- 4. one discrete step ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_one_discrete_step_is_the_european_call_struck_at_the_spot(ctx, prec):
    """min(S0, S_T) is the minimum, so the floating call pays (S_T - S0)+"""
    n, rt = 200_000, SUM_RTOL[prec]
    sim = capi.make_sim(n, 1, prec, seed=31)
    res, y = run(ctx, option(K=0.0), sim, capi.make_lookback(lr.FLOATING, lr.CALL, lr.DISCRETE))
    eur = ctx.price_paths(option(BASE["S0"]), sim)
    assert res.n == eur.n == n and res.sum > 0
    assert abs(res.sum - eur.sum) <= rt * eur.sum and abs(res.sumsq - eur.sumsq) <= rt * eur.sumsq
    assert abs(res.price - eur.price) <= rt * eur.price
    _, pay = terminal_prices(ctx, sim, BASE["S0"])
    tol = 1e-11 * (pay + BASE["S0"]) if prec == capi.F64 else 2e-3
    assert (np.abs(y - pay) <= tol).all() and ((y == 0) == (pay == 0)).mean() > 0.9999


# ---- 5. sharding -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cuts", [(0, 4097, 10_001), (0, 1, 6000, 10_001), (0, 5000, 5000, 10_001)])
def test_shards_reproduce_the_whole_job(ctx, prec, cuts):
    """bit for bit: normals AND uniforms of a path depend on its global id alone"""
    n, n_steps = 10_001, 51
    for lb in (capi.make_lookback(lr.FIXED, lr.CALL, lr.CONTINUOUS), capi.make_lookback(lr.FLOATING, lr.CALL, lr.CONTINUOUS)):
        whole, y = run(ctx, option(105.0), capi.make_sim(n, n_steps, prec, seed=3), lb)
        total, totsq, count, live = 0.0, 0.0, 0, 0.0
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            sim = capi.make_sim(n, n_steps, prec, seed=3, path_offset=lo, n_paths_local=hi - lo)
            part, y_part = run(ctx, option(105.0), sim, lb)
            if hi == lo:
                assert all(v == 0 for v in part.as_dict().values())
                continue
            assert np.array_equal(y_part, y[lo:hi])
            total, totsq, count, live = total + part.sum, totsq + part.sumsq, count + part.n, live + part.live_steps
        rt = SUM_RTOL[prec]
        assert count == n and abs(total - whole.sum) <= rt * whole.sum and abs(totsq - whole.sumsq) <= rt * whole.sumsq
        assert live == whole.live_steps


# ---- 6. repeatability and the enqueue form -----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [3000, 3_000_000])   # one wave of workgroups; beyond the 8192-workgroup cap (grid-stride)
def test_same_bits_twice_and_from_the_enqueue_form(ctx, prec, n):
    n_steps = 13
    opt, lb = option(95.0), capi.make_lookback(lr.FIXED, lr.PUT, lr.CONTINUOUS)
    sim = capi.make_sim(n + 9, n_steps, prec, seed=4, path_offset=9, n_paths_local=n)
    a, y_a = run(ctx, opt, sim, lb)
    b, y_b = run(ctx, opt, sim, lb)
    assert np.array_equal(y_a, y_b) and (a.sum, a.sumsq, a.work_steps, a.live_steps) == (b.sum, b.sumsq, b.work_steps,
                                                                                         b.live_steps)
    assert a.grid == min(-(-n // 256), 8192) and a.sum > 0
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.full((n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    ctx.price_lookback_enqueue(opt, sim, lb, stats, s)
    ms = ctx.enqueued_kernel_ms(1)
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    assert rec.tolist() == [a.sum, a.sumsq, 0.0, 0.0, 0.0, float(n)]
    assert np.array_equal(s.cpu().numpy().astype(np.float64), y_a)
    fin = capi.finalize_stats(rec, BASE["r"], BASE["T"])
    assert (fin.price, fin.std_err, fin.n) == (a.price, a.std_err, n)
    assert 0.0 < ms[0] < 1e4
    # an empty shard: zeros, still ordered on the stream
    ctx.price_lookback_enqueue(opt, capi.make_sim(n, n_steps, prec, seed=4, path_offset=5, n_paths_local=0), lb, stats)
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()


# ---- 7. the work counters ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_work_counters(ctx, prec):
    """work_steps = 64 n_steps ceil(n / 64), whatever the product (no early exit); live_steps = 0 without the bridge
    and the same for the two products that share an extremum (the comparison with the restated count is in test 1)"""
    for n, n_steps in ((10_000, 51), (3_000_000, 7)):
        sim = capi.make_sim(n, n_steps, prec, seed=6)
        live = {}
        for (strike, payoff), monitoring in itertools.product(lr.PRODUCTS, (lr.DISCRETE, lr.CONTINUOUS)):
            res, _ = run(ctx, option(), sim, capi.make_lookback(strike, payoff, monitoring), False)
            assert res.work_steps == full_work(n, n_steps), (strike, payoff, monitoring, res.work_steps)
            if monitoring == lr.DISCRETE:
                assert res.live_steps == 0.0
            else:
                assert 0 < res.live_steps < n * n_steps and res.live_steps == int(res.live_steps)
                live[strike, payoff] = res.live_steps
        assert live[lr.FLOATING, lr.PUT] == live[lr.FIXED, lr.CALL]      # both walk the maximum
        assert live[lr.FLOATING, lr.CALL] == live[lr.FIXED, lr.PUT]      # both walk the minimum


# ---- 8. flags and the empty shard --------------------------------------------------------------------------------------------

def test_flags_with_a_live_context(ctx):
    opt, lb = option(), capi.make_lookback()
    ok, _ = run(ctx, opt, capi.make_sim(1000, 12), lb, False)
    same, _ = run(ctx, opt, capi.make_sim(1000, 12, flags=capi.FLAG_LOG_SPACE), lb, False)
    assert (ok.sum, ok.sumsq) == (same.sum, same.sumsq) and ok.sum > 0
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_PRODUCT_FORM, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE,
                  capi.FLAG_LOG_SPACE | capi.FLAG_PRODUCT_FORM):
        with pytest.raises(capi.McamdError) as e:
            ctx.price_lookback(opt, capi.make_sim(1000, 12, flags=flags), lb)
        assert e.value.code == capi.ERR_INVALID and "flags" in str(e.value)
        stats = torch.zeros(6, dtype=torch.float64, device="cuda")
        with pytest.raises(capi.McamdError):
            ctx.price_lookback_enqueue(opt, capi.make_sim(1000, 12, flags=flags), lb, stats)
    bad = capi.make_lookback()
    bad.reserved = 3
    with pytest.raises(capi.McamdError):
        ctx.price_lookback(opt, capi.make_sim(1000, 12), bad)
    with pytest.raises(capi.McamdError):
        ctx.price_lookback(option(K=-1.0), capi.make_sim(1000, 12), capi.make_lookback(strike=lr.FIXED))
    # opt->B and, for a floating strike, opt->K are ignored: the same bits whatever they hold
    other, _ = run(ctx, option(K=-7.0, B=55.0), capi.make_sim(1000, 12), lb, False)
    assert (other.sum, other.sumsq) == (ok.sum, ok.sumsq)
    # an empty shard: all zeros, nothing launched
    res, _ = run(ctx, opt, capi.make_sim(1000, 12, path_offset=10, n_paths_local=0), lb, False)
    assert all(v == 0 for v in res.as_dict().values())
