"""GPU tests of the Asian pricer (mcamd_price_asian).  Run with -m gpu on an MI355X.

  1. samples, elementwise through d_samples, against the numpy restatement (tests/asian_restate.py) on normals drawn
     from the oracle's rocRAND-exact generator for (seed, global path id, block): 50, 7 and 5 steps on 4096 paths at
     global ids 5003.. under seed 77, and 7 steps on the deep inputs, ids 2^33 + 5003.. of a job of 2^40 paths under
     seed 2^40 + 77.  These step counts leave 2, 3, 1 and 3 of the 4 normals of a path's last Philox block in fp32 and
     0, 1, 1 and 1 of its 2 in fp64;
  2. the arithmetic average against the prices mcamd_simulate_trajectories stores;  3. geometric jobs against the closed
  form within 4 SE at n_steps 1, 12 and 252;  4. one step without the spot is mcamd_price_paths;  5. the control
  variate;  6. shards;  7. repeatability and the enqueue form;  8. flags, ignored fields and the empty shard.

Tolerance of 1 (elementwise_tolerance below; it comes from the restatement alone, computed and recorded on the CPU by
tests/test_asian_cpu.py): four times the largest elementwise difference between the float64 and longdouble restatements
(fp64 kernels), or between the float32 and float64 restatements (fp32 kernels), over all 32 average x strike x payoff x
include_spot x n_steps cases on the test's own inputs — S0 = 100, r = 0.1, v = 0.2, T = 1, K = 100; 50 and 7 steps, 4096
paths at global ids 5003.., seed 77 — floored at 1e-11 of the sample (fp64) and 2e-3 absolute (fp32).  Recorded:
4 x 2.0e-13 = 8.0e-13 absolute for fp64; 4 x 1.3e-4 = 5.2e-4 for fp32, i.e. the 2e-3 floor decides there.  The sample is
continuous in every input, so NO path is left out.  The 64 cases at 5 steps and on the deep inputs take the same
tolerance: their restatements differ by 7.1e-14 (fp64) and 4.8e-5 (fp32) at most, recorded as RECORD["spread_more"] and
measured again by the same CPU test, which also holds them below the record above."""
import importlib
import itertools
import math

import numpy as np
import pytest

import asian_restate as ar

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

NP_T = {capi.F64: np.float64, capi.F32: np.float32}
SUM_RTOL = {capi.F64: 1e-11, capi.F32: 2e-5}
BASE = ar.BASE
PRECS = (capi.F64, capi.F32)
CONTROL = capi.ASIAN_CONTROL_GEOMETRIC


def option(K=ar.K_ATM, **kw):
    return capi.make_option(**dict(BASE, K=K, **kw))


def elementwise_tolerance(prec, want):
    """Absolute tolerance per element: 4 x the recorded restatement difference, floored at 1e-11 of the sample (fp64) /
    2e-3 (fp32).  From the restatement alone."""
    spread = ar.RECORD["spread"][prec]
    if prec == capi.F64:
        return np.maximum(4.0 * spread, 1e-11 * np.abs(want))
    return np.full(want.shape, max(4.0 * spread, 2e-3))


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


def run(ctx, opt, sim, asian, want_samples=True):
    """(result, samples as float64 numpy or None)"""
    s = None
    if want_samples:
        s = torch.full((max(sim.n_paths_local, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    res = ctx.price_asian(opt, sim, asian, s)
    torch.cuda.synchronize()
    return res, (s[:sim.n_paths_local].cpu().numpy().astype(np.float64) if want_samples else None)


def full_work(n, n_steps):
    return 64 * -(-n // 64) * n_steps


def five(res):
    return (res.sum, res.sumsq, res.sum_c, res.sum_cc, res.sum_yc)


def mu_g(n_steps, strike, payoff, spot, K=ar.K_ATM):
    return math.exp(BASE["r"] * BASE["T"]) * capi.asian_geometric_price_f64(
        BASE["S0"], K, BASE["T"], BASE["r"], BASE["v"], n_steps, spot, strike, payoff)


# ---- 1. samples against the restatement ----------------------------------------------------------------------------------

def cases(inputs):
    return [(prec, n_steps, average) + p + (where,) for prec in PRECS for n_steps, where in inputs
            for average in (ar.ARITHMETIC, ar.GEOMETRIC) for p in ar.PRODUCTS]


def _case(case):
    """the ids of the 50- and 7-step cases on the shallow inputs are those pytest gave them before there were deep ones"""
    return pytest.param(*case, id="-".join(str(x) for x in case[:-1]) + ("-deep" if case[-1] == ar.DEEP else ""))


CASES = [_case(c) for c in cases(ar.INPUTS) + cases(ar.MORE_INPUTS)]


@pytest.mark.parametrize("prec,n_steps,average,strike,payoff,spot,where", CASES)
def test_samples_against_the_restatement(ctx, prec, n_steps, average, strike, payoff, spot, where):
    bits = 64 if prec == capi.F64 else 32
    seed, first, n_job = where
    z = ar.oracle_normals(bits, seed, first, ar.N_LOCAL, n_steps)
    own = np.asarray(ar.restate(z, average, strike, payoff, spot, NP_T[prec])["y"], dtype=np.float64)
    want = own if prec == capi.F64 else ar.restate(z, average, strike, payoff, spot, np.float64)["y"]
    tol = elementwise_tolerance(prec, want)
    sim = capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=ar.N_LOCAL)
    res, got = run(ctx, option(), sim, capi.make_asian(average, strike, payoff, spot))
    assert np.isfinite(got).all() and res.n == ar.N_LOCAL and res.block == 256 and res.grid == ar.N_LOCAL // 256
    err = np.abs(got - want)
    k = int(np.argmax(err - tol))
    print(f"prec {prec} n_steps {n_steps} average {average} strike {strike} payoff {payoff} spot {spot} first path "
          f"{first}: tolerance "
          f"{tol.min():.3e}..{tol.max():.3e}, worst deviation {err.max():.3e}, nonzero samples {(want != 0).mean():.3f}")
    assert (err <= tol).all(), (k, got[k], want[k], tol[k])   # every path: nothing is left out
    assert 0.3 < (want != 0).mean()
    rt = SUM_RTOL[prec]
    assert abs(res.sum - own.sum()) <= rt * abs(own.sum()), (res.sum, own.sum())
    assert abs(res.sumsq - (own * own).sum()) <= rt * (own * own).sum()
    fin = capi.finalize(res.sum, res.sumsq, res.n, BASE["r"], BASE["T"])
    assert (res.price, res.std_err, res.ci_lo, res.ci_hi) == (fin.price, fin.std_err, fin.ci_lo, fin.ci_hi)
    assert res.sum_c == res.sum_cc == res.sum_yc == res.cv_beta == res.cv_rho == 0.0
    assert res.work_steps == full_work(ar.N_LOCAL, n_steps) and res.live_steps == 0.0


# ---- 2. the arithmetic average against the stored trajectories ---------------------------------------------------------------

_traj = {}


def stored_prices(ctx, sim):
    """[n_steps, n] prices of mcamd_simulate_trajectories for the same sim, as float64 (shared among the cases)"""
    key = (sim.precision, sim.n_paths_local, sim.n_steps, sim.seed)
    if key not in _traj:
        n, steps = sim.n_paths_local, sim.n_steps
        traj = torch.empty(n * steps, dtype=TORCH_T[sim.precision], device="cuda")
        ctx.simulate_trajectories(option(), sim, traj)
        torch.cuda.synchronize()
        _traj[key] = traj.view(steps, n).cpu().numpy().astype(np.float64)
    return _traj[key]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("strike,payoff,spot", ar.PRODUCTS)
def test_arithmetic_average_against_the_stored_trajectories(ctx, prec, strike, payoff, spot):
    """P_i are the bits the store kernel writes, so the only difference a correct kernel can show is the rounding of
    two fp64 sums of m positive terms, 2 m 2^-53 A, plus in fp32 the narrowing of the sample, 2^-24 |y|."""
    n, n_steps = 50_000, 50
    sim = capi.make_sim(n, n_steps, prec, seed=19)
    P = stored_prices(ctx, sim)
    m = n_steps + spot
    total = np.full(n, BASE["S0"] if spot else 0.0)
    for i in range(n_steps):
        total = total + P[i]
    A = total / m
    want = ar.payoff_of(A, P[-1], ar.K_ATM, strike, payoff)
    _, got = run(ctx, option(), sim, capi.make_asian(ar.ARITHMETIC, strike, payoff, spot))
    bound = 2.0 * m * 2.0 ** -53 * A + (2.0 ** -24 * np.abs(want) if prec == capi.F32 else 0.0)
    err = np.abs(got - want)
    print(f"prec {prec} strike {strike} payoff {payoff} spot {spot}: worst deviation {err.max():.3e}, bound "
          f"{bound.min():.3e}..{bound.max():.3e}, nonzero {(want != 0).mean():.3f}")
    assert (err <= bound).all() and 0.3 < (want != 0).mean()


# ---- 3. the closed form ------------------------------------------------------------------------------------------------------

CLOSED = [(prec, n_steps, spot, strike, payoff, K) for prec in PRECS for n_steps in (1, 12, 252) for spot in (0, 1)
          for strike, payoff, K in [(ar.FIXED, p, K) for p in (ar.CALL, ar.PUT) for K in (90.0, 100.0, 110.0)] +
          [(ar.FLOATING, ar.CALL, 100.0), (ar.FLOATING, ar.PUT, 100.0)]]


@pytest.mark.parametrize("prec,n_steps,spot,strike,payoff,K", CLOSED)
def test_geometric_jobs_against_the_closed_form(ctx, prec, n_steps, spot, strike, payoff, K):
    n = 4_000_000
    sim = capi.make_sim(n, n_steps, prec, seed=2025 + n_steps)
    res, _ = run(ctx, option(K), sim, capi.make_asian(ar.GEOMETRIC, strike, payoff, spot), False)
    want = capi.asian_geometric_price_f64(BASE["S0"], K, BASE["T"], BASE["r"], BASE["v"], n_steps, spot, strike, payoff)
    dev = (res.price - want) / res.std_err if res.std_err > 0 else 0.0
    print(f"ASIAN prec {prec} n_steps {n_steps} spot {spot} strike {strike} payoff {payoff} K {K}: closed {want:.6f} "
          f"price {res.price:.6f} SE {res.std_err:.6f} ({dev:+.2f} SE) kernel {res.kernel_ms:.3f} ms")
    assert res.n == n and res.work_steps == full_work(n, n_steps)
    if strike == ar.FLOATING and n_steps == 1 and not spot:
        assert res.sum == 0.0 and res.sumsq == 0.0 and want == 0.0   # the average IS S_T, bit for bit
        return
    assert res.std_err > 0 and abs(res.price - want) <= 4.0 * res.std_err, (res.price, want, res.std_err)


# ---- 4. one step without the spot --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_one_step_without_the_spot_is_the_european_call(ctx, prec):
    n, rt = 200_000, SUM_RTOL[prec]
    sim = capi.make_sim(n, 1, prec, seed=31)
    res, _ = run(ctx, option(), sim, capi.make_asian(ar.ARITHMETIC, ar.FIXED, ar.CALL, 0), False)
    eur = ctx.price_paths(option(), sim)
    assert res.n == eur.n == n and res.sum > 0
    assert abs(res.sum - eur.sum) <= rt * eur.sum and abs(res.sumsq - eur.sumsq) <= rt * eur.sumsq
    assert abs(res.price - eur.price) <= rt * eur.price


# ---- 5. the control variate --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("strike,payoff,spot", ar.PRODUCTS)
def test_control_variate(ctx, prec, strike, payoff, spot):
    """The recomputation of the five sums from the two plain jobs' samples holds SUM_RTOL of each sum in fp64.  In fp32
    d_samples carries y and g narrowed to float, 2^-24 of each sample, which sum c — a sum of about as many positive as
    negative terms — does not hold relative to ITSELF: there the three sums with c are held to SUM_RTOL of the sum of
    the terms' magnitudes."""
    n, n_steps, rt = ar.CV_PATHS, ar.CV_STEPS, SUM_RTOL[prec]
    sim = capi.make_sim(n, n_steps, prec, seed=909)   # the record's draws are numpy's: other paths altogether
    plain, y = run(ctx, option(), sim, capi.make_asian(ar.ARITHMETIC, strike, payoff, spot))
    _, g = run(ctx, option(), sim, capi.make_asian(ar.GEOMETRIC, strike, payoff, spot))
    res, y_c = run(ctx, option(), sim, capi.make_asian(ar.ARITHMETIC, strike, payoff, spot, CONTROL))
    assert np.array_equal(y_c, y)                       # d_samples receives y, never the adjusted value
    assert (res.sum, res.sumsq) == (plain.sum, plain.sumsq) and res.n == n
    assert res.work_steps == full_work(n, n_steps) and res.live_steps == 0.0
    c = g - mu_g(n_steps, strike, payoff, spot)
    want = (y.sum(), (y * y).sum(), c.sum(), (c * c).sum(), (y * c).sum())
    scale = want if prec == capi.F64 else (want[0], want[1], np.abs(c).sum(), want[3], np.abs(y * c).sum())
    for name, a, b, s in zip(("sum", "sumsq", "sum_c", "sum_cc", "sum_yc"), five(res), want, scale):
        assert abs(a - b) <= rt * abs(s), (name, a, b)
    fin = capi.finalize_cv(five(res), n, BASE["r"], BASE["T"])
    assert (res.price, res.std_err, res.cv_beta, res.cv_rho, res.ci_lo, res.ci_hi) == \
        (fin.price, fin.std_err, fin.cv_beta, fin.cv_rho, fin.ci_lo, fin.ci_hi)
    rho = ar.RECORD["rho_min"]
    rec_price, rec_se = ar.RECORD["controlled"][strike, payoff, spot]
    print(f"prec {prec} strike {strike} payoff {payoff} spot {spot}: plain {plain.price:.6f} SE {plain.std_err:.3e}; "
          f"controlled {res.price:.6f} SE {res.std_err:.3e} (x{plain.std_err / res.std_err:.1f}) beta {res.cv_beta:.4f} "
          f"rho {res.cv_rho:.6f}; CPU record {rec_price:.6f} SE {rec_se:.3e}")
    assert 0 < res.std_err < plain.std_err * 2.0 * math.sqrt(1.0 - rho * rho)
    assert abs(res.price - rec_price) <= 4.0 * math.hypot(res.std_err, rec_se), (res.price, rec_price)


def test_control_on_a_geometric_job_is_refused(ctx):
    with pytest.raises(capi.McamdError) as e:
        ctx.price_asian(option(), capi.make_sim(1000, 12), capi.make_asian(ar.GEOMETRIC, control=CONTROL))
    assert e.value.code == capi.ERR_INVALID and "arithmetic jobs only" in str(e.value)


# ---- 6. sharding -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cuts", [(0, 4097, 10_001), (0, 1, 6000, 10_001), (0, 5000, 5000, 10_001)])
def test_shards_reproduce_the_whole_job(ctx, prec, cuts):
    """bit for bit: a path's normals depend on its global id alone"""
    n, n_steps, rt = 10_001, 51, SUM_RTOL[prec]
    for asian in (capi.make_asian(ar.ARITHMETIC, ar.FIXED, ar.CALL, 1, CONTROL),
                  capi.make_asian(ar.GEOMETRIC, ar.FLOATING, ar.PUT, 0)):
        whole, y = run(ctx, option(105.0), capi.make_sim(n, n_steps, prec, seed=3), asian)
        total, count, work = np.zeros(5), 0, 0.0
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            sim = capi.make_sim(n, n_steps, prec, seed=3, path_offset=lo, n_paths_local=hi - lo)
            part, y_part = run(ctx, option(105.0), sim, asian)
            if hi == lo:
                assert all(v == 0 for v in part.as_dict().values())
                continue
            assert np.array_equal(y_part, y[lo:hi])
            total, count, work = total + np.array(five(part)), count + part.n, work + part.work_steps
        assert count == n and work >= whole.work_steps
        for a, b in zip(total, five(whole)):
            assert abs(a - b) <= rt * abs(b), (total, five(whole))
        assert (whole.sum_cc > 0) == (asian.control == CONTROL)


# ---- 7. repeatability and the enqueue form -----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [3000, 3_000_000])   # one wave of workgroups; beyond the 8192-workgroup cap (grid-stride)
def test_same_bits_twice_and_from_the_enqueue_form(ctx, prec, n):
    n_steps = 13
    opt, asian = option(95.0), capi.make_asian(ar.ARITHMETIC, ar.FIXED, ar.PUT, 1, CONTROL)
    sim = capi.make_sim(n + 9, n_steps, prec, seed=4, path_offset=9, n_paths_local=n)
    a, y_a = run(ctx, opt, sim, asian)
    b, y_b = run(ctx, opt, sim, asian)
    assert np.array_equal(y_a, y_b) and five(a) + (a.work_steps,) == five(b) + (b.work_steps,)
    assert a.grid == min(-(-n // 256), 8192) and a.sum > 0 and a.sum_cc > 0 and a.work_steps == full_work(n, n_steps)
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.full((n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    ctx.price_asian_enqueue(opt, sim, asian, stats, s)
    ms = ctx.enqueued_kernel_ms(1)
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    assert rec.tolist() == list(five(a)) + [float(n)]
    assert np.array_equal(s.cpu().numpy().astype(np.float64), y_a)
    fin = capi.finalize_stats(rec, BASE["r"], BASE["T"], control_variate=True)
    assert (fin.price, fin.std_err, fin.cv_beta, fin.cv_rho, fin.n) == (a.price, a.std_err, a.cv_beta, a.cv_rho, n)
    assert 0.0 < ms[0] < 1e4
    # without the control the record is {sum, sumsq, 0, 0, 0, n}
    plain = capi.make_asian(ar.ARITHMETIC, ar.FIXED, ar.PUT, 1)
    ctx.price_asian_enqueue(opt, sim, plain, stats)
    torch.cuda.synchronize()
    assert stats.cpu().numpy().tolist() == [a.sum, a.sumsq, 0.0, 0.0, 0.0, float(n)]
    # an empty shard: zeros, still ordered on the stream
    ctx.price_asian_enqueue(opt, capi.make_sim(n, n_steps, prec, seed=4, path_offset=5, n_paths_local=0), asian, stats)
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()


# ---- 8. flags, ignored fields and the empty shard ----------------------------------------------------------------------------

def test_flags_with_a_live_context(ctx):
    opt, asian = option(), capi.make_asian(control=CONTROL)
    ok, _ = run(ctx, opt, capi.make_sim(1000, 12), asian, False)
    same, _ = run(ctx, opt, capi.make_sim(1000, 12, flags=capi.FLAG_LOG_SPACE), asian, False)
    assert five(ok) == five(same) and ok.sum > 0
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_PRODUCT_FORM, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE,
                  capi.FLAG_LOG_SPACE | capi.FLAG_PRODUCT_FORM):
        with pytest.raises(capi.McamdError) as e:
            ctx.price_asian(opt, capi.make_sim(1000, 12, flags=flags), asian)
        assert e.value.code == capi.ERR_INVALID and "flags" in str(e.value)
        stats = torch.zeros(6, dtype=torch.float64, device="cuda")
        with pytest.raises(capi.McamdError):
            ctx.price_asian_enqueue(opt, capi.make_sim(1000, 12, flags=flags), asian, stats)
    bad = capi.make_asian()
    bad.reserved = 3
    with pytest.raises(capi.McamdError):
        ctx.price_asian(opt, capi.make_sim(1000, 12), bad)
    with pytest.raises(capi.McamdError):
        ctx.price_asian(option(K=-1.0), capi.make_sim(1000, 12), capi.make_asian())
    # opt->B and, for a floating strike, opt->K are ignored: the same bits whatever they hold
    other, _ = run(ctx, option(B=55.0), capi.make_sim(1000, 12), asian, False)
    assert five(other) == five(ok)
    for average, control in ((ar.ARITHMETIC, CONTROL), (ar.ARITHMETIC, 0), (ar.GEOMETRIC, 0)):
        flo = capi.make_asian(average, ar.FLOATING, ar.PUT, 1, control)
        one, _ = run(ctx, opt, capi.make_sim(1000, 12), flo, False)
        two, _ = run(ctx, option(K=-7.0, B=float("nan")), capi.make_sim(1000, 12), flo, False)
        assert five(one) == five(two) and one.sum > 0
    # an empty shard: all zeros, nothing launched
    res, _ = run(ctx, opt, capi.make_sim(1000, 12, path_offset=10, n_paths_local=0), asian, False)
    assert all(v == 0 for v in res.as_dict().values())
