"""GPU tests of the basket pricer (mcamd_price_basket).  Run with -m gpu on an MI355X.

  1. samples, elementwise through d_samples, against the numpy restatement (tests/basket_restate.py) on the oracle's
     rocRAND-exact normals for (seed, global path id, block), all kinds and every barrier direction on best-of and
     worst-of: every width d = 1..8 at 1, 2, 7 and 50 steps, 4096 paths at global ids 5003.. under seed 77, and every
     width again at 7 steps on the deep inputs, ids 2^33 + 5003.. of a job of 2^40 paths under seed 2^40 + 77;
  2. d = 1 against mcamd_price_barrier;  3. knock-in plus knock-out is the unmonitored sample, bit for bit;  4. the
  closed forms within 4 SE;  5. the ordering of the aggregates, sample by sample;  6. shards and the grid-stride loop;
  7. repeatability, the enqueue form, the empty shard and refusals with a live context.  3, 5, 6 and 7 take one of
  d = 4, 6, 7 each beside d from {2, 3, 5, 8}.

All 32 kernels (d = 1..8, both precisions, with and without monitoring) are compared elementwise.  The group of steps a
kernel unrolls is G = NB / gcd(d, NB) steps of G d / NB Philox blocks (NB = 2 normals a block in fp64, 4 in fp32): in
fp32 d = 6 alone has 2 steps of 3 blocks and d = 7 alone 4 steps of 7.  1, 2, 7 and 50 steps leave n_steps % G = 1, 0,
1, 0 where G = 2 and 1, 2, 3, 2 where G = 4 (odd d in fp32): every remainder but a whole number of groups of 4, which
runs no code that 7 and 50 steps do not.

Tolerance of 1, 2 and 5 (basket_restate.elementwise_tolerance; it comes from the restatement alone, measured on the CPU
by tests/test_basket_cpu.py and recorded in basket_restate.SPREAD and DESIGN section 15): four times the largest
elementwise difference between the float64 and longdouble restatements (fp64 kernels: 4 x 4.1e-13 = 1.6e-12 absolute),
or between the float32 and float64 restatements (fp32 kernels: 4 x 2.3e-4 = 9.2e-4), over the 480 cases of test 1 with d
in {1, 2, 3, 5, 8} on ids 5003.., floored at 1e-11 of the sample (fp64) and 2e-3 absolute (fp32) as
tests/test_gpu_lookback.py floors its own; in fp32 the floor decides.  The 288 cases with d in {4, 6, 7} and the 192
deep cases are measured there too (test_elementwise_spread_and_exclusions_of_the_added_gpu_cases) and stay below those
records, so they take the same tolerance.  A barrier path whose restated min_i |ln A_i - ln B| is below MARGIN = 2e-5 in
either restatement is left out (at most 0.54 % of a case's paths on these inputs; cap 1 %): the hit is a discontinuity
no arithmetic reproduces to the last bit."""
import importlib
import math

import numpy as np
import pytest

import basket_restate as br

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

SUM_RTOL = {capi.F64: 1e-11, capi.F32: 2e-5}
PRECS = (capi.F64, capi.F32)

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


def option(K, B=0.0):
    return capi.make_option(S0=0.0, v=0.0, K=K, r=br.R, T=br.T_, B=B)   # opt->S0 and opt->v are ignored


def make(kind, payoff, barrier, d, w=None):
    S0, v, corr = br.inputs(d)
    return capi.make_basket(S0, v, br.weights(kind, d)[0] if w is None else w, corr, kind, payoff, barrier)


def run(ctx, opt, sim, bk, want_samples=True):
    """(result, samples as float64 numpy or None)"""
    s = None
    if want_samples:
        s = torch.full((max(sim.n_paths_local, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    res = ctx.price_basket(opt, sim, bk, s)
    torch.cuda.synchronize()
    return res, (s[:sim.n_paths_local].cpu().numpy().astype(np.float64) if want_samples else None)


def full_work(n, n_steps):
    return 64 * -(-n // 64) * n_steps


# ---- 1. samples against the restatement ----------------------------------------------------------------------------------

def _case(case, where=br.SHALLOW):
    """the ids of the cases on the shallow inputs are those pytest gave them before there were deep ones"""
    name = "-".join(str(x) for x in case)
    return pytest.param(*case, where, id=(name + "-deep") if where == br.DEEP else name)


SAMPLE_CASES = [_case(c) for c in br.PLAIN_CASES + br.BARRIER_CASES + br.MORE_CASES] + \
               [_case(c, br.DEEP) for c in br.DEEP_CASES]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind,payoff,barrier,d,n_steps,where", SAMPLE_CASES)
def test_samples_against_the_restatement(ctx, prec, kind, payoff, barrier, d, n_steps, where):
    seed, first, n_job = where
    want, own, keep, spread = br.compare(prec, kind, payoff, barrier, d, n_steps, where)
    tol = br.elementwise_tolerance(prec, want)
    excluded = 1.0 - keep.mean()
    assert excluded <= br.CAP, excluded
    K = br.weights(kind, d)[1]
    sim = capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=br.N_LOCAL)
    res, got = run(ctx, option(K, br.LEVEL.get(barrier, 0.0)), sim, make(kind, payoff, barrier, d))
    assert np.isfinite(got).all() and res.n == br.N_LOCAL and res.block == 256 and res.grid == br.N_LOCAL // 256
    err = np.abs(got - want)
    k = int(np.argmax(np.where(keep, err - tol, -np.inf)))
    print(f"prec {prec} kind {kind} payoff {payoff} barrier {barrier} d {d} n_steps {n_steps} first path {first}: "
          f"restatement spread {spread:.3e}, tolerance {tol.min():.3e}..{tol.max():.3e}, worst deviation "
          f"{err[keep].max():.3e}, left out {excluded:.4f}, nonzero {(want != 0).mean():.3f}, live {res.live_steps:.0f} "
          f"restated {own['live'].sum()}")
    assert (err[keep] <= tol[keep]).all(), (k, got[k], want[k], tol[k])
    # the sums are those of the kept paths plus the GPU's own left-out samples
    ref = np.where(keep, np.asarray(own["y"], dtype=np.float64), got)
    rt = SUM_RTOL[prec]
    assert abs(res.sum - ref.sum()) <= rt * abs(ref.sum()) + 1e-300, (res.sum, ref.sum())
    assert abs(res.sumsq - (ref * ref).sum()) <= rt * (ref * ref).sum() + 1e-300
    fin = capi.finalize(res.sum, res.sumsq, res.n, br.R, br.T_)
    assert (res.price, res.std_err, res.ci_lo, res.ci_hi) == (fin.price, fin.std_err, fin.ci_lo, fin.ci_hi)
    assert res.sum_c == res.sum_cc == res.sum_yc == res.cv_beta == res.cv_rho == 0.0
    if barrier == br.NO_BARRIER:
        assert res.live_steps == 0.0 and res.work_steps == full_work(br.N_LOCAL, n_steps)
    else:
        # live lane-steps are the restated ones, but for the paths left out (each can differ by at most every step)
        assert abs(res.live_steps - own["live"].sum()) <= n_steps * int((~keep).sum())
        assert 0 < res.work_steps <= full_work(br.N_LOCAL, n_steps)
        if barrier in (br.DOWN_IN, br.UP_IN):   # a knock-in runs to maturity
            assert res.work_steps == full_work(br.N_LOCAL, n_steps)


# ---- 2. one asset against mcamd_price_barrier ----------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("barrier,kind1,payoff", [(br.DOWN_IN, capi.BARRIER_DOWN_IN, br.PUT), (br.DOWN_OUT, capi.BARRIER_DOWN_OUT, br.PUT),
                                                  (br.UP_OUT, capi.BARRIER_UP_OUT, br.CALL), (br.UP_IN, capi.BARRIER_UP_IN, br.CALL)])
def test_one_asset_is_the_discrete_single_barrier(ctx, prec, barrier, kind1, payoff):
    """d = 1, worst-of, w = 1: the same option, seed and normals as mcamd_price_barrier's discrete monitoring;
    Exponents<T> differs from fma(z, vol, drift) by rounding only, so the samples agree within the elementwise
    tolerance but for the paths within MARGIN of the barrier (taken from the restatement of this call)."""
    S0, v, K, n_steps = 80.0, 0.15, 80.0, 50
    B = 64.0 if barrier in (br.DOWN_IN, br.DOWN_OUT) else 100.0
    z = br.stream(prec)
    own = br.samples(z, n_steps, [S0], [v], [1.0], [[1.0]], K, br.T_, br.R, br.WORST_OF, payoff, barrier, B, br.NP_T[prec])
    keep = own["min_abs_d"] >= br.MARGIN
    assert 1.0 - keep.mean() <= br.CAP
    sim = capi.make_sim(br.N_JOB, n_steps, prec, seed=br.SEED, path_offset=br.OFFSET, n_paths_local=br.N_LOCAL)
    bk = capi.make_basket([S0], [v], [1.0], [[1.0]], capi.BASKET_WORST_OF, payoff, barrier)
    res, got = run(ctx, option(K, B), sim, bk)
    s = torch.full((br.N_LOCAL,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    one = ctx.price_barrier(capi.make_option(S0=S0, K=K, r=br.R, v=v, T=br.T_, B=B), sim,
                            capi.make_barrier(kind1, payoff, capi.MONITOR_DISCRETE), s)
    torch.cuda.synchronize()
    ref = s.cpu().numpy().astype(np.float64)
    # the samples here are prices of an asset at 80, not performances: the fp64 floor is relative anyway, and fp32's
    # absolute 2e-3 is the project's agreement of two fp32 routes to a price of this size
    tol = br.elementwise_tolerance(prec, ref)
    err = np.abs(got - ref)
    print(f"prec {prec} barrier {barrier}: worst deviation {err[keep].max():.3e} tolerance {tol.min():.3e}, left out "
          f"{1 - keep.mean():.4f}, prices {res.price:.6f} {one.price:.6f}")
    assert (err[keep] <= tol[keep]).all() and (ref != 0).any()
    assert abs(res.live_steps - one.live_steps) <= n_steps * int((~keep).sum())


# ---- 3. in plus out ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind,d,n_steps", [(br.WORST_OF, 3, 7), (br.BEST_OF, 5, 50), (br.WORST_OF, 8, 13),
                                            (br.BEST_OF, 6, 7)])
def test_in_plus_out_is_the_unmonitored_sample(ctx, prec, kind, d, n_steps):
    n = 20_000
    sim = capi.make_sim(n, n_steps, prec, seed=12)
    for payoff in (br.CALL, br.PUT):
        plain, y = run(ctx, option(1.0), sim, make(kind, payoff, br.NO_BARRIER, d))
        for out, inn in ((br.DOWN_OUT, br.DOWN_IN), (br.UP_OUT, br.UP_IN)):
            B = br.LEVEL[out]
            a, y_out = run(ctx, option(1.0, B), sim, make(kind, payoff, out, d))
            b, y_in = run(ctx, option(1.0, B), sim, make(kind, payoff, inn, d))
            assert np.array_equal(y_out + y_in, y) and ((y_out == 0) | (y_in == 0)).all()
            assert a.live_steps == b.live_steps and 0 < a.live_steps < n * n_steps
            assert b.work_steps == full_work(n, n_steps) >= a.work_steps
            # a barrier no path reaches leaves the unmonitored samples
            far = 1e-6 if out == br.DOWN_OUT else 1e6
            c, y_far = run(ctx, option(1.0, far), sim, make(kind, payoff, out, d))
            e, y_never = run(ctx, option(1.0, far), sim, make(kind, payoff, inn, d))
            assert np.array_equal(y_far, y) and not y_never.any() and c.live_steps == n * n_steps == e.live_steps
            assert (c.sum, c.sumsq) == (plain.sum, plain.sumsq)


# ---- 4. the closed forms -------------------------------------------------------------------------------------------------

def closed_cases():
    for d in (2, 8):
        yield f"geometric d {d}", br.GEOMETRIC, br.CALL, d, None
    yield "exchange", br.ARITHMETIC, br.CALL, 2, [1.0, -1.0]
    for kind in (br.BEST_OF, br.WORST_OF):
        for payoff in (br.CALL, br.PUT):
            yield f"kind {kind} payoff {payoff}", kind, payoff, 2, None


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n_steps", [1, 4])
@pytest.mark.parametrize("case", list(closed_cases()), ids=lambda c: c[0])
def test_closed_forms(ctx, prec, n_steps, case):
    name, kind, payoff, d, w = case
    S0, v, corr = br.inputs(d)
    bk = make(kind, payoff, br.NO_BARRIER, d, w)
    if w is not None:
        K, want = 0.0, capi.exchange_price_f64(S0[0], S0[1], br.T_, v[0], v[1], corr[0][1])
    elif kind == br.GEOMETRIC:
        K = br.weights(kind, d)[1]
        want = capi.basket_geometric_price_f64(bk, K, br.T_, br.R)
    else:
        K = br.weights(kind, d)[1]
        want = br.rainbow2_by_quadrature(1.0, 1.0, v[0], v[1], corr[0][1], K, br.T_, br.R, kind == br.BEST_OF, payoff == br.PUT)
    res, _ = run(ctx, option(K), capi.make_sim(2_000_000, n_steps, prec, seed=2026 + n_steps), bk, False)
    print(f"BASKET prec {prec} {name} n_steps {n_steps}: closed {want:.6f} price {res.price:.6f} SE {res.std_err:.6f} "
          f"({(res.price - want) / res.std_err:+.2f} SE) kernel {res.kernel_ms:.3f} ms")
    assert res.std_err > 0 and abs(res.price - want) <= 4.0 * res.std_err, (res.price, want, res.std_err)


# ---- 5. the ordering of the aggregates -----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("d,n_steps", [(2, 1), (5, 7), (8, 50), (7, 7)])
def test_worst_arithmetic_best_and_geometric_arithmetic(ctx, prec, d, n_steps):
    """min <= mean <= max of the performances and geometric <= arithmetic mean, exactly so in exact arithmetic: calls
    struck at 0 are the aggregates themselves, compared within the elementwise tolerance"""
    S0 = br.inputs(d)[0]
    sim = capi.make_sim(br.N_LOCAL, n_steps, prec, seed=br.SEED)
    perf = 1.0 / (d * S0)
    _, worst = run(ctx, option(0.0), sim, make(br.WORST_OF, br.CALL, br.NO_BARRIER, d))
    _, best = run(ctx, option(0.0), sim, make(br.BEST_OF, br.CALL, br.NO_BARRIER, d))
    _, mean = run(ctx, option(0.0), sim, make(br.ARITHMETIC, br.CALL, br.NO_BARRIER, d, perf))
    tol = br.elementwise_tolerance(prec, best)
    assert (worst <= mean + tol).all() and (mean <= best + tol).all() and (worst > 0).all()
    _, geo = run(ctx, option(0.0), sim, make(br.GEOMETRIC, br.CALL, br.NO_BARRIER, d))
    _, ari = run(ctx, option(0.0), sim, make(br.ARITHMETIC, br.CALL, br.NO_BARRIER, d))
    assert (geo <= ari + br.elementwise_tolerance(prec, ari)).all() and (geo > 0).all()
    assert d == 1 or ((best > worst).all() and (ari > geo).mean() > 0.9)


# ---- 6. shards and the grid-stride loop ----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cut", [1, 255, 2049])
def test_shards_reproduce_the_whole_job(ctx, prec, cut):
    """bit for bit: a path's normals depend on its global id alone"""
    n, n_steps = 4099, 7
    for kind, barrier, d in ((br.ARITHMETIC, br.NO_BARRIER, 3), (br.WORST_OF, br.DOWN_IN, 5),
                             (br.BEST_OF, br.UP_OUT, 7)):
        K = br.weights(kind, d)[1]
        opt, bk = option(K, br.LEVEL.get(barrier, 0.0)), make(kind, br.PUT, barrier, d)
        whole, y = run(ctx, opt, capi.make_sim(n, n_steps, prec, seed=3), bk)
        parts = [run(ctx, opt, capi.make_sim(n, n_steps, prec, seed=3, path_offset=lo, n_paths_local=hi - lo), bk)
                 for lo, hi in ((0, cut), (cut, n))]
        assert np.array_equal(np.concatenate([p[1] for p in parts]), y)
        for field in ("sum", "sumsq"):
            total = sum(getattr(p[0], field) for p in parts)
            assert abs(total - getattr(whole, field)) <= 1e-12 * getattr(whole, field)
        assert sum(p[0].n for p in parts) == n and sum(p[0].live_steps for p in parts) == whole.live_steps


def test_the_grid_stride_loop(ctx):
    """2 097 152 + 300 paths: one workgroup more than kFoldMaxRecords = 8192 workgroups hold without striding"""
    n, half = 2_097_152 + 300, 1_048_576
    S0, v, corr = br.inputs(2)
    opt, bk = option(100.0), make(br.ARITHMETIC, br.CALL, br.NO_BARRIER, 2)
    whole, y = run(ctx, opt, capi.make_sim(n, 1, capi.F32, seed=5), bk)
    assert whole.grid == 8192 and whole.n == n
    a, y_a = run(ctx, opt, capi.make_sim(n, 1, capi.F32, seed=5, path_offset=0, n_paths_local=half), bk)
    b, y_b = run(ctx, opt, capi.make_sim(n, 1, capi.F32, seed=5, path_offset=half, n_paths_local=n - half), bk)
    assert a.grid == half // 256 and np.array_equal(y[:half], y_a) and np.array_equal(y[half:], y_b)
    assert abs(a.sum + b.sum - whole.sum) <= 1e-12 * whole.sum and whole.work_steps == full_work(n, 1)


# ---- 7. repeatability, the enqueue form, the empty shard, refusals ---------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind,barrier,d", [(br.ARITHMETIC, br.NO_BARRIER, 8), (br.WORST_OF, br.DOWN_OUT, 3),
                                                (br.GEOMETRIC, br.NO_BARRIER, 4)])
def test_same_bits_twice_and_from_the_enqueue_form(ctx, prec, kind, barrier, d):
    n, n_steps = 3000, 13
    K = br.weights(kind, d)[1]
    opt, bk = option(K, br.LEVEL.get(barrier, 0.0)), make(kind, br.PUT, barrier, d)
    sim = capi.make_sim(n + 9, n_steps, prec, seed=4, path_offset=9, n_paths_local=n)
    a, y_a = run(ctx, opt, sim, bk)
    b, y_b = run(ctx, opt, sim, bk)
    assert np.array_equal(y_a, y_b) and (a.sum, a.sumsq, a.work_steps, a.live_steps) == (b.sum, b.sumsq, b.work_steps,
                                                                                         b.live_steps)
    assert a.grid == -(-n // 256) and a.sum > 0
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.full((n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    ctx.price_basket_enqueue(opt, sim, bk, stats, s)
    ms = ctx.enqueued_kernel_ms(1)
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    assert rec.tolist() == [a.sum, a.sumsq, 0.0, 0.0, 0.0, float(n)]
    assert np.array_equal(s.cpu().numpy().astype(np.float64), y_a)
    fin = capi.finalize_stats(rec, br.R, br.T_)
    assert (fin.price, fin.std_err, fin.n) == (a.price, a.std_err, n)
    assert 0.0 < ms[0] < 1e4
    # an empty shard: zeros, still ordered on the stream; and all zeros from the synchronous form, nothing launched
    empty = capi.make_sim(n, n_steps, prec, seed=4, path_offset=5, n_paths_local=0)
    ctx.price_basket_enqueue(opt, empty, bk, stats)
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()
    res, _ = run(ctx, opt, empty, bk, False)
    assert all(v == 0 for v in res.as_dict().values())


def test_refusals_with_a_live_context_leave_it_usable(ctx):
    opt, bk = option(1.0, 0.8), make(br.WORST_OF, br.PUT, br.DOWN_IN, 3)
    ok, _ = run(ctx, opt, capi.make_sim(1000, 12), bk, False)
    same, _ = run(ctx, opt, capi.make_sim(1000, 12, flags=capi.FLAG_LOG_SPACE), bk, False)
    assert (ok.sum, ok.sumsq) == (same.sum, same.sumsq) and ok.sum > 0
    stats = torch.zeros(6, dtype=torch.float64, device="cuda")
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_PRODUCT_FORM, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE):
        with pytest.raises(capi.McamdError) as e:
            ctx.price_basket(opt, capi.make_sim(1000, 12, flags=flags), bk)
        assert e.value.code == capi.ERR_INVALID and "flags" in str(e.value)
        with pytest.raises(capi.McamdError):
            ctx.price_basket_enqueue(opt, capi.make_sim(1000, 12, flags=flags), bk, stats)
    bad = make(br.WORST_OF, br.PUT, br.DOWN_IN, 3)
    bad.corr[1] = bad.corr[8] = 1.0
    bad.corr[2] = bad.corr[16] = 0.6
    for wrong_opt, wrong_bk in ((opt, bad), (option(1.0, 1.5), bk), (option(-1.0, 0.8), bk),
                                (opt, make(br.ARITHMETIC, br.PUT, br.DOWN_IN, 3))):
        with pytest.raises(capi.McamdError) as e:
            ctx.price_basket(wrong_opt, capi.make_sim(1000, 12), wrong_bk)
        assert e.value.code == capi.ERR_INVALID
    again, _ = run(ctx, opt, capi.make_sim(1000, 12), bk, False)
    assert (again.sum, again.sumsq, again.live_steps) == (ok.sum, ok.sumsq, ok.live_steps)
