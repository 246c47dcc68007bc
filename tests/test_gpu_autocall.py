"""GPU tests of the worst-of autocallable pricer (mcamd_price_autocall).  Run with -m gpu on an MI355X.

  1. samples, elementwise through d_samples, against the numpy restatement (tests/autocall_restate.py) on normals drawn
     from the oracle's rocRAND-exact generator for (seed, global path id, block): every d = 1..8, both precisions, a
     knock-in at maturity and at every step, (n_steps, observe_every) in {(1,1), (2,1), (7,1), (7,7), (6,3), (50,10)}
     on 4096 paths at global ids 5003.. under seed 77, and (7,1) on the deep inputs of tests/deep_inputs.py;
  2. a level nobody reaches: 1 less the worst-of knock-in put of mcamd_price_basket, sample for sample;  3. a level
  everybody reaches: every path is paid at first_call_date and the wavefronts leave the loop there;  4. one asset, one
  date against the closed form;  5. the recorded 3-asset note;  6. shards;  7. repeatability, the grid-stride loop and
  the enqueue form;  8. flags, the empty shard and refusals with a live context.

Tolerance of 1 (it comes from the restatement alone, computed and recorded on the CPU by tests/test_autocall_cpu.py).
A path whose worst log-performance comes within MARGIN = 2e-5 of an autocall level at an observation date, or of the
knock-in level at a monitored step, in either restatement is left out of the elementwise comparison: at most
EXCLUDED = 0.32 % of a case's paths, under the cap of 1 %.  A kept path the restatement calls at date q must be paid
pay_q exactly — the double, or (float)pay_q in fp32.  A kept path not called must agree within 4 x the recorded
difference of two restatements (float64 against longdouble: 4.8e-16; float32 against float64: 2.4e-7), floored at 1e-11
of the sample in fp64 and at 2e-5 in fp32 — the project's 2e-3 on prices of size 100, on samples of size 1; the floors
decide.  The counters are exact: with a coupon a sample above 1 is a called path and its value names the date, so the
GPU's own left-out samples say what they add to n_called, sum_t_call and live_steps."""
import importlib
import math

import numpy as np
import pytest

import autocall_restate as ar
import basket_restate as br

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

SUM_RTOL = {capi.F64: 1e-11, capi.F32: 2e-5}
PRECS = (capi.F64, capi.F32)
NB = {capi.F64: 2, capi.F32: 4}

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


def option(r=ar.R, T=ar.T_):
    return capi.make_option(S0=0.0, v=0.0, K=0.0, r=r, T=T)   # opt->S0, v, K and B are ignored


def make(d, **terms):
    v, corr = ar.inputs(d)
    return capi.make_autocall(v, corr, **terms)


def run(ctx, opt, sim, ac, want_samples=True):
    """(result, samples as float64 numpy or None)"""
    s = None
    if want_samples:
        s = torch.full((max(sim.n_paths_local, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    res = ctx.price_autocall(opt, sim, ac, s)
    torch.cuda.synchronize()
    return res, (s[:sim.n_paths_local].cpu().numpy().astype(np.float64) if want_samples else None)


def group(d, prec):
    """the steps that consume whole Philox blocks: a wavefront can leave the loop at their ends only"""
    return NB[prec] // math.gcd(d, NB[prec])


def full_work(n, n_steps):
    return 64 * -(-n // 64) * n_steps


def counters(res):
    return (res.sum, res.sumsq, res.n_called, res.sum_t_call, res.n_knocked_in)


def stored(pay, prec):
    """the payments as d_samples holds them"""
    return pay if prec == capi.F64 else pay.astype(np.float32).astype(np.float64)


# ---- 1. samples against the restatement ----------------------------------------------------------------------------------

def _case(case):
    d, ki, shape, where = case
    return pytest.param(*case, id=f"{d}-{ki}-{shape[0]}-{shape[1]}" + ("-deep" if where == ar.DEEP else ""))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("d,ki,shape,where", [_case(c) for c in ar.CASES])
def test_samples_against_the_restatement(ctx, prec, d, ki, shape, where):
    seed, first, n_job = where
    n, (n_steps, every) = ar.N_LOCAL, shape
    own, other, keep, spread = ar.compare(prec, d, ki, shape, where)
    terms = ar.terms(d, shape, ki)
    _, pay, t = ar.tables(n_steps, every, ar.T_, ar.R, terms["call_level"], terms["coupon"], terms["call_step_down"])
    want = np.asarray(own["y"] if prec == capi.F64 else other["y"], dtype=np.float64)
    tol = ar.elementwise_tolerance(prec, want)
    excluded = 1.0 - keep.mean()
    called = own["date"] > 0
    assert excluded <= ar.CAP, excluded
    assert 0.05 < called.mean() < 0.95, called.mean()
    sim = capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=n)
    res, got = run(ctx, option(), sim, make(d, **terms))
    assert np.isfinite(got).all() and res.n == n and res.block == 256 and res.grid == n // 256
    err = np.abs(got - want)
    free = keep & ~called
    print(f"prec {prec} d {d} ki {ki} shape {shape} first path {first}: restatement spread {spread:.3e}, tolerance "
          f"{tol.min():.3e}..{tol.max():.3e}, worst deviation of a path not called {err[free].max():.3e}, left out "
          f"{excluded:.4f}, called {called.mean():.3f}, not called and knocked in {(own['knocked'] & ~called).mean():.3f}, "
          f"live/work {res.live_steps / res.work_steps:.3f}")
    # a kept path called at date q is paid pay_q exactly
    paid = stored(pay, prec)[np.maximum(own["date"], 1) - 1]
    k = int(np.argmax(keep & called & (got != paid)))
    assert (got == paid)[keep & called].all(), (k, got[k], paid[k], own["date"][k])
    k = int(np.argmax(np.where(free, err - tol, -np.inf)))
    assert (err[free] <= tol[free]).all(), (k, got[k], want[k], tol[k])
    # the sums are those of the kept paths plus the GPU's own left-out samples
    ref = np.where(keep, np.asarray(own["y"], dtype=np.float64), got)
    rt = SUM_RTOL[prec]
    assert abs(res.sum - ref.sum()) <= rt * abs(ref.sum()), (res.sum, ref.sum())
    assert abs(res.sumsq - (ref * ref).sum()) <= rt * (ref * ref).sum()
    fin = capi.finalize(res.sum, res.sumsq, res.n, ar.R, ar.T_)
    assert (res.price, res.std_err, res.ci_lo, res.ci_hi) == (fin.price, fin.std_err, fin.ci_lo, fin.ci_hi)
    # The counters.  pay_q > 1 (coupon > 0, r > 0) and a path not called has y <= 1: a left-out sample above 1 is a
    # called path, and its value is the payment of one date alone.
    out = ~keep
    out_date = np.zeros(n, dtype=np.int64)
    for q, p in enumerate(stored(pay, prec), 1):
        out_date[out & (got == p)] = q
    assert len(set(stored(pay, prec))) == len(pay) and ((got > 1) == (out_date > 0))[out].all()
    date = np.where(keep, own["date"], out_date)
    assert res.n_called == int((date > 0).sum())
    t_sum = t[date[date > 0] - 1].sum()
    assert abs(res.sum_t_call - t_sum) <= 1e-12 * t_sum
    assert res.live_steps == float(np.where(date > 0, date * every, n_steps).sum())
    # a left-out path not called is knocked in if it pays less than 1, and may be if it pays 1
    low = int((keep & ~called & own["knocked"]).sum() + (out & (got < 1)).sum())
    assert low <= res.n_knocked_in <= low + int((out & (got == 1)).sum())
    assert 0 < res.work_steps <= full_work(n, n_steps) and res.work_steps % 64 == 0
    assert res.live_steps <= res.work_steps


# ---- 2. never called -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("d", [1, 3, 8])
def test_never_called_is_one_less_the_worst_of_knock_in_put(ctx, prec, d):
    """The same X, the same minimum (ln(w_j S0_j) = 0 adds nothing), the same hit test and the same exponential: the
    basket forms 1 - A in fp64 where the note takes A, so 1 - y_basket is A but for the rounding of that one
    subtraction, 2^-53 at most for A <= 1.  In fp32 A is a float and so is the note's sample; the basket's 1 - A is
    exact in fp64 and then narrowed, 2^-24 at most of a value below 1."""
    n, n_steps = 20_000, 13
    S0, v, corr = br.inputs(d)
    sim = capi.make_sim(n, n_steps, prec, seed=11)
    res, got = run(ctx, option(), sim, make(d, observe_every=1, call_level=1e6, coupon=0.03, ki_level=0.8,
                                            ki_monitoring=capi.AUTOCALL_KI_EVERY_STEP))
    bk = capi.make_basket(S0, v, 1.0 / S0, corr, capi.BASKET_WORST_OF, capi.PAYOFF_PUT, capi.BASKET_DOWN_IN)
    s = torch.full((n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    put = ctx.price_basket(capi.make_option(S0=0.0, v=0.0, K=1.0, r=ar.R, T=ar.T_, B=0.8), sim, bk, s)
    torch.cuda.synchronize()
    y_put = s.cpu().numpy().astype(np.float64)
    bound = 2.0 ** -53 if prec == capi.F64 else 2.0 ** -24
    err = np.abs(got - (1.0 - y_put))
    print(f"prec {prec} d {d}: worst deviation {err.max():.3e}, bound {bound:.3e}, knocked in {(got < 1).mean():.3f}")
    assert (err <= bound).all() and 0.02 < (got < 1).mean() < 0.98 and (got <= 1).all()
    assert res.n_called == 0 and res.sum_t_call == 0.0
    assert res.work_steps == full_work(n, n_steps) == put.work_steps and res.live_steps == n * n_steps
    assert int((y_put > 0).sum()) <= res.n_knocked_in <= int((y_put > 0).sum()) + int((got == 1).sum())


# ---- 3. always called ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("d,n_steps,every", [(1, 12, 3), (2, 12, 3), (3, 14, 2), (8, 9, 3), (5, 7, 7)])
def test_always_called_pays_at_the_first_call_date(ctx, prec, d, n_steps, every):
    n, M = 3000, n_steps // every
    _, pay, t = ar.tables(n_steps, every, ar.T_, ar.R, 1e-6, 0.04)
    for first in sorted({1, min(2, M), M}):
        sim = capi.make_sim(n, n_steps, prec, seed=5)
        res, got = run(ctx, option(), sim, make(d, observe_every=every, call_level=1e-6, coupon=0.04, ki_level=1e-7,
                                                ki_monitoring=capi.AUTOCALL_KI_EVERY_STEP, first_call_date=first))
        assert (got == stored(pay, prec)[first - 1]).all()
        assert res.n_called == n and res.n_knocked_in == 0
        assert abs(res.sum_t_call - n * t[first - 1]) <= 1e-12 * n * t[first - 1]
        assert abs(res.sum - n * pay[first - 1]) <= SUM_RTOL[capi.F64] * n * pay[first - 1]
        # the wavefronts leave at the first group end at or after the step of the date (or at maturity)
        G, s_q = group(d, prec), first * every
        assert res.work_steps == full_work(n, 1) * min(-(-s_q // G) * G, n_steps), (first, res.work_steps)
        assert res.live_steps == n * s_q


# ---- 4. the closed form ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n_steps", [1, 12])
@pytest.mark.parametrize("ki,B", [(capi.AUTOCALL_KI_NONE, 0.0), (capi.AUTOCALL_KI_AT_MATURITY, 0.8)])
def test_one_asset_one_date_against_the_closed_form(ctx, prec, n_steps, ki, B):
    n, T, r, v, L, c = 4_000_000, 1.0, 0.05, 0.25, 1.02, 0.06
    sim = capi.make_sim(n, n_steps, prec, seed=2025 + n_steps)
    ac = capi.make_autocall([v], [[1.0]], n_steps, L, c, B, ki)
    res, _ = run(ctx, option(r, T), sim, ac, False)
    want = capi.autocall_single_date_price_f64(T, r, v, L, c, B, ki)
    dev = (res.price - want) / res.std_err
    print(f"AUTOCALL prec {prec} n_steps {n_steps} ki {ki}: closed {want:.6f} price {res.price:.6f} SE {res.std_err:.6f} "
          f"({dev:+.2f} SE) called {res.n_called / n:.3f} knocked in {res.n_knocked_in / n:.3f} kernel {res.kernel_ms:.3f} ms")
    assert res.n == n and res.std_err > 0 and abs(res.price - want) <= 4.0 * res.std_err, (res.price, want, res.std_err)
    assert res.work_steps == full_work(n, n_steps) and res.live_steps == n * n_steps   # the one date is maturity
    assert abs(res.sum_t_call - res.n_called * T) <= 1e-12 * n and (ki == capi.AUTOCALL_KI_NONE) == (res.n_knocked_in == 0)


# ---- 5. the recorded note --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_the_recorded_three_asset_note(ctx, prec):
    p = dict(ar.NOTE)
    d, n_steps = p.pop("d"), p.pop("n_steps")
    n = 1_000_000
    res, _ = run(ctx, option(), capi.make_sim(n, n_steps, prec, seed=909), make(d, **p), False)
    rec, rec_se = ar.NOTE_RECORD
    print(f"prec {prec}: price {res.price:.6f} SE {res.std_err:.3e}; CPU record {rec:.6f} SE {rec_se:.3e}; called "
          f"{res.n_called / n:.3f}, mean call time {res.sum_t_call / res.n_called:.3f}, knocked in {res.n_knocked_in / n:.3f}, "
          f"live/work {res.live_steps / res.work_steps:.3f}")
    assert res.std_err > 0 and abs(res.price - rec) <= 4.0 * math.hypot(res.std_err, rec_se), (res.price, rec)
    assert 0 < res.n_called < n and 0 < res.n_knocked_in < n - res.n_called
    assert res.live_steps < res.work_steps <= full_work(n, n_steps)


# ---- 6. sharding -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cuts", [(0, 4097, 10_001), (0, 1, 6000, 10_001), (0, 5000, 5000, 10_001)])
def test_shards_reproduce_the_whole_job(ctx, prec, cuts):
    """bit for bit: a path's normals depend on its global id alone"""
    n, n_steps, rt = 10_001, 51, SUM_RTOL[prec]
    ac = make(3, observe_every=17, call_level=0.98, coupon=0.03, ki_level=0.75, ki_monitoring=capi.AUTOCALL_KI_EVERY_STEP,
              call_step_down=0.01)
    whole, y = run(ctx, option(), capi.make_sim(n, n_steps, prec, seed=3), ac)
    total, counts, live = np.zeros(3), [0, 0, 0], 0.0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sim = capi.make_sim(n, n_steps, prec, seed=3, path_offset=lo, n_paths_local=hi - lo)
        part, y_part = run(ctx, option(), sim, ac)
        if hi == lo:
            assert all(v == 0 for v in part.as_dict().values())
            continue
        assert np.array_equal(y_part, y[lo:hi])
        total = total + np.array([part.sum, part.sumsq, part.sum_t_call])
        counts = [a + b for a, b in zip(counts, (part.n, part.n_called, part.n_knocked_in))]
        live += part.live_steps
    assert counts == [n, whole.n_called, whole.n_knocked_in] and live == whole.live_steps
    assert 0 < whole.n_called < n and whole.n_knocked_in > 0
    for a, b in zip(total, (whole.sum, whole.sumsq, whole.sum_t_call)):
        assert abs(a - b) <= rt * abs(b), (total, counters(whole))


# ---- 7. repeatability and the enqueue form -----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [3000, 3_000_000])   # one wave of workgroups; beyond the 8192-workgroup cap (grid-stride)
def test_same_bits_twice_and_from_the_enqueue_form(ctx, prec, n):
    n_steps = 12
    opt = option()
    ac = make(3, observe_every=3, call_level=1.0, coupon=0.02, ki_level=0.75, ki_monitoring=capi.AUTOCALL_KI_EVERY_STEP)
    sim = capi.make_sim(n + 9, n_steps, prec, seed=4, path_offset=9, n_paths_local=n)
    a, y_a = run(ctx, opt, sim, ac)
    b, y_b = run(ctx, opt, sim, ac)
    assert np.array_equal(y_a, y_b)
    assert counters(a) + (a.work_steps, a.live_steps) == counters(b) + (b.work_steps, b.live_steps)
    assert a.grid == min(-(-n // 256), 8192) and 0 < a.n_called < n and a.n_knocked_in > 0
    assert a.n_called == int((y_a > 1).sum()) and a.live_steps <= a.work_steps <= full_work(n, n_steps)
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.full((n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    ctx.price_autocall_enqueue(opt, sim, ac, stats, s)
    ms = ctx.enqueued_kernel_ms(1)
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    assert rec.tolist() == [float(x) for x in counters(a)] + [float(n)]
    assert np.array_equal(s.cpu().numpy().astype(np.float64), y_a)
    fin = capi.finalize_stats(rec, ar.R, ar.T_)   # control_variate = 0 reads the sums and n alone
    assert (fin.price, fin.std_err, fin.ci_lo, fin.ci_hi, fin.n) == (a.price, a.std_err, a.ci_lo, a.ci_hi, n)
    assert 0.0 < ms[0] < 1e4
    # the synchronous call after an enqueue: the arrival ticket was left zero
    c, _ = run(ctx, opt, sim, ac, False)
    assert counters(c) == counters(a)
    # an empty shard: zeros, still ordered on the stream
    ctx.price_autocall_enqueue(opt, capi.make_sim(n, n_steps, prec, seed=4, path_offset=5, n_paths_local=0), ac, stats)
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()


# ---- 8. flags, the empty shard, refusals with a live context -----------------------------------------------------------------

def test_flags_and_refusals_with_a_live_context(ctx):
    opt = option()
    ac = make(3, observe_every=3, call_level=1.0, coupon=0.02, ki_level=0.75, ki_monitoring=capi.AUTOCALL_KI_AT_MATURITY)
    ok, _ = run(ctx, opt, capi.make_sim(1000, 12), ac, False)
    same, _ = run(ctx, opt, capi.make_sim(1000, 12, flags=capi.FLAG_LOG_SPACE), ac, False)
    assert counters(ok) == counters(same) and ok.sum > 0
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_PRODUCT_FORM, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE,
                  capi.FLAG_LOG_SPACE | capi.FLAG_PRODUCT_FORM):
        with pytest.raises(capi.McamdError) as e:
            ctx.price_autocall(opt, capi.make_sim(1000, 12, flags=flags), ac)
        assert e.value.code == capi.ERR_INVALID and "flags" in str(e.value)
        stats = torch.zeros(6, dtype=torch.float64, device="cuda")
        with pytest.raises(capi.McamdError):
            ctx.price_autocall_enqueue(opt, capi.make_sim(1000, 12, flags=flags), ac, stats)
    bad = make(3, observe_every=3, call_level=1.0, coupon=0.02)
    bad.reserved[1] = 3
    with pytest.raises(capi.McamdError):
        ctx.price_autocall(opt, capi.make_sim(1000, 12), bad)
    with pytest.raises(capi.McamdError):
        ctx.price_autocall(opt, capi.make_sim(1000, 12), make(3, observe_every=5, call_level=1.0, coupon=0.02))
    # opt->S0, v, K and B are ignored: the same bits whatever they hold; and the context is still usable
    other, _ = run(ctx, capi.make_option(S0=float("nan"), v=-1.0, K=float("inf"), B=55.0, r=ar.R, T=ar.T_),
                   capi.make_sim(1000, 12), ac, False)
    assert counters(other) == counters(ok)
    # without a knock-in ki_level is ignored and nobody is knocked in
    free = [run(ctx, opt, capi.make_sim(1000, 12), make(3, observe_every=3, call_level=1.0, coupon=0.02, ki_level=k), False)[0]
            for k in (0.0, float("nan"))]
    assert counters(free[0]) == counters(free[1]) and free[0].n_knocked_in == 0 and free[0].sum >= ok.sum
    # an empty shard: all zeros, nothing launched
    res, _ = run(ctx, opt, capi.make_sim(1000, 12, path_offset=10, n_paths_local=0), ac, False)
    assert all(v == 0 for v in res.as_dict().values())
