"""GPU tests of the worst-of autocallable under per-asset local-volatility surfaces (mcamd_price_autocall_localvol).
Run with -m gpu on an MI355X.

  1. samples, elementwise through d_samples, against the numpy restatement (tests/autocall_localvol_restate.py) on normals
     drawn from the oracle's rocRAND-exact generator: every d = 1..8, both precisions, a knock-in at maturity and at every
     step, the six (n_steps, observe_every) shapes of the autocall tests on 4096 paths at global ids 5003.. under seed
     77, and (7, 1) on the deep inputs of tests/deep_inputs.py — skewed surfaces on four different grids and dividends;
  2. d = 1 and a level nobody reaches: 1 less mcamd_price_localvol's put, sample for sample;  3. flat surfaces and q = 0
  against mcamd_price_autocall;  4. a level everybody reaches;  5. one asset, one date, a time-only surface against the
  closed form;  6. the recorded 3-asset note;  7. plumbing: the node budget, a shared surface, shards, repeatability, the
  enqueue form, a foreign surface, the empty shard;  8. five mistakes restated in numpy, each with the test that refuses
  it.

Tolerance of 1 (it comes from the restatement alone, computed and recorded on the CPU by
tests/test_autocall_localvol_cpu.py).  A path whose worst log-performance comes within MARGIN = 2e-5 of an autocall level
at an observation date, or of the knock-in level at a monitored step, in either restatement is left out of the
elementwise comparison: at most EXCLUDED = 0.42 % of a case's paths, under the cap of 1 %.  A kept path the restatement
calls at date q must be paid pay_q exactly — the double, or (float)pay_q in fp32.  A kept path not called must agree
within 4 x the recorded difference of two restatements (float64 against longdouble: 3.8e-16; float32 against float64:
2.2e-7), floored at 1e-11 of the sample in fp64 and at 2e-5 in fp32; the floors decide.  The counters are exact: with a
coupon a sample above 1 is a called path and its value names the date, so the GPU's own left-out samples say what they
add to n_called, sum_t_call and live_steps."""
import importlib
import math

import numpy as np
import pytest

import autocall_localvol_restate as alr
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


@pytest.fixture(scope="module")
def surf(ctx):
    """surf(j, kind): asset j's surface of the shared inputs on the module's context, created once"""
    made = {}

    def get(j, kind=alr.skewed):
        if (j, kind) not in made:
            made[(j, kind)] = ctx.localvol_surface(alr.grid(j), kind(j))
        return made[(j, kind)]

    yield get
    torch.cuda.synchronize()
    for s in made.values():
        s.close()


def option(r=alr.R, T=alr.T_):
    return capi.make_option(S0=0.0, v=0.0, K=0.0, r=r, T=T)   # opt->S0, v, K and B are ignored


def make(d, q=alr.Q, **terms):
    return capi.make_autocall_localvol(q[:d], alr.corr(d), **terms)


def run(ctx, opt, sim, ac, surfaces, want_samples=True):
    """(result, samples as float64 numpy or None)"""
    s = None
    if want_samples:
        s = torch.full((max(sim.n_paths_local, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    res = ctx.price_autocall_localvol(opt, sim, ac, surfaces, s)
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
    return pytest.param(*case, id=f"{d}-{ki}-{shape[0]}-{shape[1]}" + ("-deep" if where == alr.DEEP else ""))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("d,ki,shape,where", [_case(c) for c in alr.CASES])
def test_samples_against_the_restatement(ctx, surf, prec, d, ki, shape, where):
    seed, first, n_job = where
    n, (n_steps, every) = alr.N_LOCAL, shape
    own, other, keep, spread = alr.compare(prec, d, ki, shape, where)
    terms = alr.terms(d, shape, ki)
    _, pay, t = ar.tables(n_steps, every, alr.T_, alr.R, terms["call_level"], terms["coupon"], terms["call_step_down"])
    want = np.asarray(own["y"] if prec == capi.F64 else other["y"], dtype=np.float64)
    tol = alr.elementwise_tolerance(prec, want)
    excluded = 1.0 - keep.mean()
    called = own["date"] > 0
    assert excluded <= alr.CAP, excluded
    assert 0.05 < called.mean() < 0.95, called.mean()
    sim = capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=n)
    res, got = run(ctx, option(), sim, make(d, **terms), [surf(j) for j in range(d)])
    assert np.isfinite(got).all() and res.n == n and res.block == 256 and res.grid == n // 256
    err = np.abs(got - want)
    free = keep & ~called
    print(f"ALV prec {prec} d {d} ki {ki} shape {shape} first path {first}: restatement spread {spread:.3e}, tolerance "
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
    fin = capi.finalize(res.sum, res.sumsq, res.n, alr.R, alr.T_)
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


# ---- 2. one asset, never called: the local-volatility put -------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("j,n_steps", [(0, 5), (0, 50), (3, 5), (3, 50)])
def test_one_asset_never_called_is_one_less_the_local_volatility_put(ctx, surf, prec, j, n_steps):
    """d = 1 walks mcamd_price_localvol's path bit for bit (w_0 = z_0 exactly), and with ki_level = 1 at maturity the
    note's sample is min(A, 1) where the put's is max(1 - S_T, 0) with S0 = K = 1 and S_T = A from the same exponential:
    1 - y_lv is A but for the rounding of that one subtraction, 2^-53 at most for A <= 1 (2^-24 in fp32, where the put
    forms 1 - S_T in float)."""
    n, q = 20_000, 0.03
    sim = capi.make_sim(n, n_steps, prec, seed=11, path_offset=7)
    ac = capi.make_autocall_localvol([q], [[1.0]], n_steps, 1e6, 0.03, 1.0, capi.AUTOCALL_KI_AT_MATURITY)
    res, got = run(ctx, option(), sim, ac, [surf(j)])
    s = torch.full((n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    put = ctx.price_localvol(capi.make_option(S0=1.0, v=0.0, K=1.0, r=alr.R, T=alr.T_), sim,
                             capi.make_localvol(capi.PAYOFF_PUT, q=q), surf(j), s)
    torch.cuda.synchronize()
    y_put = s.cpu().numpy().astype(np.float64)
    bound = 2.0 ** -53 if prec == capi.F64 else 2.0 ** -24
    err = np.abs(got - (1.0 - y_put))
    print(f"prec {prec} grid {alr.grid(j)} n_steps {n_steps}: worst deviation {err.max():.3e}, bound {bound:.3e}, "
          f"knocked in {(got < 1).mean():.3f}")
    assert (err <= bound).all() and 0.2 < (got < 1).mean() < 0.8 and (got <= 1).all()
    assert res.n_called == 0 and res.sum_t_call == 0.0
    assert res.work_steps == full_work(n, n_steps) == put.work_steps and res.live_steps == n * n_steps
    assert int((y_put > 0).sum()) <= res.n_knocked_in <= int((y_put > 0).sum()) + int((got == 1).sum())


# ---- 3. flat surfaces, no dividends: the constant-volatility note ----------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [(7, 1), (50, 10)])
@pytest.mark.parametrize("d", [1, 3, 6, 8])
def test_flat_surfaces_give_the_constant_volatility_note(ctx, surf, prec, d, shape):
    """against mcamd_price_autocall at v_j = sigma_j on the shallow inputs: on the paths both restatements keep, a called
    sample is the same payment bit for bit and a sample not called agrees within the tolerance"""
    seed, first, n_job = alr.SHALLOW
    n, (n_steps, every), ki = alr.N_LOCAL, shape, alr.KI_EVERY_STEP
    terms = alr.terms(d, shape, ki)
    own, _, keep_a, _ = ar.compare(prec, d, ki, shape)
    grids, sig = alr.surfaces(d, alr.flat)
    mine = alr.samples(alr.stream_of(prec, alr.SHALLOW), n_steps, grids, sig, [0.0] * d, alr.corr(d), alr.T_, alr.R,
                       dtype=alr.NP_T[prec], **terms)
    keep = keep_a & (mine["min_abs_d"] >= alr.MARGIN)
    sim = capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=n)
    res, got = run(ctx, option(), sim, make(d, q=[0.0] * 8, **terms), [surf(j, alr.flat) for j in range(d)])
    s = torch.full((n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    v, corr = ar.inputs(d)
    base = ctx.price_autocall(option(), sim, capi.make_autocall(v, corr, **terms), s)
    torch.cuda.synchronize()
    y_gbm = s.cpu().numpy().astype(np.float64)
    called = own["date"] > 0
    err = np.abs(got - y_gbm)
    tol = alr.elementwise_tolerance(prec, y_gbm)
    free = keep & ~called
    print(f"prec {prec} d {d} shape {shape}: kept {keep.mean():.4f}, called {called.mean():.3f}, worst deviation of a path "
          f"not called {err[free].max():.3e}, tolerance {tol.min():.3e}")
    assert keep.mean() >= 1.0 - 2.0 * alr.CAP and 0.05 < called.mean() < 0.95
    assert (got == y_gbm)[keep & called].all() and (got > 1)[keep & called].all()
    assert (err[free] <= tol[free]).all()
    assert abs(res.n_called - base.n_called) <= int((~keep).sum())


# ---- 4. always called ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("d,n_steps,every", [(1, 12, 3), (2, 12, 3), (3, 14, 2), (8, 9, 3), (5, 7, 7)])
def test_always_called_pays_at_the_first_call_date(ctx, surf, prec, d, n_steps, every):
    n, M = 3000, n_steps // every
    _, pay, t = ar.tables(n_steps, every, alr.T_, alr.R, 1e-6, 0.04)
    for first in sorted({1, min(2, M), M}):
        sim = capi.make_sim(n, n_steps, prec, seed=5)
        ac = make(d, observe_every=every, call_level=1e-6, coupon=0.04, ki_level=1e-7,
                  ki_monitoring=capi.AUTOCALL_KI_EVERY_STEP, first_call_date=first)
        res, got = run(ctx, option(), sim, ac, [surf(j) for j in range(d)])
        assert (got == stored(pay, prec)[first - 1]).all()
        assert res.n_called == n and res.n_knocked_in == 0
        assert abs(res.sum_t_call - n * t[first - 1]) <= 1e-12 * n * t[first - 1]
        assert abs(res.sum - n * pay[first - 1]) <= SUM_RTOL[capi.F64] * n * pay[first - 1]
        # the wavefronts leave at the first group end at or after the step of the date (or at maturity)
        G, s_q = group(d, prec), first * every
        assert res.work_steps == full_work(n, 1) * min(-(-s_q // G) * G, n_steps), (first, res.work_steps)
        assert res.live_steps == n * s_q


# ---- 5. the closed form ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n_steps", [1, 4, 12])
@pytest.mark.parametrize("ki,B", [(capi.AUTOCALL_KI_NONE, 0.0), (capi.AUTOCALL_KI_AT_MATURITY, 0.8)])
def test_one_asset_one_date_time_only_surface_against_the_closed_form(ctx, prec, n_steps, ki, B):
    """a surface that varies in time only leaves S_T / S_0 lognormal with the rms volatility of the rows the steps use"""
    n, T, r, L, c = 2 ** 19, 1.0, 0.05, 1.02, 0.06
    v = alr.rms_volatility(n_steps)
    sim = capi.make_sim(n, n_steps, prec, seed=2026 + n_steps)
    ac = capi.make_autocall_localvol([0.0], [[1.0]], n_steps, L, c, B, ki)
    with ctx.localvol_surface(alr.TIME_ONLY_GRID, alr.TIME_ONLY_SIGMA) as surface:
        res, _ = run(ctx, option(r, T), sim, ac, [surface], False)
    want = capi.autocall_single_date_price_f64(T, r, v, L, c, B, ki)
    dev = (res.price - want) / res.std_err
    print(f"ALV closed form prec {prec} n_steps {n_steps} ki {ki}: rms vol {v:.5f} closed {want:.6f} price {res.price:.6f} "
          f"SE {res.std_err:.6f} ({dev:+.2f} SE) called {res.n_called / n:.3f} knocked in {res.n_knocked_in / n:.3f}")
    assert res.n == n and res.std_err > 0 and abs(res.price - want) <= 4.0 * res.std_err, (res.price, want, res.std_err)
    assert res.work_steps == full_work(n, n_steps) and res.live_steps == n * n_steps   # the one date is maturity
    assert abs(res.sum_t_call - res.n_called * T) <= 1e-12 * n and (ki == capi.AUTOCALL_KI_NONE) == (res.n_knocked_in == 0)


# ---- 6. the recorded note --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_the_recorded_three_asset_note(ctx, surf, prec):
    p = dict(alr.NOTE)
    d, n_steps = p.pop("d"), p.pop("n_steps")
    n = 1_000_000
    res, _ = run(ctx, option(), capi.make_sim(n, n_steps, prec, seed=909), make(d, **p), [surf(j) for j in range(d)], False)
    rec, rec_se = alr.NOTE_RECORD
    print(f"ALV note prec {prec}: price {res.price:.6f} SE {res.std_err:.3e}; CPU record {rec:.6f} SE {rec_se:.3e}; called "
          f"{res.n_called / n:.3f}, mean call time {res.sum_t_call / res.n_called:.3f}, knocked in {res.n_knocked_in / n:.3f}, "
          f"live/work {res.live_steps / res.work_steps:.3f}")
    assert res.std_err > 0 and abs(res.price - rec) <= 4.0 * math.hypot(res.std_err, rec_se), (res.price, rec)
    assert 0 < res.n_called < n and 0 < res.n_knocked_in < n - res.n_called
    assert res.live_steps < res.work_steps <= full_work(n, n_steps)


# ---- 7. plumbing -------------------------------------------------------------------------------------------------------------

def _big_sigma():
    x = np.linspace(-1.5, 1.5, 64)
    return (0.18 + 0.01 * np.arange(16))[:, None] * (1.0 + 0.5 * np.exp(-x))[None, :] / 1.5


def test_the_node_budget_is_shared_by_the_assets(ctx):
    """two assets of 16 x 64 nodes fill the 2048 nodes exactly and run; a third surface of 1 x 2 nodes is refused"""
    opt, terms = option(), dict(observe_every=3, call_level=1.0, coupon=0.02, ki_level=0.7,
                                ki_monitoring=capi.AUTOCALL_KI_EVERY_STEP)
    with ctx.localvol_surface((16, 64, -1.5, 1.5), _big_sigma()) as a, \
            ctx.localvol_surface((16, 64, -1.5, 1.5), 1.1 * _big_sigma()) as b, \
            ctx.localvol_surface((1, 2, -0.5, 0.5), [[0.2, 0.2]]) as c:
        for prec in PRECS:
            sim = capi.make_sim(5000, 12, prec, seed=8)
            res, y = run(ctx, opt, sim, make(2, **terms), [a, b])
            assert np.isfinite(y).all() and 0 < res.n_called < 5000 and res.n_knocked_in > 0
            again, y2 = run(ctx, opt, sim, make(2, **terms), [a, b])
            assert np.array_equal(y, y2) and counters(res) == counters(again)
            for form in ("sync", "enqueue"):
                with pytest.raises(capi.McamdError) as e:
                    if form == "sync":
                        ctx.price_autocall_localvol(opt, sim, make(3, **terms), [a, b, c])
                    else:
                        ctx.price_autocall_localvol_enqueue(opt, sim, make(3, **terms), [a, b, c],
                                                            torch.zeros(6, dtype=torch.float64, device="cuda"))
                assert e.value.code == capi.ERR_INVALID and "2050 nodes" in str(e.value)
            # and the context is still usable
            assert counters(run(ctx, opt, sim, make(2, **terms), [a, b], False)[0]) == counters(res)
        torch.cuda.synchronize()


@pytest.mark.parametrize("prec", PRECS)
def test_one_surface_shared_by_three_assets(ctx, surf, prec):
    """the same object three times, or three equal surfaces: the same bits"""
    terms = dict(observe_every=3, call_level=0.97, coupon=0.02, ki_level=0.7, ki_monitoring=capi.AUTOCALL_KI_EVERY_STEP)
    sim = capi.make_sim(6000, 12, prec, seed=21)
    shared, y = run(ctx, option(), sim, make(3, **terms), [surf(0)] * 3)
    with ctx.localvol_surface(alr.grid(0), alr.skewed(0)) as b, ctx.localvol_surface(alr.grid(0), alr.skewed(0)) as c:
        apart, y2 = run(ctx, option(), sim, make(3, **terms), [surf(0), b, c])
    assert np.array_equal(y, y2) and counters(shared) == counters(apart)
    assert 0 < shared.n_called < 6000 and shared.n_knocked_in > 0


@pytest.mark.parametrize("prec", PRECS)
def test_ten_shards_add_up_to_the_whole_job(ctx, surf, prec):
    """bit for bit: a path's normals depend on its global id alone"""
    n, n_steps, rt = 10_001, 51, SUM_RTOL[prec]
    ac = make(3, observe_every=17, call_level=0.98, coupon=0.03, ki_level=0.75, ki_monitoring=capi.AUTOCALL_KI_EVERY_STEP,
              call_step_down=0.01)
    surfaces = [surf(j) for j in range(3)]
    whole, y = run(ctx, option(), capi.make_sim(n, n_steps, prec, seed=3), ac, surfaces)
    cuts = (0, 1, 257, 4097, 4097, 5000, 6000, 7001, 8192, 9999, n)
    total, counts, live = np.zeros(3), [0, 0, 0], 0.0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sim = capi.make_sim(n, n_steps, prec, seed=3, path_offset=lo, n_paths_local=hi - lo)
        part, y_part = run(ctx, option(), sim, ac, surfaces)
        if hi == lo:   # an empty shard: all zeros, nothing launched
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


@pytest.mark.parametrize("prec", PRECS)
def test_same_bits_twice_and_from_the_enqueue_form(ctx, surf, prec):
    n, n_steps = 300_000, 12
    opt = option()
    ac = make(3, observe_every=3, call_level=1.0, coupon=0.02, ki_level=0.75, ki_monitoring=capi.AUTOCALL_KI_EVERY_STEP)
    sets = ([surf(j) for j in range(3)], [surf(3), surf(0), surf(1)])
    sim = capi.make_sim(n + 9, n_steps, prec, seed=4, path_offset=9, n_paths_local=n)
    sync = []
    for surfaces in sets:
        a, y_a = run(ctx, opt, sim, ac, surfaces)
        b, y_b = run(ctx, opt, sim, ac, surfaces)
        assert np.array_equal(y_a, y_b)
        assert counters(a) + (a.work_steps, a.live_steps) == counters(b) + (b.work_steps, b.live_steps)
        assert a.grid == -(-n // 256) and 0 < a.n_called < n and a.n_knocked_in > 0
        assert a.n_called == int((y_a > 1).sum()) and a.live_steps <= a.work_steps <= full_work(n, n_steps)
        sync.append((a, y_a))
    assert counters(sync[0][0]) != counters(sync[1][0])
    # eight calls enqueued back to back, alternating between the two surface sets
    stats = torch.full((8, 6), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.full((8, n), float("nan"), dtype=TORCH_T[prec], device="cuda")
    for k in range(8):
        ctx.price_autocall_localvol_enqueue(opt, sim, ac, sets[k % 2], stats[k], s[k])
    ms = ctx.enqueued_kernel_ms(8)
    torch.cuda.synchronize()
    rec, ys = stats.cpu().numpy(), s.cpu().numpy().astype(np.float64)
    for k in range(8):
        a, y_a = sync[k % 2]
        assert rec[k].tolist() == [float(x) for x in counters(a)] + [float(n)]
        assert np.array_equal(ys[k], y_a)
        assert 0.0 < ms[k] < 1e4
    fin = capi.finalize_stats(rec[0], alr.R, alr.T_)   # control_variate = 0 reads the sums and n alone
    a = sync[0][0]
    assert (fin.price, fin.std_err, fin.ci_lo, fin.ci_hi, fin.n) == (a.price, a.std_err, a.ci_lo, a.ci_hi, n)
    # the synchronous call after the enqueues: the arrival ticket was left zero
    c, _ = run(ctx, opt, sim, ac, sets[0], False)
    assert counters(c) == counters(a)
    # an empty shard: zeros, still ordered on the stream
    one = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    ctx.price_autocall_localvol_enqueue(opt, capi.make_sim(n, n_steps, prec, seed=4, path_offset=5, n_paths_local=0), ac,
                                        sets[0], one)
    torch.cuda.synchronize()
    assert not one.cpu().numpy().any()
    res, _ = run(ctx, opt, capi.make_sim(n, n_steps, prec, path_offset=10, n_paths_local=0), ac, sets[0], False)
    assert all(v == 0 for v in res.as_dict().values())


def test_a_foreign_surface_and_the_other_refusals_with_a_live_context(ctx, surf):
    opt = option()
    ac = make(2, observe_every=3, call_level=1.0, coupon=0.02, ki_level=0.75, ki_monitoring=capi.AUTOCALL_KI_AT_MATURITY)
    sim = capi.make_sim(1000, 12)
    ok, _ = run(ctx, opt, sim, ac, [surf(0), surf(1)], False)
    other = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        with other.localvol_surface(alr.grid(1), alr.skewed(1)) as foreign:
            for surfaces in ([surf(0), foreign], [foreign, surf(1)]):
                with pytest.raises(capi.McamdError) as e:
                    ctx.price_autocall_localvol(opt, sim, ac, surfaces)
                assert e.value.code == capi.ERR_INVALID and "another context" in str(e.value)
            with pytest.raises(capi.McamdError):
                ctx.price_autocall_localvol_enqueue(opt, sim, ac, [surf(0), foreign],
                                                    torch.zeros(6, dtype=torch.float64, device="cuda"))
            # a request that is wrong on its own is refused for that, whatever the surfaces are
            with pytest.raises(capi.McamdError) as e:
                ctx.price_autocall_localvol(opt, capi.make_sim(1000, 12, flags=capi.FLAG_ANTITHETIC), ac, [surf(0), foreign])
            assert "flags" in str(e.value)
    finally:
        other.close()
    for surfaces, words in ((None, "surfaces must be non-NULL"), ([surf(0), None], "surfaces[1] is NULL")):
        with pytest.raises(capi.McamdError) as e:
            ctx.price_autocall_localvol(opt, sim, ac, surfaces)
        assert e.value.code == capi.ERR_INVALID and words in str(e.value)
    # fp64: the exponent-range bound at the surface's largest entry
    with ctx.localvol_surface((1, 2, -0.5, 0.5), [[0.2, 300.0]]) as wild:
        with pytest.raises(capi.McamdError) as e:
            ctx.price_autocall_localvol(opt, sim, ac, [surf(0), wild])
        assert "exponent range" in str(e.value)
    # opt->S0, v, K and B are ignored: the same bits whatever they hold; and the context is still usable
    same, _ = run(ctx, capi.make_option(S0=float("nan"), v=-1.0, K=float("inf"), B=55.0, r=alr.R, T=alr.T_), sim, ac,
                  [surf(0), surf(1)], False)
    assert counters(same) == counters(ok) and ok.sum > 0
    flagged, _ = run(ctx, opt, capi.make_sim(1000, 12, flags=capi.FLAG_LOG_SPACE), ac, [surf(0), surf(1)], False)
    assert counters(flagged) == counters(ok)


# ---- 8. mistakes, restated in numpy only, and the test that refuses each ---------------------------------------------------

def _refused(prec, d, ki, shape, mistake, where=alr.SHALLOW, z=None):
    """the paths on which test 1 would fail had the kernel made the mistake: kept paths whose call date differs (their
    payment is then another one) or that are not called and differ by more than the tolerance"""
    own, other, keep, _ = alr.compare(prec, d, ki, shape, where)
    grids, sig = alr.surfaces(d)
    wrong = alr.samples(alr.stream_of(prec, where) if z is None else z, shape[0], grids, sig, alr.Q, alr.corr(d), alr.T_,
                        alr.R, dtype=alr.NP_T[prec], mistake=mistake, **alr.terms(d, shape, ki))
    want = np.asarray(own["y"] if prec == capi.F64 else other["y"], dtype=np.float64)
    err = np.abs(np.asarray(wrong["y"], dtype=np.float64) - want)
    bad = keep & ((wrong["date"] != own["date"]) | ((own["date"] == 0) & (err > alr.elementwise_tolerance(prec, want))))
    return int(bad.sum())


@pytest.mark.parametrize("prec", PRECS)
def test_mistakes_test_1_refuses(prec):
    ki = alr.KI_EVERY_STEP
    for d in (2, 3, 8):   # asset j reading asset 0's table base
        assert _refused(prec, d, ki, (7, 1), alr.TABLE_BASE_OF_ASSET_0) >= 10, d
    # the row carry of asset 0 (4 rows) serving every asset: asset 3 has the 7 x 9 grid
    for shape in ((7, 1), (50, 10)):
        assert _refused(prec, 4, ki, shape, alr.SHARED_ROW_CARRY) >= 10, shape
    assert _refused(prec, 3, ki, (7, 1), alr.SHARED_ROW_CARRY) >= 10        # and asset 2 has 3 rows
    for d in (2, 5):      # q_j dropped (q_0 = 0: d = 1 cannot tell)
        assert _refused(prec, d, ki, (7, 1), alr.NO_DIVIDEND) >= 10, d
    # a dropped high word of the path id, of the seed or of both: the streams of the deep cases' low words
    seed, first, _ = alr.DEEP
    for s_, f_ in ((seed % 2 ** 32, first), (seed, first % 2 ** 32), (seed % 2 ** 32, first % 2 ** 32)):
        z = br.stream(prec, s_, f_, n_normals=max(br.DS) * br.DEEP_STEPS)
        for d in (1, 8):
            assert _refused(prec, d, ki, alr.DEEP_SHAPE, None, alr.DEEP, z) >= 100, (s_, f_, d)


@pytest.mark.parametrize("dtype,bound", [(np.float64, 2.0 ** -53), (np.float32, 2.0 ** -24)])
def test_mistake_test_2_refuses(dtype, bound):
    """w started from the drift instead of 0: at d = 1 the path is no longer mcamd_price_localvol's"""
    n_steps, j, q = 5, 0, 0.03
    z = np.random.default_rng(3).standard_normal((n_steps, 20_000))
    kw = dict(observe_every=n_steps, call_level=1e6, coupon=0.03, ki_level=1.0, ki_monitoring=alr.KI_AT_MATURITY, dtype=dtype)
    right = alr.samples(z, n_steps, [alr.grid(j)], [alr.skewed(j)], [q], [[1.0]], alr.T_, alr.R, **kw)
    wrong = alr.samples(z, n_steps, [alr.grid(j)], [alr.skewed(j)], [q], [[1.0]], alr.T_, alr.R,
                        mistake=alr.W_FROM_DRIFT, **kw)
    moved = np.abs(np.asarray(wrong["y"] - right["y"], dtype=np.float64)) > bound
    assert moved.mean() > 0.2, moved.mean()
