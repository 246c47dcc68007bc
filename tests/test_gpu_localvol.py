"""GPU tests of the local-volatility pricer (mcamd_price_localvol).  Run with -m gpu on an MI355X.

  1. samples, elementwise through d_samples, against the numpy restatement (tests/localvol_restate.py) on normals drawn
     from the oracle's rocRAND-exact generator for (seed, global path id, block): the inputs of tests/test_gpu_barrier.py
     — 50, 3 and 5 steps on 4096 paths at global ids 5003.. under seed 77, and 7 steps on the deep inputs — on the
     surface SKEW: n_t = 4, n_x = 65 on [-1.5, 1.5], sigma_j(x) = (0.18 + 0.04 j)(1 + 0.5 e^-x) / 1.5, with r = 0.1,
     q = 0.03, S0 = K = 100, B = 92 (down) / 110 (up); both precisions x {no barrier, 4 kinds x 2 monitorings} x call / put;
  2. the same comparison where the slice rule and the clamp do the work: (n_t, n_steps) = (3, 50) and (7, 5), a surface
     on [-0.05, 0.05] that most paths leave on either side, the smallest surface (1 x 2) and the largest (16 x 128);
  3. a flat surface with q = 0 against mcamd_price_barrier's d_samples on the same job, all 16 barrier cases, and the
     step counters;
  4. closed forms within 4 SE: a surface that varies in time only against Black-Scholes at the rms volatility, flat
     continuous barriers at 1, 12 and 252 steps against Reiner-Rubinstein, displaced diffusion against its exact price;
  5. two surfaces alive in one context, shards, repeatability, the enqueue form;  6. refusals that need a context.

Tolerance of 1-3 (elementwise_tolerance; it comes from the restatement alone, computed on the CPU): four times the
largest elementwise difference between the float64 and longdouble restatements (fp64 kernels), or between the float32
and float64 restatements (fp32 kernels), over the kept paths of all 18 cases per precision on the 50-step inputs of
test 1, floored as in the barrier test at 1e-11 of the sample (fp64) and 2e-3 absolute (fp32).  Measured with the Philox
normals on an x86-64 CPU (80-bit longdouble): 4 x 2.66e-13 = 1.06e-12 absolute for fp64 (5.5e-14 without a
barrier); 4 x 1.18e-4 = 4.7e-4 for fp32 (4.0e-5 without a barrier), i.e. the 2e-3 floor decides there.  Barrier cases
leave out a path whose restated min_i |d_i| is below MARGIN = 2e-5 (the hit test is a discontinuity no arithmetic
reproduces to the last bit), at most 1 % of a case; the restatement leaves out at most 0.73 % on the inputs of tests
1-3.  The cases without a barrier leave out nothing: the interpolation and the clamp are continuous in X.
test_restatement_stays_under_the_spread_and_the_cap asserts, without running a kernel, that on every other input of
tests 1-3 the restatements differ by no more than twice what they do on the inputs the tolerance is taken from (largest:
the flat surface, 2.74e-13 and 9.3e-5) and stay under the cap; it
lives in this module and so runs with -m gpu."""
import importlib
import itertools
import math

import numpy as np
import pytest

import barrier_restate as br
import localvol_restate as lv
from deep_inputs import DEEP, SHALLOW, check_deep_draws_differ

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

NP_T = {capi.F64: np.float64, capi.F32: np.float32}
SUM_RTOL = {capi.F64: 1e-11, capi.F32: 2e-5}
MARGIN = 2e-5
CAP = 0.01
BASE = dict(S0=100.0, K=100.0, r=0.1, T=1.0)
Q_DIV = 0.03
B_DOWN, B_UP = 92.0, 110.0
N_LOCAL, N_STEPS = 4096, 50
MORE_INPUTS = ((3, SHALLOW), (5, SHALLOW), (7, DEEP))   # (n_steps, where) beside (N_STEPS, SHALLOW)
NONE = lv.NO_BARRIER


def skew(n_t, n_x, x_min, x_max, lo=0.18, step=0.04):
    x = np.linspace(x_min, x_max, n_x)
    return (n_t, n_x, x_min, x_max), np.array([(lo + step * j) * (1.0 + 0.5 * np.exp(-x)) / 1.5 for j in range(n_t)])


SURFACES = {
    "skew": skew(4, 65, -1.5, 1.5),
    "skew3": skew(3, 65, -1.5, 1.5),          # n_t does not divide 50 steps
    "skew7": skew(7, 65, -1.5, 1.5, 0.16, 0.03),   # more slices than the 5 steps: rows 3 and 6 are skipped
    "narrow": skew(4, 65, -0.05, 0.05),       # most paths run clamped, on either side
    "two": ((1, 2, -1.5, 1.5), np.array([[0.30, 0.14]])),
    "full": skew(16, 128, -1.5, 1.5, 0.15, 0.01),   # MCAMD_LOCALVOL_MAX_NODES nodes: 32 KiB of fp64 pairs
    "flat": ((1, 2, -1.0, 1.0), np.array([[0.2, 0.2]])),
}


def level(barrier):
    return B_UP if barrier in (lv.UP_OUT, lv.UP_IN) else B_DOWN


def option(barrier, **kw):
    # v is ignored by the call: leave something in it that any use would show
    return capi.make_option(**dict(BASE, v=float("nan"), B=level(barrier) if barrier != NONE else 0.0, **kw))


_normals = {}


def normals(prec, seed, first, n, n_steps):
    """[n_steps, n] normals of global paths first..first+n-1, as the kernels draw them (as float64 values)"""
    from oracle import pyoracle as o
    key = (prec, seed, first, n, n_steps)
    if key not in _normals:
        per, draw = (2, o.normal2_f64) if prec == capi.F64 else (4, o.normal4_f32)
        blocks = -(-n_steps // per)
        z = np.empty((blocks * per, n))
        for p in range(n):
            for k in range(blocks):
                z[k * per:(k + 1) * per, p] = draw(seed, first + p, k)
        _normals[key] = z[:n_steps]
    return _normals[key]


_restated = {}


def restate(surface, q, barrier, payoff, monitoring, prec, where, n_steps, dtype):
    """one restatement per (case, dtype), shared by every test that needs it and left unchanged"""
    key = (surface, q, barrier, payoff, monitoring, prec, where, n_steps, np.dtype(dtype).name)
    if key not in _restated:
        grid, sigma = SURFACES[surface]
        z = normals(prec, where[0], where[1], N_LOCAL, n_steps)
        _restated[key] = lv.samples(z, BASE["S0"], BASE["K"], level(barrier), BASE["T"], BASE["r"], q, grid, sigma, barrier,
                                    payoff, monitoring, dtype)
    return _restated[key]


def compare(surface, q, barrier, payoff, monitoring, prec, where, n_steps):
    """(kept mask, restated samples to compare with, restatement in the kernel's precision, largest kept difference
    between the two restatements the tolerance is taken from) — CPU only"""
    own = restate(surface, q, barrier, payoff, monitoring, prec, where, n_steps, NP_T[prec])
    other = restate(surface, q, barrier, payoff, monitoring, prec, where, n_steps,
                    np.longdouble if prec == capi.F64 else np.float64)
    keep = (own["min_abs_d"] >= MARGIN) & (other["min_abs_d"] >= MARGIN)
    spread = float(np.abs(own["y"][keep] - other["y"][keep]).max())
    # an fp64 kernel is compared with the float64 restatement, an fp32 kernel with the float64 one too
    want = own["y"] if prec == capi.F64 else other["y"]
    return keep, want, own, spread


JOBS = [(NONE, payoff, lv.DISCRETE) for payoff in (lv.CALL, lv.PUT)] + \
       list(itertools.product(lv.KINDS, (lv.CALL, lv.PUT), (lv.DISCRETE, lv.CONTINUOUS)))
CASES = [(prec, *job) for prec in (capi.F64, capi.F32) for job in JOBS]
# tests 2 and 3 beside test 1: (surface, q, n_steps, where, jobs)
FEW = [(NONE, lv.CALL, lv.DISCRETE), (lv.UP_OUT, lv.PUT, lv.CONTINUOUS), (lv.DOWN_IN, lv.CALL, lv.DISCRETE),
       (lv.DOWN_OUT, lv.CALL, lv.CONTINUOUS)]
OTHER = [("skew3", Q_DIV, 50, SHALLOW, FEW), ("skew7", Q_DIV, 5, SHALLOW, FEW), ("narrow", Q_DIV, 50, SHALLOW, FEW),
         ("two", Q_DIV, 50, SHALLOW, FEW), ("full", Q_DIV, 50, SHALLOW, FEW), ("flat", 0.0, 50, SHALLOW, JOBS[2:])]

_spread = {}


def measured_spread(prec, jobs=JOBS):
    """the largest restatement difference over the cases of test 1's 50-step inputs"""
    key = (prec, tuple(jobs))
    if key not in _spread:
        _spread[key] = max(compare("skew", Q_DIV, *job, prec, SHALLOW, N_STEPS)[3] for job in jobs)
    return _spread[key]


def elementwise_tolerance(prec, want):
    """Absolute tolerance per element: 4 x the largest restatement difference over the 18 cases of test 1's 50-step
    inputs, floored at 1e-11 of the sample (fp64) / 2e-3 (fp32).  From the restatement alone."""
    if prec == capi.F64:
        return np.maximum(4.0 * measured_spread(prec), 1e-11 * np.abs(want))
    return np.full(want.shape, max(4.0 * measured_spread(prec), 2e-3))


def _name(case, n_steps, where):
    return "-".join(str(x) for x in case) + f"-{n_steps}" + ("-deep" if where == DEEP else "")


SAMPLE_CASES = [pytest.param(*c, n_steps, where, id=_name(c, n_steps, where))
                for n_steps, where in ((N_STEPS, SHALLOW),) + MORE_INPUTS for c in CASES]
OTHER_CASES = [pytest.param(surface, q, n_steps, where, prec, *job, id=surface + "-" + _name((prec, *job), n_steps, where))
               for surface, q, n_steps, where, jobs in OTHER if surface != "flat"
               for prec in (capi.F64, capi.F32) for job in jobs]
FLAT_CASES = [pytest.param(prec, *job, id="-".join(str(x) for x in (prec, *job)))
              for prec in (capi.F64, capi.F32) for job in JOBS[2:]]


def test_restatement_stays_under_the_spread_and_the_cap():
    """no kernel runs: on every input of tests 1-3 the restatement alone leaves out at most 1 % of a case, more than 2 %
    of a case's samples are non-zero, and away from the inputs the tolerance is taken from the two restatements differ
    by no more than twice what they do on them, i.e. the restatement's own rounding uses up at most half the tolerance"""
    for prec in (capi.F64, capi.F32):
        print(f"prec {prec}: restatement spread on the 50-step inputs {measured_spread(prec):.3e} "
              f"(without a barrier {measured_spread(prec, JOBS[:2]):.3e})")
    inputs = [("skew", Q_DIV, n_steps, where, JOBS) for n_steps, where in ((N_STEPS, SHALLOW),) + MORE_INPUTS] + OTHER
    for surface, q, n_steps, where, jobs in inputs:
        spreads, left_out, nonzero = {capi.F64: 0.0, capi.F32: 0.0}, 0.0, 1.0
        for prec, job in itertools.product((capi.F64, capi.F32), jobs):
            keep, want, own, spread = compare(surface, q, *job, prec, where, n_steps)
            spreads[prec] = max(spreads[prec], spread)
            left_out, nonzero = max(left_out, 1.0 - keep.mean()), min(nonzero, (want != 0).mean())
            assert spread <= 2.0 * measured_spread(prec), (surface, n_steps, where, prec, job, spread)
            assert 1.0 - keep.mean() <= CAP and 0.02 < (want != 0).mean(), (surface, n_steps, prec, job)
            if job[0] == NONE:
                assert keep.all()
        print(f"{surface} n_steps {n_steps} first path {where[1]}: largest restatement difference "
              f"{spreads[capi.F64]:.3e} (fp64) {spreads[capi.F32]:.3e} (fp32), largest excluded fraction {left_out:.4f}, "
              f"smallest non-zero share {nonzero:.3f}")


def test_the_narrow_surface_clamps_most_paths_on_either_side():
    """no kernel runs: what makes the narrow surface worth running"""
    own = restate("narrow", Q_DIV, NONE, lv.CALL, lv.DISCRETE, capi.F64, SHALLOW, N_STEPS, np.float64)
    x = np.log(own["S_T"] / BASE["S0"])
    assert (x < -0.05).mean() > 0.2 and (x > 0.05).mean() > 0.2


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_deep_normals_are_those_of_neither_shallow_word(prec):
    """no kernel runs: the deep normals share nothing with the streams a dropped high word lands on"""
    check_deep_draws_differ(lambda seed, first: normals(prec, seed, first, 64, 7))


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
def surfaces(ctx):
    made = {name: ctx.localvol_surface(grid, sigma) for name, (grid, sigma) in SURFACES.items()}
    yield made
    for s in made.values():
        s.close()


def run(ctx, opt, sim, job, surface, want_samples=True):
    """(result, samples as float64 numpy or None)"""
    s = None
    if want_samples:
        s = torch.full((max(sim.n_paths_local, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    res = ctx.price_localvol(opt, sim, job, surface, s)
    torch.cuda.synchronize()
    return res, (s[:sim.n_paths_local].cpu().numpy().astype(np.float64) if want_samples else None)


def full_work(n, n_steps):
    return 64 * -(-n // 64) * n_steps


def check_against_the_restatement(ctx, surfaces, surface, q, prec, barrier, payoff, monitoring, n_steps, where):
    seed, first, n_job = where
    keep, want, own, spread = compare(surface, q, barrier, payoff, monitoring, prec, where, n_steps)
    tol = elementwise_tolerance(prec, want)
    excluded = 1.0 - keep.mean()
    assert excluded <= CAP, excluded
    sim = capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=N_LOCAL)
    res, got = run(ctx, option(barrier), sim, capi.make_localvol(payoff, barrier, monitoring, q), surfaces[surface])
    assert np.isfinite(got).all() and res.n == N_LOCAL and res.block == 256 and res.grid == N_LOCAL // 256
    err = np.abs(got - want)
    k = int(np.argmax(np.where(keep, err - tol, -np.inf)))
    print(f"{surface} prec {prec} barrier {barrier} payoff {payoff} monitoring {monitoring} n_steps {n_steps} first path "
          f"{first}: restatement spread {spread:.3e}, tolerance {tol[keep].min():.3e}..{tol[keep].max():.3e}, worst kept "
          f"deviation {err[keep].max():.3e}, excluded {excluded:.4f}, nonzero samples {(want != 0).mean():.3f}")
    assert (err[keep] <= tol[keep]).all(), (k, got[k], want[k], tol[k])
    assert 0.02 < (want != 0).mean()
    if barrier != NONE and monitoring == lv.CONTINUOUS:
        assert (want[keep] != own["h"][keep]).any()
    # the sums: a path near the barrier contributes whatever the kernel made of it, the others the restated values
    ref = np.where(keep, own["y"], got)
    rt = SUM_RTOL[prec]
    assert abs(res.sum - ref.sum()) <= rt * abs(ref.sum()), (res.sum, ref.sum())
    assert abs(res.sumsq - (ref * ref).sum()) <= rt * (ref * ref).sum()
    fin = capi.finalize(res.sum, res.sumsq, res.n, BASE["r"], BASE["T"])
    assert (res.price, res.std_err, res.ci_lo, res.ci_hi) == (fin.price, fin.std_err, fin.ci_lo, fin.ci_hi)
    assert res.sum_c == res.sum_cc == res.sum_yc == res.cv_beta == res.cv_rho == 0.0
    # live lane-steps are the restated ones, but for the paths left out (each can differ by at most every step)
    assert abs(res.live_steps - own["live"].sum()) <= n_steps * int((~keep).sum())
    if barrier == NONE or not lv.is_out(barrier):
        assert res.work_steps == full_work(N_LOCAL, n_steps)
    return res, got, keep


# ---- 1. samples against the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec,barrier,payoff,monitoring,n_steps,where", SAMPLE_CASES)
def test_samples_against_the_restatement(ctx, surfaces, prec, barrier, payoff, monitoring, n_steps, where):
    check_against_the_restatement(ctx, surfaces, "skew", Q_DIV, prec, barrier, payoff, monitoring, n_steps, where)


# ---- 2. the slice rule and the clamp ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("surface,q,n_steps,where,prec,barrier,payoff,monitoring", OTHER_CASES)
def test_slice_rule_clamp_and_table_sizes(ctx, surfaces, surface, q, n_steps, where, prec, barrier, payoff, monitoring):
    check_against_the_restatement(ctx, surfaces, surface, q, prec, barrier, payoff, monitoring, n_steps, where)


# ---- 3. a flat surface is the barrier pricer ---------------------------------------------------------------------------

@pytest.mark.parametrize("prec,barrier,payoff,monitoring", FLAT_CASES)
def test_flat_surface_against_the_barrier_pricer(ctx, surfaces, prec, barrier, payoff, monitoring):
    seed, first, n_job = SHALLOW
    res, got, keep = check_against_the_restatement(ctx, surfaces, "flat", 0.0, prec, barrier, payoff, monitoring, N_STEPS,
                                                   SHALLOW)
    sim = capi.make_sim(n_job, N_STEPS, prec, seed=seed, path_offset=first, n_paths_local=N_LOCAL)
    s = torch.full((N_LOCAL,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    opt = capi.make_option(**dict(BASE, v=0.2, B=level(barrier)))
    bar = ctx.price_barrier(opt, sim, capi.make_barrier(barrier, payoff, monitoring), s)
    torch.cuda.synchronize()
    want = s.cpu().numpy().astype(np.float64)
    tol = elementwise_tolerance(prec, want)
    err = np.abs(got - want)
    print(f"flat prec {prec} barrier {barrier} payoff {payoff} monitoring {monitoring}: worst kept deviation from "
          f"mcamd_price_barrier {err[keep].max():.3e}, tolerance {tol[keep].min():.3e}..{tol[keep].max():.3e}")
    assert (err[keep] <= tol[keep]).all()
    assert (res.work_steps, res.live_steps, res.n, res.grid) == (bar.work_steps, bar.live_steps, bar.n, bar.grid)
    rt = SUM_RTOL[prec]
    assert abs(res.sum - bar.sum) <= rt * bar.sum + float(np.abs(got - want)[~keep].sum())


# ---- 4. closed forms ---------------------------------------------------------------------------------------------------

def within_4_se(tag, res, want):
    print(f"{tag}: closed {want:.6f} price {res.price:.6f} SE {res.std_err:.6f} ({(res.price - want) / res.std_err:+.2f} SE) "
          f"kernel {res.kernel_ms:.3f} ms")
    assert res.std_err > 0 and abs(res.price - want) <= 4.0 * res.std_err, (tag, res.price, want, res.std_err)


@pytest.mark.parametrize("prec,payoff", [(capi.F64, lv.CALL), (capi.F64, lv.PUT), (capi.F32, lv.CALL), (capi.F32, lv.PUT)])
def test_time_only_surface_prices_to_black_scholes_at_the_rms_volatility(ctx, prec, payoff):
    """sigma depends on the slice alone: X_n is normal with variance sum s_i^2 dt whatever the step count"""
    vols = (0.15, 0.30, 0.20, 0.25)
    rms = math.sqrt(sum(v * v for v in vols) / 4)
    sim = capi.make_sim(1 << 20, 12, prec, seed=2031)
    with ctx.localvol_surface((4, 2, -1.0, 1.0), [[v, v] for v in vols]) as surface:
        res, _ = run(ctx, option(NONE), sim, capi.make_localvol(payoff, q=Q_DIV), surface, False)
    want = capi.bs_price_f64(BASE["S0"], BASE["K"], BASE["T"], BASE["r"], Q_DIV, rms, payoff)
    within_4_se(f"TIME-ONLY prec {prec} payoff {payoff}", res, want)
    assert res.work_steps == res.live_steps == full_work(1 << 20, 12)


CLOSED = [(capi.F64, kind, payoff, n_steps)
          for kind, payoff in ((lv.DOWN_OUT, lv.CALL), (lv.UP_OUT, lv.PUT), (lv.DOWN_IN, lv.PUT), (lv.UP_IN, lv.CALL))
          for n_steps in (1, 12, 252)] + [(capi.F32, lv.UP_OUT, lv.PUT, 12), (capi.F32, lv.DOWN_IN, lv.CALL, 252)]


@pytest.mark.parametrize("prec,kind,payoff,n_steps", CLOSED)
def test_flat_continuous_barrier_against_the_closed_form(ctx, surfaces, prec, kind, payoff, n_steps):
    sim = capi.make_sim(1 << 20, n_steps, prec, seed=2024 + n_steps)
    res, _ = run(ctx, option(kind), sim, capi.make_localvol(payoff, kind, lv.CONTINUOUS), surfaces["flat"], False)
    want = capi.barrier_price_f64(BASE["S0"], BASE["K"], level(kind), BASE["T"], BASE["r"], 0.2, kind, payoff)
    within_4_se(f"FLAT BARRIER prec {prec} kind {kind} payoff {payoff} n_steps {n_steps}", res, want)


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_displaced_diffusion_against_its_exact_price(ctx, prec):
    """r = q = 0, sigma(x) = sigma_d (1 + a / (S0 e^x)) on 65 nodes: call(K) = BS(S0 + a, K + a, sigma_d)"""
    S0, a, sigma_d = 100.0, 50.0, 0.2 * 100.0 / 150.0
    x = np.linspace(-1.5, 1.5, 65)
    sim = capi.make_sim(1 << 19, 64, prec, seed=909)
    with ctx.localvol_surface((1, 65, -1.5, 1.5), [sigma_d * (1.0 + a / (S0 * np.exp(x)))]) as surface:
        for K in (80.0, 100.0, 125.0):
            opt = capi.make_option(S0=S0, K=K, r=0.0, T=1.0, v=0.0)
            res, _ = run(ctx, opt, sim, capi.make_localvol(lv.CALL), surface, False)
            within_4_se(f"DISPLACED prec {prec} K {K}", res, capi.bs_price_f64(S0 + a, K + a, 1.0, 0.0, 0.0, sigma_d))


# ---- 5. state and ordering -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_two_surfaces_alive_in_one_context(ctx, surfaces, prec):
    """priced alternately, enqueued back to back without a wait between them: each call sees its own table"""
    sim = capi.make_sim(10_000, 13, prec, seed=21)
    opt, job = option(NONE), capi.make_localvol(lv.PUT, q=Q_DIV)
    names = ("skew", "two", "full", "flat")
    alone = {name: run(ctx, opt, sim, job, surfaces[name])[1] for name in names}
    assert all(not np.array_equal(alone[a], alone[b]) for a, b in itertools.combinations(names, 2))
    stats = [torch.zeros(6, dtype=torch.float64, device="cuda") for _ in range(8)]
    outs = [torch.full((10_000,), float("nan"), dtype=TORCH_T[prec], device="cuda") for _ in range(8)]
    for i in range(8):
        ctx.price_localvol_enqueue(opt, sim, job, surfaces[names[i % 4]], stats[i], outs[i])
    torch.cuda.synchronize()
    for i in range(8):
        assert np.array_equal(outs[i].cpu().numpy().astype(np.float64), alone[names[i % 4]])
    # a surface created and closed in between disturbs none of the others
    with ctx.localvol_surface((1, 2, -1.0, 1.0), [[0.9, 0.9]]) as extra:
        _, y = run(ctx, opt, sim, job, extra)
    assert not np.array_equal(y, alone["flat"])
    assert np.array_equal(run(ctx, opt, sim, job, surfaces["skew"])[1], alone["skew"])


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("cuts", [(0, 4097, 10_001), (0, 1, 6000, 10_001), (0, 5000, 5000, 10_001)])
def test_shards_reproduce_the_whole_job(ctx, surfaces, prec, cuts):
    n, n_steps, kind = 10_001, 50, lv.DOWN_OUT
    job = capi.make_localvol(lv.CALL, kind, lv.CONTINUOUS, Q_DIV)
    whole, y = run(ctx, option(kind), capi.make_sim(n, n_steps, prec, seed=3), job, surfaces["skew"])
    total, totsq, count = 0.0, 0.0, 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sim = capi.make_sim(n, n_steps, prec, seed=3, path_offset=lo, n_paths_local=hi - lo)
        part, y_part = run(ctx, option(kind), sim, job, surfaces["skew"])
        if hi == lo:
            assert all(v == 0 for v in part.as_dict().values())
            continue
        assert np.array_equal(y_part, y[lo:hi])
        total, totsq, count = total + part.sum, totsq + part.sumsq, count + part.n
    assert count == n and abs(total - whole.sum) <= 1e-11 * whole.sum and abs(totsq - whole.sumsq) <= 1e-11 * whole.sumsq


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("n", [3000, 3_000_000])   # one wave of workgroups; beyond the 8192-workgroup cap (grid-stride)
@pytest.mark.parametrize("barrier", [NONE, lv.UP_OUT])
def test_same_bits_twice_and_from_the_enqueue_form(ctx, surfaces, prec, n, barrier):
    n_steps = 13
    opt, job = option(barrier), capi.make_localvol(lv.PUT, barrier, lv.CONTINUOUS, Q_DIV)
    sim = capi.make_sim(n + 9, n_steps, prec, seed=4, path_offset=9, n_paths_local=n)
    a, y_a = run(ctx, opt, sim, job, surfaces["skew"])
    b, y_b = run(ctx, opt, sim, job, surfaces["skew"])
    assert np.array_equal(y_a, y_b) and (a.sum, a.sumsq, a.work_steps, a.live_steps) == (b.sum, b.sumsq, b.work_steps,
                                                                                         b.live_steps)
    assert a.grid == min(-(-n // 256), 8192) and a.sum > 0
    assert 0 < a.live_steps <= a.work_steps <= full_work(n, n_steps)
    if barrier == NONE:
        assert a.live_steps == n * n_steps and a.work_steps == full_work(n, n_steps)
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.full((n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    ctx.price_localvol_enqueue(opt, sim, job, surfaces["skew"], stats, s)
    ms = ctx.enqueued_kernel_ms(1)
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    assert rec.tolist() == [a.sum, a.sumsq, 0.0, 0.0, 0.0, float(n)]
    assert np.array_equal(s.cpu().numpy().astype(np.float64), y_a)
    fin = capi.finalize_stats(rec, BASE["r"], BASE["T"])
    assert (fin.price, fin.std_err, fin.n) == (a.price, a.std_err, n)
    assert 0.0 < ms[0] < 1e4
    # an empty shard: zeros, still ordered on the stream
    ctx.price_localvol_enqueue(opt, capi.make_sim(n, n_steps, prec, seed=4, path_offset=5, n_paths_local=0), job,
                               surfaces["skew"], stats)
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()


def test_a_knock_out_wavefront_leaves_early(ctx, surfaces):
    """a barrier just beside the spot knocks whole wavefronts before maturity (tests/test_gpu_barrier.py, test 7)"""
    n, n_steps = 100_000, 51
    for prec in (capi.F64, capi.F32):
        opt = capi.make_option(**dict(BASE, v=0.0, B=100.1))
        res, _ = run(ctx, opt, capi.make_sim(n, n_steps, prec, seed=6),
                     capi.make_localvol(lv.CALL, lv.UP_OUT, lv.DISCRETE), surfaces["flat"], False)
        assert 0 < res.live_steps <= res.work_steps < full_work(n, n_steps) and res.work_steps % 64 == 0


# ---- 6. refusals that need a context -----------------------------------------------------------------------------------

def test_refusals_with_a_live_context(ctx, surfaces):
    opt, job, sim = option(NONE), capi.make_localvol(), capi.make_sim(1000, 12)
    ok, _ = run(ctx, opt, sim, job, surfaces["skew"], False)
    same, _ = run(ctx, opt, capi.make_sim(1000, 12, flags=capi.FLAG_LOG_SPACE), job, surfaces["skew"], False)
    assert (ok.sum, ok.sumsq) == (same.sum, same.sumsq) and ok.sum > 0
    stats = torch.zeros(6, dtype=torch.float64, device="cuda")
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_PRODUCT_FORM, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE,
                  capi.FLAG_LOG_SPACE | capi.FLAG_PRODUCT_FORM):
        with pytest.raises(capi.McamdError) as e:
            ctx.price_localvol(opt, capi.make_sim(1000, 12, flags=flags), job, surfaces["skew"])
        assert e.value.code == capi.ERR_INVALID and "flags" in str(e.value)
        with pytest.raises(capi.McamdError):
            ctx.price_localvol_enqueue(opt, capi.make_sim(1000, 12, flags=flags), job, surfaces["skew"], stats)
    # a surface serves the context it was created on and no other
    other = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        with other.localvol_surface(*SURFACES["skew"]) as foreign:
            for call in (lambda: ctx.price_localvol(opt, sim, job, foreign),
                         lambda: ctx.price_localvol_enqueue(opt, sim, job, foreign, stats)):
                with pytest.raises(capi.McamdError) as e:
                    call()
                assert e.value.code == capi.ERR_INVALID and "another context" in str(e.value)
            mine = other.price_localvol(opt, sim, job, foreign)
            assert (mine.sum, mine.sumsq) == (ok.sum, ok.sumsq)
    finally:
        other.close()
    # a table the grid does not admit is refused with a live context too, and leaves no surface behind
    with pytest.raises(capi.McamdError) as e:
        ctx.localvol_surface((2, 2, -1.0, 1.0), [[0.2, 0.2], [0.2, -0.2]])
    assert e.value.code == capi.ERR_INVALID and "finite and > 0" in str(e.value)
    # the fp64 exponent-range bound is taken at the surface's largest entry
    with ctx.localvol_surface((1, 2, -1.0, 1.0), [[0.2, 100.0]]) as wild:
        with pytest.raises(capi.McamdError) as e:
            ctx.price_localvol(capi.make_option(**dict(BASE, T=100.0, v=0.0)), capi.make_sim(1000, 50), job, wild)
        assert e.value.code == capi.ERR_INVALID and "exponent range" in str(e.value)
    # an empty shard: all zeros, nothing launched
    res, _ = run(ctx, opt, capi.make_sim(1000, 12, path_offset=10, n_paths_local=0), job, surfaces["skew"], False)
    assert all(v == 0 for v in res.as_dict().values())
