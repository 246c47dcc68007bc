"""GPU tests of the single-barrier pricer (mcamd_price_barrier).  Run with -m gpu on an MI355X.

  1. samples, elementwise through d_samples, against the numpy restatement (tests/barrier_restate.py) on normals drawn
     from the oracle's rocRAND-exact generator for (seed, global path id, block): 50, 3 and 5 steps on 4096 paths at
     global ids 5003.. under seed 77, and 7 steps on the deep inputs, ids 2^33 + 5003.. of a job of 2^40 paths under
     seed 2^40 + 77.  The last, partial Philox block of a path is a branch of its own in the kernel: these step counts
     leave 2, 3, 1 and 3 of its 4 normals in fp32 and 0, 1, 1 and 1 of its 2 in fp64;
  2. the discrete down-barrier calls against the bullet window of mcamd_price_paths; in + out = European;
  3. continuous monitoring against the Reiner-Rubinstein closed form within 4 SE at n_steps 1, 12 and 252;
  4. discrete >= continuous sample for sample;  5. shards;  6. repeatability and the enqueue form;
  7. the work counters;  8. flags.

Tolerance of 1 (compare / elementwise_tolerance below; it comes from the restatement alone, computed on the
CPU): four times the largest elementwise difference between the float64 and longdouble restatements (fp64 kernels),
or between the float32 and float64 restatements (fp32 kernels), over the kept paths of all 16 kind x payoff x
monitoring cases on the test's own inputs — S0 = K = 100, r = 0.1, v = 0.2, T = 1, B = 92 (down) / 110 (up),
50 steps, 4096 paths at global ids 5003.., seed 77 — floored at 1e-11 of the sample (fp64) and 2e-3 absolute (fp32).
Measured on an x86-64 CPU (80-bit longdouble): 4 x 2.74e-13 = 1.10e-12 absolute for fp64; 4 x 8.73e-5 = 3.5e-4 for
fp32, i.e. the 2e-3 floor decides there.  A path whose restated min_i |d_i| is below MARGIN = 2e-5 (natural-log units) is
left out: the hit test is a discontinuity no arithmetic reproduces to the last bit, and a bridge factor's relative
error grows like ulp(X) / d.  The restatement leaves out at most 0.46 % of a case's paths on these inputs (cap: 1 %).
The tolerance is taken from the 50-step inputs alone.  On the other inputs of test 1 (MORE_INPUTS) the restatements
differ by less — at most 8.6e-14 (fp64) and 4.7e-5 (fp32), 0.10 % of a case left out, at least 3.8 % of a case's samples
non-zero — which test_added_inputs_stay_under_the_spread_and_the_cap asserts; like the exclusion-cap check it runs no
kernel, but it lives in this module and so runs with -m gpu.  One step is not among them:
a knock-in pays nothing then."""
import importlib
import itertools
import math

import numpy as np
import pytest

import barrier_restate as br
from deep_inputs import DEEP, SHALLOW, check_deep_draws_differ

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

NP_T = {capi.F64: np.float64, capi.F32: np.float32}
SUM_RTOL = {capi.F64: 1e-11, capi.F32: 2e-5}
MARGIN = 2e-5
CAP = 0.01
BASE = dict(S0=100.0, K=100.0, r=0.1, v=0.2, T=1.0)
B_DOWN, B_UP = 92.0, 110.0
N_JOB, OFFSET, N_LOCAL, N_STEPS, SEED = 20_000, 5003, 4096, 50, 77
assert SHALLOW == (SEED, OFFSET, N_JOB)   # (seed, first path, paths of the job); DEEP: tests/deep_inputs.py
MORE_INPUTS = ((3, SHALLOW), (5, SHALLOW), (7, DEEP))                        # (n_steps, where) beside (N_STEPS, SHALLOW)


def level(kind):
    return B_UP if br.is_up(kind) else B_DOWN


def option(kind, **kw):
    return capi.make_option(**dict(BASE, B=level(kind), **kw))


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


def restate(prec, kind, payoff, monitoring, z, dtype=None):
    dtype = dtype or NP_T[prec]
    return br.samples(z, BASE["S0"], BASE["K"], level(kind), BASE["T"], BASE["r"], BASE["v"], kind, payoff, monitoring,
                      dtype)


def compare(prec, kind, payoff, monitoring, z):
    """(kept mask, restated samples to compare with, restatement in the kernel's precision, largest kept difference
    between the two restatements the tolerance is taken from) — CPU only"""
    own = restate(prec, kind, payoff, monitoring, z)
    other = restate(prec, kind, payoff, monitoring, z, np.longdouble if prec == capi.F64 else np.float64)
    keep = (own["min_abs_d"] >= MARGIN) & (other["min_abs_d"] >= MARGIN)
    spread = float(np.abs(own["y"][keep] - other["y"][keep]).max())
    # an fp64 kernel is compared with the float64 restatement, an fp32 kernel with the float64 one too
    want = own["y"] if prec == capi.F64 else other["y"]
    return keep, want, own, spread


_spread = {}


def measured_spread(prec):
    """the largest restatement difference over the 16 cases of test 1's 50-step inputs"""
    if prec not in _spread:
        z = normals(prec, SEED, OFFSET, N_LOCAL, N_STEPS)
        _spread[prec] = max(compare(prec, kind, payoff, monitoring, z)[3]
                            for kind, payoff, monitoring in itertools.product(br.KINDS, (br.CALL, br.PUT),
                                                                              (br.DISCRETE, br.CONTINUOUS)))
    return _spread[prec]


def elementwise_tolerance(prec, want):
    """Absolute tolerance per element: 4 x the largest restatement difference over the 16 cases of test 1's inputs,
    floored at 1e-11 of the sample (fp64) / 2e-3 (fp32).  From the restatement alone."""
    if prec == capi.F64:
        return np.maximum(4.0 * measured_spread(prec), 1e-11 * np.abs(want))
    return np.full(want.shape, max(4.0 * measured_spread(prec), 2e-3))


CASES = list(itertools.product((capi.F64, capi.F32), br.KINDS, (br.CALL, br.PUT), (br.DISCRETE, br.CONTINUOUS)))


def _name(case, n_steps, where):
    return "-".join(str(x) for x in case) + f"-{n_steps}" + ("-deep" if where == DEEP else "")


# the ids of the 50-step cases are those pytest gave them before there were others
SAMPLE_CASES = [pytest.param(*c, N_STEPS, SHALLOW, id="-".join(str(x) for x in c)) for c in CASES] + \
               [pytest.param(*c, n_steps, where, id=_name(c, n_steps, where)) for n_steps, where in MORE_INPUTS for c in CASES]


def test_restatement_stays_under_the_exclusion_cap():
    """no kernel runs: on the inputs of test 1 the restatement alone leaves out less than 1 % of every case"""
    worst = 0.0
    for prec, kind, payoff, monitoring in CASES:
        z = normals(prec, SEED, OFFSET, N_LOCAL, N_STEPS)
        keep, want, own, spread = compare(prec, kind, payoff, monitoring, z)
        worst = max(worst, 1.0 - keep.mean())
        assert 1.0 - keep.mean() <= CAP
    print(f"largest excluded fraction {worst:.4f}")


def test_added_inputs_stay_under_the_spread_and_the_cap():
    """no kernel runs: on MORE_INPUTS the two restatements differ by no more than on the inputs the tolerance is taken
    from, leave out less than 1 % of every case, and more than 2 % of every case's samples are non-zero"""
    for n_steps, where in MORE_INPUTS:
        spreads, left_out, nonzero = {capi.F64: 0.0, capi.F32: 0.0}, 0.0, 1.0
        for prec, kind, payoff, monitoring in CASES:
            z = normals(prec, where[0], where[1], N_LOCAL, n_steps)
            keep, want, own, spread = compare(prec, kind, payoff, monitoring, z)
            spreads[prec] = max(spreads[prec], spread)
            left_out, nonzero = max(left_out, 1.0 - keep.mean()), min(nonzero, (want != 0).mean())
            assert spread <= measured_spread(prec), (n_steps, where, prec, kind, payoff, monitoring, spread)
            assert 1.0 - keep.mean() <= CAP and 0.02 < (want != 0).mean()
        print(f"n_steps {n_steps} first path {where[1]}: largest restatement difference {spreads[capi.F64]:.3e} (fp64; the "
              f"tolerance's {measured_spread(capi.F64):.3e}) {spreads[capi.F32]:.3e} (fp32; {measured_spread(capi.F32):.3e}), "
              f"largest excluded fraction {left_out:.4f}, smallest non-zero share {nonzero:.3f}")


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_deep_normals_are_those_of_neither_shallow_word(prec):
    """no kernel runs.  What makes the deep cases worth running: the deep normals share nothing with the streams a
    dropped high word of the path id or of the seed lands on (tests/deep_inputs.py)."""
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


def run(ctx, opt, sim, bar, want_samples=True):
    """(result, samples as float64 numpy or None)"""
    s = None
    if want_samples:
        s = torch.full((max(sim.n_paths_local, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    res = ctx.price_barrier(opt, sim, bar, s)
    torch.cuda.synchronize()
    return res, (s[:sim.n_paths_local].cpu().numpy().astype(np.float64) if want_samples else None)


def full_work(n, n_steps):
    return 64 * -(-n // 64) * n_steps


# ---- 1. samples against the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec,kind,payoff,monitoring,n_steps,where", SAMPLE_CASES)
def test_samples_against_the_restatement(ctx, prec, kind, payoff, monitoring, n_steps, where):
    seed, first, n_job = where
    z = normals(prec, seed, first, N_LOCAL, n_steps)
    keep, want, own, spread = compare(prec, kind, payoff, monitoring, z)
    tol = elementwise_tolerance(prec, want)
    excluded = 1.0 - keep.mean()
    assert excluded <= CAP, excluded
    sim = capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=N_LOCAL)
    res, got = run(ctx, option(kind), sim, capi.make_barrier(kind, payoff, monitoring))
    assert np.isfinite(got).all() and res.n == N_LOCAL and res.block == 256 and res.grid == N_LOCAL // 256
    err = np.abs(got - want)
    k = int(np.argmax(np.where(keep, err - tol, -np.inf)))
    print(f"prec {prec} kind {kind} payoff {payoff} monitoring {monitoring} n_steps {n_steps} first path {first}: "
          f"restatement spread {spread:.3e}, "
          f"tolerance {tol[keep].min():.3e}..{tol[keep].max():.3e}, worst kept deviation {err[keep].max():.3e}, "
          f"excluded {excluded:.4f}, nonzero samples {(want != 0).mean():.3f}")
    assert (err[keep] <= tol[keep]).all(), (k, got[k], want[k], tol[k])
    assert 0.02 < (want != 0).mean() and (monitoring == br.DISCRETE or (want[keep] != own["h"][keep]).any())
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


# ---- 2. agreement with what exists -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("n_steps", [50, 7])
def test_discrete_down_calls_are_the_bullet_window(ctx, prec, n_steps):
    n, rt = 100_000, SUM_RTOL[prec]
    sim = capi.make_sim(n, n_steps, prec, seed=11)
    for kind, P1, P2 in ((br.DOWN_OUT, 0, 0), (br.DOWN_IN, 1, n_steps)):
        res, _ = run(ctx, option(kind), sim, capi.make_barrier(kind, br.CALL, br.DISCRETE), False)
        bullet = ctx.price_paths(option(kind, P1=P1, P2=P2, use_window=1), sim)
        assert res.n == bullet.n == n and res.sum > 0
        assert abs(res.sum - bullet.sum) <= rt * bullet.sum and abs(res.sumsq - bullet.sumsq) <= rt * bullet.sumsq


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("kind,payoff", [(br.DOWN_OUT, br.CALL), (br.UP_OUT, br.CALL), (br.DOWN_OUT, br.PUT)])
def test_in_plus_out_is_the_european_payoff(ctx, prec, kind, payoff):
    n, n_steps, rt = 50_000, 50, SUM_RTOL[prec]
    sim = capi.make_sim(n, n_steps, prec, seed=12)
    out, y_out = run(ctx, option(kind), sim, capi.make_barrier(kind, payoff, br.DISCRETE))
    inn, y_in = run(ctx, option(kind), sim, capi.make_barrier(kind + 1, payoff, br.DISCRETE))
    assert ((y_out == 0) | (y_in == 0)).all() and (y_out != 0).any() and (y_in != 0).any()
    if payoff == br.CALL:
        eur = ctx.price_paths(capi.make_option(**BASE), sim)
        assert abs(out.sum + inn.sum - eur.sum) <= rt * eur.sum
    # per path: h(S_T), which the far-barrier knock-out returns
    far = capi.make_option(**dict(BASE, B=1e-3 if kind == br.DOWN_OUT else 1e7))
    _, h = run(ctx, far, sim, capi.make_barrier(kind, payoff, br.DISCRETE))
    assert np.array_equal(y_out + y_in, h)


# ---- 3. the closed form ------------------------------------------------------------------------------------------------------

CLOSED = [(capi.F64, kind, payoff, n_steps) for kind, payoff in itertools.product(br.KINDS, (br.CALL, br.PUT))
          for n_steps in (1, 12, 252)] + [(capi.F32, br.UP_OUT, br.PUT, 12)]


@pytest.mark.parametrize("prec,kind,payoff,n_steps", CLOSED)
def test_continuous_monitoring_against_the_closed_form(ctx, prec, kind, payoff, n_steps):
    n = 4_000_000
    sim = capi.make_sim(n, n_steps, prec, seed=2024 + n_steps)
    res, _ = run(ctx, option(kind), sim, capi.make_barrier(kind, payoff, br.CONTINUOUS), False)
    want = capi.barrier_price_f64(BASE["S0"], BASE["K"], level(kind), BASE["T"], BASE["r"], BASE["v"], kind, payoff)
    print(f"BARRIER prec {prec} kind {kind} payoff {payoff} n_steps {n_steps}: closed {want:.6f} price {res.price:.6f} "
          f"SE {res.std_err:.6f} ({(res.price - want) / res.std_err:+.2f} SE) live/work "
          f"{res.live_steps / res.work_steps:.4f} kernel {res.kernel_ms:.3f} ms")
    assert res.std_err > 0 and abs(res.price - want) <= 4.0 * res.std_err, (res.price, want, res.std_err)


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("payoff", [br.CALL, br.PUT])
def test_a_far_barrier_leaves_the_european_price(ctx, prec, payoff):
    """B so far away that every q >= Q: no factor is applied, w = 1 exactly"""
    n, n_steps, rt = 200_000, 12, SUM_RTOL[prec]
    sim = capi.make_sim(n, n_steps, prec, seed=5)
    for kind, B in ((br.DOWN_OUT, 1e-3), (br.UP_OUT, 1e7)):
        opt = capi.make_option(**dict(BASE, B=B))
        out, y = run(ctx, opt, sim, capi.make_barrier(kind, payoff, br.CONTINUOUS))
        disc, y_d = run(ctx, opt, sim, capi.make_barrier(kind, payoff, br.DISCRETE))
        inn, y_in = run(ctx, opt, sim, capi.make_barrier(kind + 1, payoff, br.CONTINUOUS))
        assert np.array_equal(y, y_d) and out.sum == disc.sum and out.sumsq == disc.sumsq
        assert inn.sum == 0.0 and inn.sumsq == 0.0 and inn.price == 0.0 and not y_in.any()
        if payoff == br.CALL:
            eur = ctx.price_paths(capi.make_option(**BASE), sim)
            assert abs(out.sum - eur.sum) <= rt * eur.sum and abs(out.price - eur.price) <= rt * eur.price


# ---- 4. ordering -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("kind,payoff", [(br.DOWN_OUT, br.CALL), (br.UP_OUT, br.PUT), (br.UP_OUT, br.CALL)])
def test_discrete_knock_out_dominates_the_continuous_one(ctx, prec, kind, payoff):
    sim = capi.make_sim(100_000, 12, prec, seed=8)
    d, y_d = run(ctx, option(kind), sim, capi.make_barrier(kind, payoff, br.DISCRETE))
    c, y_c = run(ctx, option(kind), sim, capi.make_barrier(kind, payoff, br.CONTINUOUS))
    assert (y_d >= y_c).all() and (y_d > y_c).any() and d.sum > c.sum
    assert ((y_c == 0) | (y_d > 0)).all()   # w_continuous > 0 only where w_discrete = 1


# ---- 5. sharding -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("cuts", [(0, 4097, 10_001), (0, 1, 6000, 10_001), (0, 5000, 5000, 10_001)])
def test_shards_reproduce_the_whole_job(ctx, prec, cuts):
    n, n_steps, kind = 10_001, 50, br.DOWN_OUT
    bar = capi.make_barrier(kind, br.CALL, br.CONTINUOUS)
    whole, y = run(ctx, option(kind), capi.make_sim(n, n_steps, prec, seed=3), bar)
    total, totsq, count = 0.0, 0.0, 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sim = capi.make_sim(n, n_steps, prec, seed=3, path_offset=lo, n_paths_local=hi - lo)
        part, y_part = run(ctx, option(kind), sim, bar)
        if hi == lo:
            assert all(v == 0 for v in part.as_dict().values())
            continue
        assert np.array_equal(y_part, y[lo:hi])
        total, totsq, count = total + part.sum, totsq + part.sumsq, count + part.n
    assert count == n and abs(total - whole.sum) <= 1e-11 * whole.sum and abs(totsq - whole.sumsq) <= 1e-11 * whole.sumsq


# ---- 6. repeatability and the enqueue form -----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("n", [3000, 3_000_000])   # one wave of workgroups; beyond the 8192-workgroup cap (grid-stride)
def test_same_bits_twice_and_from_the_enqueue_form(ctx, prec, n):
    kind, n_steps = br.UP_IN, 13
    opt, bar = option(kind), capi.make_barrier(kind, br.PUT, br.CONTINUOUS)
    sim = capi.make_sim(n + 9, n_steps, prec, seed=4, path_offset=9, n_paths_local=n)
    a, y_a = run(ctx, opt, sim, bar)
    b, y_b = run(ctx, opt, sim, bar)
    assert np.array_equal(y_a, y_b) and (a.sum, a.sumsq, a.work_steps, a.live_steps) == (b.sum, b.sumsq, b.work_steps,
                                                                                         b.live_steps)
    assert a.grid == min(-(-n // 256), 8192) and a.sum > 0
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.full((n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    ctx.price_barrier_enqueue(opt, sim, bar, stats, s)
    ms = ctx.enqueued_kernel_ms(1)
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    assert rec.tolist() == [a.sum, a.sumsq, 0.0, 0.0, 0.0, float(n)]
    assert np.array_equal(s.cpu().numpy().astype(np.float64), y_a)
    fin = capi.finalize_stats(rec, BASE["r"], BASE["T"])
    assert (fin.price, fin.std_err, fin.n) == (a.price, a.std_err, n)
    assert 0.0 < ms[0] < 1e4
    # an empty shard: zeros, still ordered on the stream
    ctx.price_barrier_enqueue(opt, capi.make_sim(n, n_steps, prec, seed=4, path_offset=5, n_paths_local=0), bar, stats)
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()


# ---- 7. the work counters ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("monitoring", [br.DISCRETE, br.CONTINUOUS])
def test_work_counters(ctx, prec, monitoring):
    n, n_steps = 10_000, 51
    sim = capi.make_sim(n, n_steps, prec, seed=6)
    full = full_work(n, n_steps)
    for kind in br.KINDS:
        res, _ = run(ctx, option(kind), sim, capi.make_barrier(kind, br.CALL, monitoring), False)
        assert 0 < res.live_steps <= res.work_steps <= full, (kind, res.live_steps, res.work_steps, full)
        if not br.is_out(kind):
            assert res.work_steps == full
    # knock-in and knock-out walk the same paths: the same live lane-steps
    a, _ = run(ctx, option(br.DOWN_OUT), sim, capi.make_barrier(br.DOWN_OUT, br.CALL, monitoring), False)
    b, _ = run(ctx, option(br.DOWN_IN), sim, capi.make_barrier(br.DOWN_IN, br.CALL, monitoring), False)
    assert a.live_steps == b.live_steps
    # A barrier just beside the spot, with the drift towards it, knocks whole wavefronts early.  About 4-5 % of the paths
    # survive all 51 dates (Brownian hitting probability with the discrete-monitoring shift 0.5826 v sqrt(dt)), so a
    # wavefront is fully knocked with probability ~0.95^64 = 4 %: some 60 of the 1563 wavefronts leave early.
    big = capi.make_sim(100_000, n_steps, prec, seed=6)
    for kind, B, r, v in ((br.DOWN_OUT, 99.9, 0.0, 0.4), (br.UP_OUT, 100.1, 0.1, 0.2)):
        res, _ = run(ctx, capi.make_option(**dict(BASE, B=B, r=r, v=v)), big, capi.make_barrier(kind, br.CALL, monitoring),
                     False)
        assert 0 < res.live_steps <= res.work_steps < full_work(100_000, n_steps), (kind, res.work_steps)
        assert res.work_steps % 64 == 0


# ---- 8. flags ----------------------------------------------------------------------------------------------------------------

def test_flags_with_a_live_context(ctx):
    opt, bar = option(br.DOWN_OUT), capi.make_barrier()
    ok, _ = run(ctx, opt, capi.make_sim(1000, 12), bar, False)
    same, _ = run(ctx, opt, capi.make_sim(1000, 12, flags=capi.FLAG_LOG_SPACE), bar, False)
    assert (ok.sum, ok.sumsq) == (same.sum, same.sumsq) and ok.sum > 0
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_PRODUCT_FORM, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE,
                  capi.FLAG_LOG_SPACE | capi.FLAG_PRODUCT_FORM):
        with pytest.raises(capi.McamdError) as e:
            ctx.price_barrier(opt, capi.make_sim(1000, 12, flags=flags), bar)
        assert e.value.code == capi.ERR_INVALID and "flags" in str(e.value)
        stats = torch.zeros(6, dtype=torch.float64, device="cuda")
        with pytest.raises(capi.McamdError):
            ctx.price_barrier_enqueue(opt, capi.make_sim(1000, 12, flags=flags), bar, stats)
    # an empty shard: all zeros, nothing launched
    res, _ = run(ctx, opt, capi.make_sim(1000, 12, path_offset=10, n_paths_local=0), bar, False)
    assert all(v == 0 for v in res.as_dict().values())
