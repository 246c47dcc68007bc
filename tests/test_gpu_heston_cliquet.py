"""GPU tests of the Heston cliquet pricer (mcamd_price_heston_cliquet).  Run with -m gpu on an MI355X.

  1. samples, elementwise through d_samples, against the numpy restatement (tests/heston_cliquet_restate.py) on the two
     normal streams drawn from the oracle's rocRAND-exact generator: 256 paths per case, the shapes, jobs and inputs of
     tests/heston_cliquet_cases.py (three kinds x both precisions on F and N, fp64 on H); the counters against the
     restated flags, truncated_steps and mean_variance against the restated ones;
  2. identities: at xi = 0, kappa = 0 against mcamd_price_cliquet's own samples on a flat surface; one unbounded period
     of SUM against mcamd_price_heston's S_T; mean_variance and truncated_steps against mcamd_price_heston's;
  3. shards, repeatability, the enqueue record, eight calls back to back, an empty shard, the refusals with a context;
  4. one statistical run on F against the closed form (mcamd_heston_cliquet_price_f64).

Tolerance of 1 and 2 (heston_cliquet_cases.tolerance; from the restatement alone, computed on the CPU): four times the
largest elementwise difference between the two restatements over all jobs on the (48, 4, 1) shape of the input, floored
at 1e-13 (fp64) / 2e-5 (fp32) per unit of notional.  n_floored and n_capped may differ from the restated counts by at
most the number of paths whose restated A lies within that tolerance of the bound, at most 2 % of a case.
truncated_steps: exact in fp64; in fp32 it may differ by the number of paths whose restated |v_i| comes within 1e-6 of
0 (tests/heston_cases.py), at most 2 % of a case."""
import importlib
import math

import numpy as np
import pytest

import heston_cases as hc
import heston_cliquet_cases as cases
import heston_cliquet_restate as hq
import heston_restate as hr
from deep_inputs import SHALLOW

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

S0, T_, R, Q = hr.S0, hr.T_, hr.R, hr.Q_DIV
N_LOCAL = cases.N_LOCAL
PRECS = (capi.F64, capi.F32)
INF = float("inf")
SUM, COMPOUND, VARIANCE = hq.SUM, hq.COMPOUND, hq.VARIANCE

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


def option(K=float("nan")):
    # v, K and B are ignored by the call: leave something in them that any use would show
    return capi.make_option(S0=S0, K=K, r=R, T=T_, v=float("nan"), B=float("nan"))


def model(name, **changes):
    q, v0, kappa, theta, xi, rho = hr.params(name, **changes)
    return capi.make_heston(capi.PAYOFF_CALL, q, v0, kappa, theta, xi, rho)


def make(job, reset_every, first_period=1, q=Q):
    return capi.make_cliquet(job[0], reset_every, first_period, *job[1:], q)


def shard(prec, n_steps, where, n=N_LOCAL):
    seed, first, n_job = where
    return capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=n)


def run(ctx, sim, hs, cq, want_samples=True):
    """(result, samples as float64 numpy or None)"""
    s = None
    if want_samples:
        s = torch.full((max(sim.n_paths_local, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    res = ctx.price_heston_cliquet(option(), sim, hs, cq, s)
    torch.cuda.synchronize()
    return res, (s[:sim.n_paths_local].cpu().numpy().astype(np.float64) if want_samples else None)


def full_work(n, n_steps):
    return 64 * -(-n // 64) * n_steps


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- 1. against the restatement ----------------------------------------------------------------------------------------

PARITY = [pytest.param(prec, name, shape, id=f"{prec}-{name}-{cases.shape_name(shape)}")
          for shape in cases.SHAPES for name, precs in cases.MODELS for prec in precs]


@pytest.mark.parametrize("prec,name,shape", PARITY)
def test_samples_and_counters_against_the_restatement(ctx, prec, name, shape):
    n_steps, reset_every, first, where = shape
    tol = cases.tolerance(prec, name)
    rv_tol = hc.tolerance(prec, name)["rv"]   # test_gpu_heston.py's, for the same quantity
    for job in cases.JOBS:
        want, own, spread = cases.compare(prec, name, job, shape)
        res, got = run(ctx, shard(prec, n_steps, where), model(name), make(job, reset_every, first))
        assert np.isfinite(got).all()
        assert (res.n, res.block, res.grid) == (N_LOCAL, 256, 1) and res.work_steps == full_work(N_LOCAL, n_steps)
        err = np.abs(got - f64(want["y"]))
        k = int(np.argmax(err))
        near_floor, near_cap = cases.near(want, job, tol)
        near_zero = int((want["min_abs_v"] < hc.NEAR_ZERO).sum())
        rv_err = abs(res.mean_variance - float(f64(want["rv"]).mean()))
        print(f"{name} fp{prec} {cases.shape_name(shape)} job {cases.job_name(job)}: restatement spread {spread:.3e}, "
              f"tolerance {tol:.3e}, worst deviation {err.max():.3e}; floored {res.n_floored} (restated "
              f"{int(want['floored'].sum())}, near {int(near_floor.sum())}), capped {res.n_capped} (restated "
              f"{int(want['capped'].sum())}, near {int(near_cap.sum())}); truncated {res.truncated_steps:.0f} (restated "
              f"{int(want['trunc'].sum())}, paths near zero {near_zero}); mean variance off by {rv_err:.3e}")
        assert (err <= tol).all(), (k, got[k], want["y"][k], tol)
        assert near_floor.mean() <= cases.NEAR_CAP and near_cap.mean() <= cases.NEAR_CAP
        assert abs(res.n_floored - int(want["floored"].sum())) <= int(near_floor.sum())
        assert abs(res.n_capped - int(want["capped"].sum())) <= int(near_cap.sum())
        if job[3] == -INF:
            assert res.n_floored == 0
        if job[4] == INF:
            assert res.n_capped == 0
        if prec == capi.F64:
            assert res.truncated_steps == float(want["trunc"].sum())
        else:
            assert near_zero <= hc.NEAR_CAP * N_LOCAL
            assert abs(res.truncated_steps - float(want["trunc"].sum())) <= near_zero
        assert rv_err <= rv_tol, (rv_err, rv_tol)
        # the sums are those of the fp64 samples the kernel narrowed into d_samples: half an ulp of the path precision each
        half_ulp = 0.5 * float(np.finfo(cases.NP_T[prec]).eps) if prec == capi.F32 else 0.0
        slack = N_LOCAL * half_ulp * float(np.abs(got).max())
        assert abs(res.sum - got.sum()) <= slack + 1e-12 * float(np.abs(got).sum())
        assert abs(res.sumsq - (got * got).sum()) <= 2.0 * slack * float(np.abs(got).max()) + 1e-12 * float((got * got).sum())
        fin = capi.finalize(res.sum, res.sumsq, res.n, R, T_)
        assert (res.price, res.std_err, res.ci_lo, res.ci_hi) == (fin.price, fin.std_err, fin.ci_lo, fin.ci_hi)


# ---- 2. identities -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [cases.FIRST_SHAPE, (6, 3, 1, SHALLOW), (5, 1, 2, SHALLOW)], ids=cases.shape_name)
def test_constant_variance_gives_the_samples_of_the_surface_call(ctx, prec, shape):
    """xi = 0, kappa = 0, v0 = fl(0.2 * 0.2): mcamd_price_cliquet's samples on a flat 1 x 2 surface at 0.2, same ids"""
    n_steps, reset_every, first, where = shape
    v0 = float(np.float64(0.2) * np.float64(0.2))
    tol = cases.tolerance(prec, "F")
    hs = model("F", v0=v0, xi=0.0, kappa=0.0, theta=0.3)
    with ctx.localvol_surface((1, 2, -1.0, 1.0), [[0.2, 0.2]]) as flat:
        for job in cases.JOBS:
            cq = make(job, reset_every, first)
            res, got = run(ctx, shard(prec, n_steps, where), hs, cq)
            s = torch.full((N_LOCAL,), float("nan"), dtype=TORCH_T[prec], device="cuda")
            lv = ctx.price_cliquet(option(), shard(prec, n_steps, where), cq, flat, s)
            torch.cuda.synchronize()
            want = s.cpu().numpy().astype(np.float64)
            err = np.abs(got - want)
            print(f"fp{prec} {cases.shape_name(shape)} job {cases.job_name(job)}: worst deviation from mcamd_price_cliquet "
                  f"{err.max():.3e}, tolerance {tol:.3e}")
            assert (err <= tol).all()
            assert res.truncated_steps == 0 and abs(res.mean_variance - v0) <= hc.FLOOR[prec]["rv"]
            assert (res.n, res.grid, res.work_steps) == (lv.n, lv.grid, lv.work_steps)


@pytest.mark.parametrize("prec,name", [(p, n) for n, precs in cases.MODELS for p in precs])
@pytest.mark.parametrize("n_steps", [50, 3])
def test_one_unbounded_period_against_the_european_call(ctx, prec, name, n_steps):
    """S0 (y + 1) against mcamd_price_heston's S_T within DESIGN 23's floor for S_T; the two diagnostics are the
    European call's on the same job, mean_variance bit for bit in fp64"""
    sim = shard(prec, n_steps, SHALLOW)
    res, y = run(ctx, sim, model(name), capi.make_cliquet(SUM, n_steps, 1, q=Q))
    state = torch.full((2 * N_LOCAL,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    eu = ctx.price_heston(option(100.0), sim, model(name), None, state)
    torch.cuda.synchronize()
    S_T = state.cpu().numpy().astype(np.float64)[:N_LOCAL]
    err = np.abs(S0 * (y + 1.0) - S_T)
    floor = hc.FLOOR[prec]["S_T"]
    print(f"{name} fp{prec} {n_steps} steps: worst deviation of S0 (y + 1) from mcamd_price_heston's S_T {err.max():.3e}, "
          f"floor {floor:.1e}; truncated {res.truncated_steps:.0f} and {eu.truncated_steps:.0f}; mean variance "
          f"{res.mean_variance!r} and {eu.mean_variance!r}")
    assert (err <= floor).all()
    assert res.truncated_steps == eu.truncated_steps
    if prec == capi.F64:
        assert res.mean_variance == eu.mean_variance
    else:
        assert abs(res.mean_variance - eu.mean_variance) <= 1e-12 * eu.mean_variance
    assert (res.n, res.grid, res.work_steps) == (eu.n, eu.grid, eu.work_steps)


# ---- 3. plumbing -------------------------------------------------------------------------------------------------------------

def counted(r):
    return (r.sum, r.sumsq, r.n_floored, r.n_capped, r.truncated_steps, r.mean_variance, r.work_steps, r.n)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("job", [cases.JOBS[0], cases.JOBS[3], cases.JOBS[5]], ids=cases.job_name)
def test_three_shards_add_up_to_the_whole_job(ctx, prec, job):
    n, n_steps = 513, 12
    hs, cq = model("N"), make(job, 3, 2)
    whole, y = run(ctx, capi.make_sim(n, n_steps, prec, seed=3), hs, cq)
    parts = []
    for lo, hi in ((0, 100), (100, 101), (101, 513)):
        part, y_part = run(ctx, capi.make_sim(n, n_steps, prec, seed=3, path_offset=lo, n_paths_local=hi - lo), hs, cq)
        assert np.array_equal(y_part, y[lo:hi])
        parts.append(part)
    assert abs(sum(p.sum for p in parts) - whole.sum) <= 1e-13 * abs(whole.sum)
    assert abs(sum(p.sumsq for p in parts) - whole.sumsq) <= 1e-13 * whole.sumsq
    assert sum(p.n for p in parts) == whole.n == n and whole.grid == 3
    assert sum(p.n_floored for p in parts) == whole.n_floored and sum(p.n_capped for p in parts) == whole.n_capped
    assert sum(p.truncated_steps for p in parts) == whole.truncated_steps
    assert abs(sum(p.mean_variance * p.n for p in parts) - whole.mean_variance * n) <= 1e-13 * whole.mean_variance * n
    assert whole.n_floored + whole.n_capped > 0 and whole.sum > 0 and whole.truncated_steps > 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("job", [cases.JOBS[0], cases.JOBS[4], cases.JOBS[6]], ids=cases.job_name)
def test_same_bits_twice_and_the_enqueue_record(ctx, prec, job):
    n, n_steps = 3000, 13
    hs, cq = model("N"), make(job, 1, 2)
    sim = capi.make_sim(n + 9, n_steps, prec, seed=4, path_offset=9, n_paths_local=n)
    a, y_a = run(ctx, sim, hs, cq)
    b, y_b = run(ctx, sim, hs, cq)
    assert np.array_equal(y_a, y_b) and counted(a) == counted(b)
    assert a.grid == -(-n // 256) and a.sum > 0 and a.work_steps == full_work(n, n_steps)
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.full((n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    ctx.price_heston_cliquet_enqueue(option(), sim, hs, cq, stats, s)
    ms = ctx.enqueued_kernel_ms(1)
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    assert rec.tolist() == [a.sum, a.sumsq, float(a.n_floored), float(a.n_capped), rec[4], float(n)]
    assert rec[4] / n == a.mean_variance
    assert np.array_equal(s.cpu().numpy().astype(np.float64), y_a)
    fin = capi.finalize_stats(rec, R, T_)
    assert (fin.price, fin.std_err, fin.n) == (a.price, a.std_err, n)
    assert 0.0 < ms[0] < 1e4


def test_eight_calls_enqueued_back_to_back(ctx):
    n, n_steps = 1000, 12
    rows = [(prec, job, name) for prec in PRECS for job, name in ((cases.JOBS[0], "F"), (cases.JOBS[3], "N"),
                                                                  (cases.JOBS[5], "N"), (cases.JOBS[1], "H"))]
    stats = torch.full((len(rows), 6), float("nan"), dtype=torch.float64, device="cuda")
    for row, (prec, job, name) in enumerate(rows):
        ctx.price_heston_cliquet_enqueue(option(), capi.make_sim(n, n_steps, prec, seed=5 + row), model(name),
                                         make(job, 4, 1 + row % 3), stats[row])
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    for row, (prec, job, name) in enumerate(rows):
        res, _ = run(ctx, capi.make_sim(n, n_steps, prec, seed=5 + row), model(name), make(job, 4, 1 + row % 3), False)
        assert rec[row].tolist() == [res.sum, res.sumsq, float(res.n_floored), float(res.n_capped), rec[row][4], float(n)]
        assert rec[row][4] / n == res.mean_variance and res.sumsq > 0


def test_an_empty_shard_launches_nothing(ctx):
    hs, cq = model("F"), make(cases.JOBS[0], 4)
    sim = capi.make_sim(1000, 12, path_offset=10, n_paths_local=0)
    res, _ = run(ctx, sim, hs, cq, False)
    assert all(v == 0 for v in res.as_dict().values())
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    ctx.price_heston_cliquet_enqueue(option(), sim, hs, cq, stats)
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()


def test_refusals_with_a_live_context(ctx):
    """what the CPU tests see refused without a context is refused with one, by both forms, and nothing is launched:
    the statistics stay as they were"""
    sim = capi.make_sim(1000, 12)
    stats = torch.full((6,), -1.0, dtype=torch.float64, device="cuda")
    bad_reserved = make(cases.JOBS[0], 4)
    bad_reserved.reserved = 1
    bad = [(model("F"), make((3, -INF, INF, -INF, INF), 4), sim, "kind"),
           (model("F"), bad_reserved, sim, "reserved"),
           (model("F"), make(cases.JOBS[0], 5), sim, "reset_every"),
           (model("F"), make(cases.JOBS[0], 4, 4), sim, "first_period"),
           (model("F"), make((SUM, 0.05, 0.05, -INF, INF), 4), sim, "local_floor"),
           (model("F"), make((SUM, -0.03, 0.05, 0.2, 0.1), 4), sim, "global_floor"),
           (model("F"), make((COMPOUND, -1.5, 0.05, -INF, INF), 4), sim, "compounding"),
           (model("F"), make((COMPOUND, -INF, -1.0, -INF, INF), 4), sim, "compounding"),
           (model("F"), make((VARIANCE, 0.0, INF, -INF, INF), 4), sim, "realized variance"),
           (model("F"), make(cases.JOBS[0], 4), capi.make_sim(1000, 12, flags=capi.FLAG_ANTITHETIC), "flags"),
           (model("F"), make(cases.JOBS[0], 4), capi.make_sim(1000, 12, precision=16), "precision"),
           (model("F", xi=-0.1), make(cases.JOBS[0], 4), sim, ">= 0"),
           (model("F", rho=1.5), make(cases.JOBS[0], 4), sim, "rho"),
           (capi.make_heston(2), make(cases.JOBS[0], 4, q=0.0), sim, "payoff"),
           (capi.make_heston(0, scheme=1), make(cases.JOBS[0], 4, q=0.0), sim, "scheme"),
           (model("F"), make(cases.JOBS[0], 4, q=0.02), sim, "same dividend yield"),
           (model("F", q=0.0), make(cases.JOBS[0], 4, q=-0.0), sim, "same dividend yield")]
    for hs, cq, s, words in bad:
        for call in (lambda: ctx.price_heston_cliquet(option(), s, hs, cq),
                     lambda: ctx.price_heston_cliquet_enqueue(option(), s, hs, cq, stats)):
            with pytest.raises(capi.McamdError) as e:
                call()
            assert e.value.code == capi.ERR_INVALID and words in str(e.value), (words, str(e.value))
    with pytest.raises(capi.McamdError) as e:
        ctx.price_heston_cliquet_enqueue(option(), sim, model("F"), make(cases.JOBS[0], 4), None)
    assert "d_stats is NULL" in str(e.value)
    torch.cuda.synchronize()
    assert (stats.cpu().numpy() == -1.0).all()
    ok, _ = run(ctx, sim, model("F"), make(cases.JOBS[0], 4), False)   # and the context still serves
    assert ok.n == 1000 and ok.sumsq > 0


# ---- 4. against the closed form ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tag,kind,M,floor,cap", [("cliquet", SUM, 4, 0.0, 0.08), ("variance swap", VARIANCE, 4, -INF, INF)])
def test_statistical_run_against_the_closed_form(ctx, prec, tag, kind, M, floor, cap):
    """F, 2^18 paths x 128 steps: DESIGN 23 measured F's discretisation bias at this step count as below that noise"""
    n, n_steps = 1 << 18, 128
    q, v0, kappa, theta, xi, rho = hr.params("F")
    sim = capi.make_sim(n, n_steps, prec, seed=2042 + kind)
    res, _ = run(ctx, sim, model("F"), capi.make_cliquet(kind, n_steps // M, 1, floor, cap, q=Q), False)
    want = capi.heston_cliquet_price(kind, T_, R, q, v0, kappa, theta, xi, rho, M, 1, floor, cap)
    print(f"{tag} fp{prec}: closed {want:.6f} price {res.price:.6f} SE {res.std_err:.6f} "
          f"({(res.price - want) / res.std_err:+.2f} SE), truncated {res.truncated_steps / (n * n_steps):.5f} of the steps, "
          f"mean variance {res.mean_variance:.5f}, kernel {res.kernel_ms:.3f} ms")
    assert res.std_err > 0 and abs(res.price - want) <= 4.0 * res.std_err
    assert res.work_steps == full_work(n, n_steps) and res.n_floored == res.n_capped == 0
    assert abs(res.mean_variance - theta) <= 1e-3
