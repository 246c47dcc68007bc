"""GPU tests of the cliquet pricer (mcamd_price_cliquet).  Run with -m gpu on an MI355X.

  1. samples, elementwise through d_samples, against the numpy restatement (tests/cliquet_restate.py) on normals drawn
     from the oracle's rocRAND-exact generator for (seed, global path id, block): 4096 paths at global ids 5003.. under
     seed 77 and the deep inputs of tests/deep_inputs.py, on the surface SKEW of tests/test_gpu_localvol.py (4 x 65 on
     [-1.5, 1.5], r = 0.1, q = 0.03); both precisions x three kinds x the bounds below x (n_steps, reset_every,
     first_period) = (48, 4, 1); (50, 5, 3) on the 3-slice surface; (6, 3, 1): a reset inside an fp32 Philox block;
     (5, 1, 2): a reset at every step and a remainder block; (7, 7, 1) on the deep inputs: one period, path ids beyond 32
     bits; (3, 1, 3): only the last period counts.  The counters against the restated flags;
  2. no kernel: the restatement's own spread, the near-bound share and the clipped share on every input of test 1, and
     the deep normals against both shallow words;
  3. SUM with one period and a floor alone against mcamd_price_localvol's call sample on the same job and surface;
  4. closed forms (mcamd_cliquet_price_f64) within 4 SE on time-only and flat surfaces;
  5. shards, repeatability, the enqueue form, an empty shard, a surface of another context.

Tolerance of 1 and 3 (elementwise_tolerance; from the restatement alone, computed on the CPU): four times the largest
elementwise difference between the float64 and longdouble restatements (fp64 kernels), or between the float32 and
float64 restatements (fp32 kernels), over all 8 jobs on the (48, 4, 1) inputs, floored at the floors of
tests/test_gpu_localvol.py per unit of notional (those tests use a spot of 100): 1e-13 absolute (fp64), 2e-5 absolute
(fp32).  Measured with the Philox normals on an x86-64 CPU (80-bit longdouble): 9.7e-16 for fp64 and 6.0e-7 for fp32, so
the floors decide; on the other inputs the restatements differ by 3.1e-16 .. 9.4e-16 and 2.7e-7 .. 4.3e-7.  The kernels
themselves, on an MI355X: at most 1.8e-15 (fp64) and 4.8e-7 (fp32) from the restatement over all 96 cases of test 1, and in
test 3 at most 5.7e-14 and 6.7e-6 per 100 of spot from mcamd_price_localvol's sample.  No path is left out of the sample comparison: every operation between X and y (min, max, the clamp
of the lookup) is continuous.  n_floored and n_capped may differ from the restated counts by at most the number of paths
whose restated A lies within MARGIN = 2e-5 of that bound, at most 1 % of a case."""
import importlib
import math

import numpy as np
import pytest

import cliquet_restate as cr
from deep_inputs import DEEP, SHALLOW, check_deep_draws_differ

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

NP_T = {capi.F64: np.float64, capi.F32: np.float32}
WIDER = {capi.F64: np.longdouble, capi.F32: np.float64}
FLOOR = {capi.F64: 1e-13, capi.F32: 2e-5}
SUM_RTOL = {capi.F64: 1e-11, capi.F32: 2e-5}
MARGIN = 2e-5
CAP = 0.01
R, Q_DIV, T_, S0 = 0.1, 0.03, 1.0, 100.0
N_LOCAL = 4096
INF = float("inf")
PRECS = (capi.F64, capi.F32)


def skew(n_t, n_x, x_min, x_max, lo=0.18, step=0.04):
    x = np.linspace(x_min, x_max, n_x)
    return (n_t, n_x, x_min, x_max), np.array([(lo + step * j) * (1.0 + 0.5 * np.exp(-x)) / 1.5 for j in range(n_t)])


def time_only(vols):
    return (len(vols), 2, -1.0, 1.0), np.array([[v, v] for v in vols])


SURFACES = {
    "skew": skew(4, 65, -1.5, 1.5),
    "skew3": skew(3, 65, -1.5, 1.5),   # n_t does not divide 50 steps
    "flat": time_only((0.2,)),
    "slices3": time_only((0.15, 0.30, 0.20)),
    "slices2": time_only((0.15, 0.30)),
}

# (n_steps, reset_every, first_period, where, surface); the first is what the tolerance is taken from
FIRST_INPUT = (48, 4, 1, SHALLOW, "skew")
INPUTS = (FIRST_INPUT, (50, 5, 3, SHALLOW, "skew3"), (6, 3, 1, SHALLOW, "skew"), (5, 1, 2, SHALLOW, "skew"),
          (7, 7, 1, DEEP, "skew"), (3, 1, 3, SHALLOW, "skew"))
# (local_floor, local_cap, global_floor, global_cap)
BOUNDS = ((-0.03, 0.05, 0.0, 0.25), (0.0, 0.04, -INF, INF), (-1.0, INF, 0.0, INF))
JOBS = [(kind, *b) for kind in (cr.SUM, cr.COMPOUND) for b in BOUNDS] + \
       [(cr.VARIANCE, -INF, INF, -INF, INF), (cr.VARIANCE, -INF, INF, -INF, 0.06)]


def option():
    # v, K and B are ignored by the call: leave something in them that any use would show
    return capi.make_option(S0=S0, K=float("nan"), r=R, T=T_, v=float("nan"), B=float("nan"))


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


def restate(prec, job, inp, dtype):
    """one restatement per (case, dtype), shared by every test that needs it and left unchanged"""
    key = (prec, job, inp, np.dtype(dtype).name)
    if key not in _restated:
        n_steps, reset_every, first, where, surface = inp
        grid, sigma = SURFACES[surface]
        z = normals(prec, where[0], where[1], N_LOCAL, n_steps)
        _restated[key] = cr.samples(z, T_, R, Q_DIV, grid, sigma, job[0], reset_every, first, *job[1:], dtype=dtype)
    return _restated[key]


def compare(prec, job, inp):
    """(restated samples to compare with, restatement in the kernel's precision, largest difference between the two
    restatements the tolerance is taken from) — CPU only"""
    own, other = restate(prec, job, inp, NP_T[prec]), restate(prec, job, inp, WIDER[prec])
    spread = float(np.abs(own["y"] - other["y"]).max())
    # an fp64 kernel is compared with the float64 restatement, an fp32 kernel with the float64 one too
    want = own if prec == capi.F64 else other
    return want, own, spread


_spread = {}


def measured_spread(prec):
    """the largest restatement difference over all jobs on the (48, 4, 1) inputs"""
    if prec not in _spread:
        _spread[prec] = max(compare(prec, job, FIRST_INPUT)[2] for job in JOBS)
    return _spread[prec]


def elementwise_tolerance(prec):
    """Absolute tolerance per element, per unit of notional: 4 x the largest restatement difference over the jobs of the
    (48, 4, 1) inputs, floored at 1e-13 (fp64) / 2e-5 (fp32).  From the restatement alone."""
    return max(4.0 * measured_spread(prec), FLOOR[prec])


def near(want, job):
    """per path: the restated A lies within MARGIN of the global floor / of the global cap"""
    A = np.asarray(want["A"], dtype=np.float64)
    return np.abs(A - job[3]) <= MARGIN, np.abs(A - job[4]) <= MARGIN


def _job_name(job):
    return "-".join(str(x) for x in job)


def _inp_name(inp):
    return f"{inp[0]}-{inp[1]}-{inp[2]}" + ("-deep" if inp[3] == DEEP else "")


SAMPLE_CASES = [pytest.param(prec, job, inp, id=f"{prec}-{_job_name(job)}-{_inp_name(inp)}")
                for inp in INPUTS for prec in PRECS for job in JOBS]


# ---- 2. no kernel ----------------------------------------------------------------------------------------------------

def test_restatement_stays_under_the_spread_and_the_cap():
    """no kernel runs: on every input of test 1 the two restatements differ by at most twice the spread the tolerance is
    taken from; at most 1 % of a case lies within MARGIN of a global bound; every case with a global bound has more than
    2 % of its paths on a bound and more than 2 % off it"""
    for prec in PRECS:
        print(f"prec {prec}: restatement spread on the (48, 4, 1) inputs {measured_spread(prec):.3e}, tolerance "
              f"{elementwise_tolerance(prec):.3e}")
    for inp in INPUTS:
        for prec in PRECS:
            worst, near_share, lo_share, hi_share = 0.0, 0.0, 1.0, 0.0
            for job in JOBS:
                want, own, spread = compare(prec, job, inp)
                worst = max(worst, spread)
                assert np.isfinite(np.asarray(want["y"], dtype=np.float64)).all()
                assert spread <= 2.0 * measured_spread(prec), (inp, prec, job, spread)
                for flags in near(want, job):
                    near_share = max(near_share, flags.mean())
                    assert flags.mean() <= CAP, (inp, prec, job, flags.mean())
                if job[3] > -INF or job[4] < INF:
                    on = (want["floored"] | want["capped"]).mean()
                    lo_share, hi_share = min(lo_share, on), max(hi_share, on)
                    assert 0.02 < on < 0.98, (inp, prec, job, on)
                    assert np.array_equal(own["floored"] | own["capped"], np.asarray(own["y"] != own["A"]) |
                                          (own["A"] == job[3]) | (own["A"] == job[4]))
                else:
                    assert not want["floored"].any() and not want["capped"].any()
            print(f"{_inp_name(inp)} prec {prec}: largest restatement difference {worst:.3e}, largest near-bound share "
                  f"{near_share:.4f}, share on a global bound {lo_share:.3f}..{hi_share:.3f}")


def test_bound_shares_on_the_first_input():
    """no kernel runs: on the Philox normals of the (48, 4, 1) inputs the bounded SUM and COMPOUND jobs put 22-42 % of
    the paths on a global bound and the doubly bounded ones 8-10 % on the cap, the shares measured on numpy normals; the
    ranges asserted are those, widened by three standard deviations of a 4096-path share (0.02 at most, rounded up)"""
    for prec in PRECS:
        for job in JOBS:
            if job[0] == cr.VARIANCE or (job[3] == -INF and job[4] == INF):
                continue
            want, _, _ = compare(prec, job, FIRST_INPUT)
            on, capped = (want["floored"] | want["capped"]).mean(), want["capped"].mean()
            print(f"prec {prec} job {_job_name(job)}: on a global bound {on:.3f}, on the cap {capped:.3f}")
            assert 0.20 <= on <= 0.45, (prec, job, on)
            if job[4] < INF:
                assert 0.06 <= capped <= 0.12, (prec, job, capped)


@pytest.mark.parametrize("prec", PRECS)
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


def make(job, reset_every, first_period=1, q=Q_DIV):
    return capi.make_cliquet(job[0], reset_every, first_period, *job[1:], q)


def run(ctx, sim, cliquet, surface, want_samples=True):
    """(result, samples as float64 numpy or None)"""
    s = None
    if want_samples:
        s = torch.full((max(sim.n_paths_local, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    res = ctx.price_cliquet(option(), sim, cliquet, surface, s)
    torch.cuda.synchronize()
    return res, (s[:sim.n_paths_local].cpu().numpy().astype(np.float64) if want_samples else None)


def full_work(n, n_steps):
    return 64 * -(-n // 64) * n_steps


# ---- 1. samples against the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec,job,inp", SAMPLE_CASES)
def test_samples_against_the_restatement(ctx, surfaces, prec, job, inp):
    n_steps, reset_every, first, where, surface = inp
    seed, first_path, n_job = where
    want, own, spread = compare(prec, job, inp)
    tol = elementwise_tolerance(prec)
    sim = capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first_path, n_paths_local=N_LOCAL)
    res, got = run(ctx, sim, make(job, reset_every, first), surfaces[surface])
    assert np.isfinite(got).all() and res.n == N_LOCAL and res.block == 256 and res.grid == N_LOCAL // 256
    err = np.abs(got - np.asarray(want["y"], dtype=np.float64))
    k = int(np.argmax(err))
    near_floor, near_cap = near(want, job)
    print(f"{surface} prec {prec} job {_job_name(job)} input {_inp_name(inp)}: restatement spread {spread:.3e}, tolerance "
          f"{tol:.3e}, worst deviation {err.max():.3e}, floored {res.n_floored} (restated {int(want['floored'].sum())}, near "
          f"{int(near_floor.sum())}), capped {res.n_capped} (restated {int(want['capped'].sum())}, near {int(near_cap.sum())})")
    assert (err <= tol).all(), (k, got[k], want["y"][k], tol)
    assert near_floor.mean() <= CAP and near_cap.mean() <= CAP
    assert abs(res.n_floored - int(want["floored"].sum())) <= int(near_floor.sum())
    assert abs(res.n_capped - int(want["capped"].sum())) <= int(near_cap.sum())
    if job[3] == -INF:
        assert res.n_floored == 0
    if job[4] == INF:
        assert res.n_capped == 0
    # the sums are those of the fp64 samples the kernel narrowed into d_samples: half an ulp of the path precision each
    half_ulp = 0.5 * float(np.finfo(NP_T[prec]).eps) if prec == capi.F32 else 0.0
    slack = N_LOCAL * half_ulp * float(np.abs(got).max())
    assert abs(res.sum - got.sum()) <= slack + 1e-12 * float(np.abs(got).sum())
    assert abs(res.sumsq - (got * got).sum()) <= 2.0 * slack * float(np.abs(got).max()) + 1e-12 * float((got * got).sum())
    fin = capi.finalize(res.sum, res.sumsq, res.n, R, T_)
    assert (res.price, res.std_err, res.ci_lo, res.ci_hi) == (fin.price, fin.std_err, fin.ci_lo, fin.ci_hi)
    assert res.work_steps == full_work(N_LOCAL, n_steps)


# ---- 3. one period with a floor alone is the European call ------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("k", [0.9, 1.0, 1.1])
def test_single_period_sum_against_the_localvol_call_sample(ctx, surfaces, prec, k):
    """S0 (y - (k - 1)) = (S_T - k S0)+ of mcamd_price_localvol on the same job and surface"""
    n_steps = FIRST_INPUT[0]
    seed, first_path, n_job = SHALLOW
    sim = capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first_path, n_paths_local=N_LOCAL)
    res, y = run(ctx, sim, capi.make_cliquet(cr.SUM, n_steps, 1, local_floor=k - 1.0, q=Q_DIV), surfaces["skew"])
    s = torch.full((N_LOCAL,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    opt = capi.make_option(S0=S0, K=k * S0, r=R, T=T_, v=float("nan"))
    call = ctx.price_localvol(opt, sim, capi.make_localvol(capi.PAYOFF_CALL, q=Q_DIV), surfaces["skew"], s)
    torch.cuda.synchronize()
    want = s.cpu().numpy().astype(np.float64)
    got = S0 * (y - (k - 1.0))
    tol = S0 * elementwise_tolerance(prec)
    err = np.abs(got - want)
    print(f"prec {prec} k {k}: worst deviation from mcamd_price_localvol {err.max():.3e}, tolerance {tol:.3e}, "
          f"non-zero call samples {(want != 0).mean():.3f}")
    assert (err <= tol).all() and 0.02 < (want != 0).mean() < 0.98
    assert res.work_steps == call.work_steps == full_work(N_LOCAL, n_steps)
    assert res.n_floored == res.n_capped == 0 and (res.n, res.grid) == (call.n, call.grid)


# ---- 4. closed forms ---------------------------------------------------------------------------------------------------

def within_4_se(tag, res, want):
    print(f"{tag}: closed {want:.6f} price {res.price:.6f} SE {res.std_err:.6f} ({(res.price - want) / res.std_err:+.2f} SE) "
          f"kernel {res.kernel_ms:.3f} ms")
    assert res.std_err > 0 and abs(res.price - want) <= 4.0 * res.std_err, (tag, res.price, want, res.std_err)


LOCAL = {cr.SUM: (-0.03, 0.05), cr.COMPOUND: (-0.03, 0.05), cr.VARIANCE: (-INF, INF)}
RMS2 = math.sqrt((0.15 ** 2 + 0.30 ** 2) / 2)
# (surface, n_steps, reset_every, first_period, period volatilities, kinds)
CLOSED = [("slices3", 12, 4, 1, (0.15, 0.30, 0.20), cr.KINDS), ("slices3", 12, 4, 3, (0.15, 0.30, 0.20), cr.KINDS),
          ("slices2", 4, 4, 1, (RMS2,), cr.KINDS),   # one period spans two slices: the rms volatility
          ("flat", 252, 21, 1, (0.2,) * 12, (cr.SUM, cr.VARIANCE))]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("surface,n_steps,reset_every,first,vols,kinds", CLOSED,
                         ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" for c in CLOSED])
def test_closed_forms_within_4_se(ctx, surfaces, prec, surface, n_steps, reset_every, first, vols, kinds):
    for kind in kinds:
        sim = capi.make_sim(1 << 20, n_steps, prec, seed=2040 + n_steps + kind)
        res, _ = run(ctx, sim, capi.make_cliquet(kind, reset_every, first, *LOCAL[kind], q=Q_DIV), surfaces[surface], False)
        want = capi.cliquet_price(kind, T_, R, Q_DIV, vols, first, *LOCAL[kind])
        within_4_se(f"{surface} ({n_steps}, {reset_every}, {first}) kind {kind} prec {prec}", res, want)
        assert res.work_steps == full_work(1 << 20, n_steps) and res.n_floored == res.n_capped == 0


# ---- 5. plumbing ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("job", [JOBS[0], JOBS[3], JOBS[7]], ids=_job_name)
def test_two_shards_add_up_to_the_whole_job(ctx, surfaces, prec, job):
    n, n_steps, cut = 10_001, 12, 4097
    cq = make(job, 3, 2)
    whole, y = run(ctx, capi.make_sim(n, n_steps, prec, seed=3), cq, surfaces["skew"])
    parts = []
    for lo, hi in ((0, cut), (cut, n)):
        part, y_part = run(ctx, capi.make_sim(n, n_steps, prec, seed=3, path_offset=lo, n_paths_local=hi - lo), cq,
                           surfaces["skew"])
        assert np.array_equal(y_part, y[lo:hi])
        parts.append(part)
    rt = SUM_RTOL[prec]
    assert abs(parts[0].sum + parts[1].sum - whole.sum) <= rt * abs(whole.sum)
    assert abs(parts[0].sumsq + parts[1].sumsq - whole.sumsq) <= rt * whole.sumsq
    assert parts[0].n + parts[1].n == whole.n == n
    assert parts[0].n_floored + parts[1].n_floored == whole.n_floored
    assert parts[0].n_capped + parts[1].n_capped == whole.n_capped
    assert whole.n_floored + whole.n_capped > 0 and whole.sum > 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [3000, 3_000_000])   # one wave of workgroups; beyond the 8192-workgroup cap (grid-stride)
@pytest.mark.parametrize("job", [JOBS[0], JOBS[5], JOBS[7]], ids=_job_name)
def test_same_bits_twice_and_from_the_enqueue_form(ctx, surfaces, prec, n, job):
    n_steps = 13
    cq = make(job, 1, 2)
    sim = capi.make_sim(n + 9, n_steps, prec, seed=4, path_offset=9, n_paths_local=n)
    a, y_a = run(ctx, sim, cq, surfaces["skew"])
    b, y_b = run(ctx, sim, cq, surfaces["skew"])
    counted = lambda r: (r.sum, r.sumsq, r.n_floored, r.n_capped, r.work_steps, r.n)
    assert np.array_equal(y_a, y_b) and counted(a) == counted(b)
    assert a.grid == min(-(-n // 256), 8192) and a.sum > 0 and a.work_steps == full_work(n, n_steps)
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.full((n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    ctx.price_cliquet_enqueue(option(), sim, cq, surfaces["skew"], stats, s)
    ms = ctx.enqueued_kernel_ms(1)
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    assert rec.tolist() == [a.sum, a.sumsq, float(a.n_floored), float(a.n_capped), 0.0, float(n)]
    assert np.array_equal(s.cpu().numpy().astype(np.float64), y_a)
    fin = capi.finalize_stats(rec, R, T_)
    assert (fin.price, fin.std_err, fin.n) == (a.price, a.std_err, n)
    assert 0.0 < ms[0] < 1e4


def test_an_empty_shard_launches_nothing(ctx, surfaces):
    cq = make(JOBS[0], 4)
    sim = capi.make_sim(1000, 12, path_offset=10, n_paths_local=0)
    res, _ = run(ctx, sim, cq, surfaces["skew"], False)
    assert all(v == 0 for v in res.as_dict().values())
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    ctx.price_cliquet_enqueue(option(), sim, cq, surfaces["skew"], stats)
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()


def test_a_surface_of_another_context_is_refused(ctx, surfaces):
    cq, sim = make(JOBS[0], 4), capi.make_sim(1000, 12)
    ok, _ = run(ctx, sim, cq, surfaces["skew"], False)
    stats = torch.zeros(6, dtype=torch.float64, device="cuda")
    other = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        with other.localvol_surface(*SURFACES["skew"]) as foreign:
            for call in (lambda: ctx.price_cliquet(option(), sim, cq, foreign),
                         lambda: ctx.price_cliquet_enqueue(option(), sim, cq, foreign, stats)):
                with pytest.raises(capi.McamdError) as e:
                    call()
                assert e.value.code == capi.ERR_INVALID and "another context" in str(e.value)
            mine = other.price_cliquet(option(), sim, cq, foreign)
            assert (mine.sum, mine.sumsq, mine.n_floored, mine.n_capped) == (ok.sum, ok.sumsq, ok.n_floored, ok.n_capped)
    finally:
        other.close()
    # the fp64 exponent-range bound is taken at the surface's largest entry, once the request itself has passed
    with ctx.localvol_surface((1, 2, -1.0, 1.0), [[0.2, 100.0]]) as wild:
        with pytest.raises(capi.McamdError) as e:
            ctx.price_cliquet(capi.make_option(S0=S0, r=R, T=100.0, v=0.0), capi.make_sim(1000, 50), make(JOBS[0], 5), wild)
        assert e.value.code == capi.ERR_INVALID and "exponent range" in str(e.value)
