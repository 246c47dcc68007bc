"""GPU tests of the smile pricer (mcamd_price_localvol_smile).  Run with -m gpu on an MI355X.

  1. spots, elementwise through d_spots, against the numpy restatement (tests/localvol_smile_restate.py) on normals drawn
     from the oracle's rocRAND-exact generator for (seed, global path id, block), on the ids, seeds and surfaces of
     tests/test_gpu_localvol.py (q = 0.03): 4096 paths at the shallow ids, 50 steps, expiries (1, 2, 3, 4, 5, 25, 26, 49,
     50) — an expiry on every position of a Philox block in both precisions, consecutive expiries, the first and the last
     step —; 7 steps on the deep ids with expiries (3, 6), the last one below n_steps and inside the remainder block;
     5 steps on skew7, where rows are skipped; 50 steps on skew3 and narrow;
  2. the strike phase alone: node sums against sums formed in numpy from the returned d_spots (h in the path precision,
     summed in float64), (n_e, n_K) in {(1, 1), (1, 2), (3, 63), (2, 64), (32, 64)}, calls and puts, strikes from deep in
     to deep out of the money, n_paths_local in {1, 2, 63, 64, 65, 255, 257, 4097}, and one job of
     3 grid 256 + 77 paths at (32, 64) whose wavefronts make several trips; every job is run a second time after another
     pricer and another smile have left their numbers in the context's scratch buffer, and must not move;
  3. against the pricer it extends: at the last step every strike's sums are mcamd_price_localvol's; on the flat surface an
     inner expiry s is the call with T s / n and n_steps = s;
  4. closed forms within 4 SE at every node: a surface that varies in time only against Black-Scholes at the rms
     volatility up to each expiry, and the flat surface, whose implied volatilities lie within 4 SE / vega of 0.2;
  5. shards, repeatability, the enqueue form, two surfaces with eight enqueued calls, a foreign surface, an empty shard;
  6. four mistakes restated in numpy only (no mutated kernel is run), each refused by one of the cases above.

Tolerance of 1 (spot_tolerance; from the restatement alone, computed on the CPU): four times the largest elementwise
difference between the float64 and longdouble restatements (fp64 kernels), or between the float32 and float64
restatements (fp32 kernels), over all cases of test 1, floored at 1e-11 of the spot (fp64) and 2e-3 absolute (fp32).
Measured with the Philox normals on an x86-64 CPU (80-bit longdouble): 4 x 9.29e-14 = 3.7e-13 absolute for fp64, where
the floor of 1e-11 S (some 1e-9) decides, and 4 x 4.34e-5 = 1.7e-4 for fp32, where the 2e-3 floor decides.  Nothing is left
out: S is continuous in every input.  Tolerance of 2, 3 and 5: 1e-11 (fp64) / 2e-5 (fp32) of the node's sum, exactly 0
where no path pays; the flat inner expiries of 3 take 1e-9 in fp64 because dt differs in the last bit.

Measured on an MI355X: largest deviation of the kernels' spots from the restatement 1.14e-13 (fp64) and 5.03e-5 (fp32);
node sums within 4.5e-15 relative of the numpy sums (fp64), equal to them in fp32; closed forms within 2.6 SE.

The seeds of 4 were checked on the CPU with the restatement (every node inside 4 SE at 2^14 paths) before they were
fixed."""
import importlib
import itertools
import math

import numpy as np
import pytest

import localvol_smile_restate as sm
from deep_inputs import DEEP, DEEP_SEED, OFFSET, SHALLOW, check_deep_draws_differ
from smile_cases import SUM_RTOL, check_result_fields, check_sums_from_spots, strikes_for

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

NP_T = {capi.F64: np.float64, capi.F32: np.float32}
WIDER = {capi.F64: np.longdouble, capi.F32: np.float64}
FLAT_INNER_RTOL = {capi.F64: 1e-9, capi.F32: 2e-5}
BASE = dict(S0=100.0, r=0.1, T=1.0)
Q_DIV = 0.03
N_LOCAL = 4096
PRECS = [capi.F64, capi.F32]
PAYOFFS = [capi.PAYOFF_CALL, capi.PAYOFF_PUT]


def skew(n_t, n_x, x_min, x_max, lo=0.18, step=0.04):
    x = np.linspace(x_min, x_max, n_x)
    return (n_t, n_x, x_min, x_max), np.array([(lo + step * j) * (1.0 + 0.5 * np.exp(-x)) / 1.5 for j in range(n_t)])


TIME_ONLY_VOLS = (0.15, 0.30, 0.20, 0.25)
SURFACES = {
    "skew": skew(4, 65, -1.5, 1.5),
    "skew3": skew(3, 65, -1.5, 1.5),          # n_t does not divide 50 steps
    "skew7": skew(7, 65, -1.5, 1.5, 0.16, 0.03),   # more slices than the 5 steps: rows 3 and 6 are skipped
    "narrow": skew(4, 65, -0.05, 0.05),       # most paths run clamped, on either side
    "flat": ((1, 2, -1.0, 1.0), np.array([[0.2, 0.2]])),
    "time": ((4, 2, -1.0, 1.0), np.array([[v, v] for v in TIME_ONLY_VOLS])),
}

EVERY_SLOT = (1, 2, 3, 4, 5, 25, 26, 49, 50)
# (surface, where, n_steps, expiry steps)
SPOT_CASES = [("skew", SHALLOW, 50, EVERY_SLOT), ("skew", DEEP, 7, (3, 6)), ("skew7", SHALLOW, 5, (1, 3, 5)),
              ("skew3", SHALLOW, 50, EVERY_SLOT), ("narrow", SHALLOW, 50, EVERY_SLOT)]


def option():
    # v and K are ignored by the call: leave something in them that any use would show
    return capi.make_option(**dict(BASE, v=float("nan"), K=float("nan")))


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


def restate(prec, surface, where, n_steps, steps, dtype, n=N_LOCAL, mutate=None, first=None):
    """one restatement per (case, dtype), shared by every test that needs it and left unchanged"""
    key = (prec, surface, where, n_steps, tuple(steps), np.dtype(dtype).name, n, mutate, first)
    if key not in _restated:
        grid, sigma = SURFACES[surface]
        z = normals(prec, where[0], where[1] if first is None else first, n, n_steps)
        _restated[key] = sm.spots(z, BASE["S0"], BASE["T"], BASE["r"], Q_DIV, grid, sigma, n_steps, steps, dtype, mutate)
    return _restated[key]


_spread = {}


def measured_spread(prec):
    """the largest elementwise difference between the two restatements over the cases of test 1"""
    if prec not in _spread:
        _spread[prec] = max(float(np.abs(restate(prec, *case, NP_T[prec]).astype(np.longdouble) -
                                         restate(prec, *case, WIDER[prec]).astype(np.longdouble)).max())
                            for case in SPOT_CASES)
    return _spread[prec]


def spot_tolerance(prec, want):
    if prec == capi.F64:
        return np.maximum(4.0 * measured_spread(prec), 1e-11 * np.abs(want))
    return np.full(want.shape, max(4.0 * measured_spread(prec), 2e-3))


def wanted_spots(prec, case):
    """what a kernel of this precision is compared with: the float64 restatement"""
    return restate(prec, *case, np.float64).astype(np.float64)


def test_restatement_spread():
    """no kernel runs: what the tolerance of test 1 is made of"""
    for prec in PRECS:
        print(f"prec {prec}: largest restatement difference over the cases of test 1 {measured_spread(prec):.3e}")
    assert measured_spread(capi.F64) < 1e-11 and measured_spread(capi.F32) < 5e-4


@pytest.mark.parametrize("prec", PRECS)
def test_deep_normals_are_those_of_neither_shallow_word(prec):
    """no kernel runs: the deep normals share nothing with the streams a dropped high word lands on"""
    check_deep_draws_differ(lambda seed, first: normals(prec, seed, first, 64, 7))


# ---- 6. mistakes, restated in numpy only -----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_mistakes_restated_in_numpy_are_beyond_the_tolerances(prec):
    """no kernel runs.  Each mistake moves the restated result of a case of tests 1 and 2 by more than that case's
    tolerance, so the test named here refuses a kernel that makes it."""
    # an expiry taken one step late: test 1, on nearly every path of the 50-step case
    case = SPOT_CASES[0]
    want = wanted_spots(prec, case)
    late = restate(prec, *case, np.float64, mutate=sm.LATE_EXPIRY).astype(np.float64)
    assert (np.abs(late - want)[:-1] > spot_tolerance(prec, want)[:-1]).mean() > 0.99
    # a dropped high word of the path id: test 1 on the deep ids draws the normals of path 5003 + p instead
    case = SPOT_CASES[1]
    want = wanted_spots(prec, case)
    dropped = restate(prec, case[0], (DEEP_SEED, OFFSET, 0), *case[2:], np.float64).astype(np.float64)
    assert (np.abs(dropped - want) > spot_tolerance(prec, want)).mean() > 0.99
    # the strike loop over all 64 lanes with a partial prefix: test 2 at 65 paths (the second wavefront holds one)
    S = restate(prec, "skew", SHALLOW, 40, (40,), NP_T[prec], n=65)
    for payoff in PAYOFFS:
        K = strikes_for(64)
        right, wrong = sm.node_sums(S, K, payoff), sm.node_sums(S, K, payoff, mutate=sm.ALL_LANES)
        pays = right[0] > 0
        assert pays.any() and (np.abs(wrong[0] - right[0])[pays] > SUM_RTOL[prec] * right[0][pays]).all()
        # a first trip that adds instead of writes: test 2's second run finds the other smile's sums in the buffer
        stale = sm.node_sums(S, [0.5 * k for k in K], payoff)[0]
        wrong = sm.node_sums(S, K, payoff, mutate=sm.FIRST_TRIP_ADDS, stale=stale)
        assert (stale > 0).any() and (np.abs(wrong[0] - right[0])[stale > 0] > SUM_RTOL[prec] * right[0][stale > 0]).all()


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


def run(ctx, sim, payoff, steps, strikes, surface, want_spots=True, opt=None):
    """(price, std_err, stats, res, spots [n_e, n_local] in the path precision or None)"""
    smile = capi.make_smile(len(steps), len(strikes), payoff, Q_DIV)
    s = None
    if want_spots:
        s = torch.full((len(steps) * max(sim.n_paths_local, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    price, se, stats, res = ctx.price_localvol_smile(opt or option(), sim, smile, steps, strikes, surface, s)
    torch.cuda.synchronize()
    spots = s[:len(steps) * sim.n_paths_local].cpu().numpy().reshape(len(steps), sim.n_paths_local) if want_spots else None
    return price, se, stats, res, spots


# ---- 1. spots against the restatement --------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", SPOT_CASES, ids=lambda c: f"{c[0]}-{c[2]}" + ("-deep" if c[1] == DEEP else ""))
def test_spots_against_the_restatement(ctx, surfaces, prec, case):
    surface, (seed, first, n_job), n_steps, steps = case
    want = wanted_spots(prec, case)
    tol = spot_tolerance(prec, want)
    sim = capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=N_LOCAL)
    strikes = [80.0, 100.0, 125.0]
    price, se, stats, res, spots = run(ctx, sim, capi.PAYOFF_CALL, steps, strikes, surfaces[surface])
    got = spots.astype(np.float64)
    assert np.isfinite(got).all() and res.grid == N_LOCAL // 256
    err = np.abs(got - want)
    k = np.unravel_index(int(np.argmax(err - tol)), err.shape)
    print(f"{surface} prec {prec} n_steps {n_steps} first path {first} expiries {steps}: restatement spread "
          f"{measured_spread(prec):.3e}, tolerance {tol.min():.3e}..{tol.max():.3e}, worst deviation {err.max():.3e}")
    assert (err <= tol).all(), (k, got[k], want[k], tol[k])
    check_result_fields(res, stats, N_LOCAL, steps, len(strikes), n_steps, BASE["r"], BASE["T"])
    check_sums_from_spots(prec, spots, strikes, capi.PAYOFF_CALL, stats, f"{surface} prec {prec}")
    want_price, want_se = sm.finalize(stats, N_LOCAL, BASE["r"], BASE["T"], n_steps, steps, len(strikes))
    assert np.allclose(price, want_price, rtol=1e-13, atol=0) and np.allclose(se, want_se, rtol=1e-9, atol=0)


# ---- 2. the strike phase alone ---------------------------------------------------------------------------------------------

STRIKE_STEPS = 40
EXPIRIES = {1: (40,), 2: (7, 40), 3: (1, 20, 39), 32: tuple(range(2, 34))}
SHAPES = [(1, 1), (1, 2), (3, 63), (2, 64), (32, 64)]
PATH_COUNTS = [1, 2, 63, 64, 65, 255, 257, 4097]


def pollute(ctx, surfaces, sim, payoff, steps, strikes):
    """another pricer, then another smile of the same shape whose every node pays, leave their numbers in the scratch"""
    ctx.price_localvol(capi.make_option(**dict(BASE, K=60.0, v=0.0)), sim, capi.make_localvol(q=Q_DIV), surfaces["narrow"])
    other = [1e-3 * k for k in strikes] if payoff == capi.PAYOFF_CALL else [1e3 * k for k in strikes]
    _, _, stats, _, _ = run(ctx, capi.make_sim(sim.n_paths, sim.n_steps, sim.precision, seed=sim.seed + 1,
                                               n_paths_local=sim.n_paths_local),
                            payoff, steps, other, surfaces["narrow"], False)
    assert (stats > 0).all()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("payoff", PAYOFFS)
@pytest.mark.parametrize("n_e,n_K", SHAPES)
def test_node_sums_from_the_returned_spots(ctx, surfaces, prec, payoff, n_e, n_K):
    steps, strikes = EXPIRIES[n_e], strikes_for(n_K)
    for n in PATH_COUNTS:
        sim = capi.make_sim(20_000, STRIKE_STEPS, prec, seed=77, path_offset=5003, n_paths_local=n)
        _, _, stats, res, spots = run(ctx, sim, payoff, steps, strikes, surfaces["skew"])
        assert np.isfinite(spots).all() and res.grid == -(-n // 256)
        want, paying = check_sums_from_spots(prec, spots, strikes, payoff, stats,
                                             f"({n_e}, {n_K}) payoff {payoff} prec {prec} n {n}")
        if n_K > 1:
            assert (want == 0).any() and (paying == n).any()
        check_result_fields(res, stats, n, steps, n_K, STRIKE_STEPS, BASE["r"], BASE["T"])
        # what the scratch buffer held before plays no part
        pollute(ctx, surfaces, sim, payoff, steps, strikes)
        _, _, again, _, spots_again = run(ctx, sim, payoff, steps, strikes, surfaces["skew"])
        assert np.array_equal(again, stats) and np.array_equal(spots_again, spots)


@pytest.mark.parametrize("prec", PRECS)
def test_wavefronts_that_make_several_trips(ctx, surfaces, prec):
    """32 x 64 nodes cap the grid lowest; 3 grid 256 + 77 paths then send every wavefront on three or four trips, the
    last of them partial: the read-modify-write of the records runs.  32 expiries need 32 steps (not 3)."""
    steps, strikes, payoff = tuple(range(1, 33)), strikes_for(64), capi.PAYOFF_CALL
    first = run(ctx, capi.make_sim(600_000, 32, prec, seed=5), payoff, steps, strikes, surfaces["skew"], False)[3]
    n = 3 * first.grid * 256 + 77
    assert first.grid < -(-600_000 // 256) and n > first.grid * 256
    sim = capi.make_sim(n, 32, prec, seed=5)
    _, _, stats, res, spots = run(ctx, sim, payoff, steps, strikes, surfaces["skew"])
    assert res.grid == first.grid and n > res.grid * 256 and np.isfinite(spots).all()
    check_sums_from_spots(prec, spots, strikes, payoff, stats, f"several trips prec {prec} grid {res.grid} n {n}", threads=8)
    check_result_fields(res, stats, n, steps, 64, 32, BASE["r"], BASE["T"])
    pollute(ctx, surfaces, sim, payoff, steps, strikes)
    again = run(ctx, sim, payoff, steps, strikes, surfaces["skew"], False)[2]
    assert np.array_equal(again, stats)


# ---- 3. against the pricer it extends ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("payoff", PAYOFFS)
def test_the_last_step_is_the_localvol_pricer(ctx, surfaces, prec, payoff):
    seed, first, n_job = SHALLOW
    strikes = [70.0, 90.0, 100.0, 115.0, 140.0]
    sim = capi.make_sim(n_job, 50, prec, seed=seed, path_offset=first, n_paths_local=N_LOCAL)
    _, _, stats, res, _ = run(ctx, sim, payoff, (13, 50), strikes, surfaces["skew"], False)
    rt = SUM_RTOL[prec]
    for k, K in enumerate(strikes):
        one = ctx.price_localvol(capi.make_option(**dict(BASE, K=K, v=0.0)), sim, capi.make_localvol(payoff, q=Q_DIV),
                                 surfaces["skew"])
        got, gotsq = stats[5 + k], stats[15 + k]
        print(f"prec {prec} payoff {payoff} K {K}: sum {got!r} against {one.sum!r}")
        assert one.sum > 0 and abs(got - one.sum) <= rt * one.sum and abs(gotsq - one.sumsq) <= rt * one.sumsq
    assert (res.work_steps, res.n) == (one.work_steps, one.n)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("payoff", PAYOFFS)
def test_an_inner_expiry_on_the_flat_surface_is_the_shorter_job(ctx, surfaces, prec, payoff):
    strikes, steps, n_steps = [90.0, 100.0, 110.0], (1, 6, 12), 12
    sim = capi.make_sim(N_LOCAL, n_steps, prec, seed=8)
    _, _, stats, _, _ = run(ctx, sim, payoff, steps, strikes, surfaces["flat"], False)
    rt = FLAT_INNER_RTOL[prec]
    for (m, s), (k, K) in itertools.product(enumerate(steps), enumerate(strikes)):
        opt = capi.make_option(**dict(BASE, T=BASE["T"] * s / n_steps, K=K, v=0.0))
        one = ctx.price_localvol(opt, capi.make_sim(N_LOCAL, s, prec, seed=8), capi.make_localvol(payoff, q=Q_DIV),
                                 surfaces["flat"])
        got, gotsq = stats[m * 3 + k], stats[9 + m * 3 + k]
        assert abs(got - one.sum) <= rt * one.sum and abs(gotsq - one.sumsq) <= rt * one.sumsq, (s, K, got, one.sum)
    assert stats[:9].max() > 0


# ---- 4. closed forms -------------------------------------------------------------------------------------------------------

# strikes within a standard deviation and a half of the forward at the first expiry: every node has a vega to speak of
CLOSED_STEPS, CLOSED_EXPIRIES, CLOSED_STRIKES, CLOSED_PATHS = 12, (1, 6, 12), [92.0, 96.0, 100.0, 104.0, 108.0], 1 << 19
CLOSED_SEED = {"time": 2031, "flat": 2032}


def rms_vol(surface, s):
    """the rms volatility over steps 0 .. s - 1 of CLOSED_STEPS on a surface that varies in time only"""
    (n_t, _, _, _), sigma = SURFACES[surface]
    rows = [sigma[(i * n_t) // CLOSED_STEPS][0] for i in range(s)]
    return math.sqrt(sum(v * v for v in rows) / s)


def closed_prices(surface, payoff):
    return np.array([[capi.bs_price_f64(BASE["S0"], K, BASE["T"] * s / CLOSED_STEPS, BASE["r"], Q_DIV, rms_vol(surface, s),
                                        payoff) for K in CLOSED_STRIKES] for s in CLOSED_EXPIRIES])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("payoff", PAYOFFS)
@pytest.mark.parametrize("surface", ["time", "flat"])
def test_closed_forms_at_every_node(ctx, surfaces, surface, payoff, prec):
    """sigma depends on the slice alone: X_s is normal with variance sum s_i^2 dt whatever the step count, so every node
    prices to Black-Scholes at the rms volatility up to its expiry, discounted to that expiry"""
    sim = capi.make_sim(CLOSED_PATHS, CLOSED_STEPS, prec, seed=CLOSED_SEED[surface])
    price, se, _, res, _ = run(ctx, sim, payoff, CLOSED_EXPIRIES, CLOSED_STRIKES, surfaces[surface], False)
    want = closed_prices(surface, payoff)
    off = (price - want) / se
    print(f"{surface} prec {prec} payoff {payoff}: deviations in SE\n{np.array2string(off, precision=2)}\n"
          f"kernel {res.kernel_ms:.3f} ms, total {res.total_ms:.3f} ms")
    assert (se > 0).all() and (np.abs(price - want) <= 4.0 * se).all()
    if surface == "flat":
        times = [BASE["T"] * s / CLOSED_STEPS for s in CLOSED_EXPIRIES]
        vols = capi.implied_vols(BASE["S0"], CLOSED_STRIKES, times, BASE["r"], Q_DIV, price, payoff)
        for (m, t), (k, K) in itertools.product(enumerate(times), enumerate(CLOSED_STRIKES)):
            d1 = (math.log(BASE["S0"] / K) + (BASE["r"] - Q_DIV + 0.02) * t) / (0.2 * math.sqrt(t))
            vega = BASE["S0"] * math.exp(-Q_DIV * t) * math.sqrt(t) * math.exp(-0.5 * d1 * d1) / math.sqrt(2.0 * math.pi)
            assert abs(vols[m, k] - 0.2) <= 4.0 * se[m, k] / vega, (t, K, vols[m, k], se[m, k], vega)
        print(f"implied volatilities\n{np.array2string(vols, precision=5)}")


# ---- 5. plumbing -----------------------------------------------------------------------------------------------------------

SOME_STEPS, SOME_STRIKES = (3, 8, 13), [60.0, 85.0, 100.0, 120.0, 170.0]


@pytest.mark.parametrize("prec", PRECS)
def test_ten_shards_add_up_to_the_whole_job(ctx, surfaces, prec):
    n, cuts = 10_001, (0, 1, 64, 1000, 1001, 4097, 5000, 5000, 7777, 9999, 10_001)
    whole = run(ctx, capi.make_sim(n, 13, prec, seed=3), capi.PAYOFF_PUT, SOME_STEPS, SOME_STRIKES, surfaces["skew"])
    total, count = np.zeros_like(whole[2]), 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sim = capi.make_sim(n, 13, prec, seed=3, path_offset=lo, n_paths_local=hi - lo)
        price, se, stats, res, spots = run(ctx, sim, capi.PAYOFF_PUT, SOME_STEPS, SOME_STRIKES, surfaces["skew"])
        if hi == lo:   # an empty shard: zeros, nothing launched
            assert all(v == 0 for v in res.as_dict().values()) and not stats.any() and not price.any() and not se.any()
            continue
        assert np.array_equal(spots, whole[4][:, lo:hi])
        total, count = total + stats, count + res.n
    assert count == n and (whole[2] > 0).sum() >= 20 and (np.abs(total - whole[2]) <= SUM_RTOL[prec] * whole[2]).all()
    price, se = capi.finalize_smile(total, count, option(), 13, capi.make_smile(3, 5, capi.PAYOFF_PUT, Q_DIV), SOME_STEPS)
    assert np.allclose(price, whole[0], rtol=10 * SUM_RTOL[prec], atol=0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [3000, 300_000])
def test_same_bits_twice_and_from_the_enqueue_form(ctx, surfaces, prec, n):
    sim = capi.make_sim(n + 9, 13, prec, seed=4, path_offset=9, n_paths_local=n)
    a = run(ctx, sim, capi.PAYOFF_CALL, SOME_STEPS, SOME_STRIKES, surfaces["skew"])
    b = run(ctx, sim, capi.PAYOFF_CALL, SOME_STEPS, SOME_STRIKES, surfaces["skew"])
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[4], b[4]) and (a[2] > 0).sum() >= 20
    assert a[3].grid == -(-n // 256)
    smile = capi.make_smile(3, 5, capi.PAYOFF_CALL, Q_DIV)
    stats = torch.full((31,), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.full((3 * n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    ctx.price_localvol_smile_enqueue(option(), sim, smile, SOME_STEPS, SOME_STRIKES, surfaces["skew"], stats, s)
    ms = ctx.enqueued_kernel_ms(1)
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    assert np.array_equal(rec[:30], a[2]) and rec[30] == float(n)
    assert np.array_equal(s.cpu().numpy().reshape(3, n), a[4])
    price, se = capi.finalize_smile(rec, n, option(), 13, smile, SOME_STEPS)
    assert np.array_equal(price, a[0]) and np.array_equal(se, a[1]) and 0.0 < ms[0] < 1e4
    # an empty shard: zeros, n included, still ordered on the stream
    ctx.price_localvol_smile_enqueue(option(), capi.make_sim(n, 13, prec, seed=4, path_offset=5, n_paths_local=0), smile,
                                     SOME_STEPS, SOME_STRIKES, surfaces["skew"], stats)
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()


@pytest.mark.parametrize("prec", PRECS)
def test_two_surfaces_and_eight_enqueued_calls_back_to_back(ctx, surfaces, prec):
    """enqueued without a wait between them, the smile's shape changing from call to call: each call sees its own table
    and its own records"""
    sim = capi.make_sim(10_000, 13, prec, seed=21)
    jobs = [("skew", SOME_STEPS, SOME_STRIKES), ("flat", (13,), [100.0]), ("skew", (1, 2), strikes_for(64)),
            ("flat", SOME_STEPS, SOME_STRIKES)]
    alone = [run(ctx, sim, capi.PAYOFF_PUT, steps, strikes, surfaces[name])[2] for name, steps, strikes in jobs]
    assert not np.array_equal(alone[0], alone[3])
    stats = [torch.full((2 * len(j[1]) * len(j[2]) + 1,), float("nan"), dtype=torch.float64, device="cuda") for j in jobs * 2]
    for i, (name, steps, strikes) in enumerate(jobs * 2):
        ctx.price_localvol_smile_enqueue(option(), sim, capi.make_smile(len(steps), len(strikes), capi.PAYOFF_PUT, Q_DIV),
                                         steps, strikes, surfaces[name], stats[i])
    torch.cuda.synchronize()
    for i in range(8):
        rec = stats[i].cpu().numpy()
        assert np.array_equal(rec[:-1], alone[i % 4]) and rec[-1] == 10_000.0


def test_refusals_with_a_live_context(ctx, surfaces):
    sim, smile = capi.make_sim(1000, 13), capi.make_smile(3, 5, q=Q_DIV)
    ok = run(ctx, sim, capi.PAYOFF_CALL, SOME_STEPS, SOME_STRIKES, surfaces["skew"], False)
    same = run(ctx, capi.make_sim(1000, 13, flags=capi.FLAG_LOG_SPACE), capi.PAYOFF_CALL, SOME_STEPS, SOME_STRIKES,
               surfaces["skew"], False)
    assert np.array_equal(ok[2], same[2]) and (ok[2] > 0).sum() >= 20
    stats = torch.zeros(31, dtype=torch.float64, device="cuda")
    # a surface serves the context it was created on and no other
    other = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        with other.localvol_surface(*SURFACES["skew"]) as foreign:
            for call in (lambda: ctx.price_localvol_smile(option(), sim, smile, SOME_STEPS, SOME_STRIKES, foreign),
                         lambda: ctx.price_localvol_smile_enqueue(option(), sim, smile, SOME_STEPS, SOME_STRIKES, foreign,
                                                                  stats)):
                with pytest.raises(capi.McamdError) as e:
                    call()
                assert e.value.code == capi.ERR_INVALID and "another context" in str(e.value)
            mine = other.price_localvol_smile(option(), sim, smile, SOME_STEPS, SOME_STRIKES, foreign)
            assert np.array_equal(mine[2], ok[2])
    finally:
        other.close()
    # the fp64 exponent-range bound is taken at the surface's largest entry
    with ctx.localvol_surface((1, 2, -1.0, 1.0), [[0.2, 100.0]]) as wild:
        with pytest.raises(capi.McamdError) as e:
            ctx.price_localvol_smile(capi.make_option(**dict(BASE, T=100.0, v=0.0)), capi.make_sim(1000, 50), smile,
                                     SOME_STEPS, SOME_STRIKES, wild)
        assert e.value.code == capi.ERR_INVALID and "exponent range" in str(e.value)
    # an empty shard: all zeros, nothing launched
    price, se, stats0, res, _ = run(ctx, capi.make_sim(1000, 13, path_offset=10, n_paths_local=0), capi.PAYOFF_CALL,
                                    SOME_STEPS, SOME_STRIKES, surfaces["skew"], False)
    assert all(v == 0 for v in res.as_dict().values()) and not stats0.any() and not price.any() and not se.any()
