"""GPU tests of the Heston smile pricer (mcamd_price_heston_smile).  Run with -m gpu on an MI355X.  Everything
elementwise goes through d_state: the spots at every expiry, then the raw variances at every expiry.

  1. spots and variances elementwise against the numpy restatement (tests/heston_smile_restate.py) on the two normal
     streams drawn from the oracle's rocRAND-exact generator, 300 paths (two workgroups, the last wavefront with 44 valid
     lanes): A, the shallow ids, 50 steps, expiries (1, 2, 3, 4, 5, 25, 26, 49, 50) — an expiry on every position of a
     Philox block in both precisions, consecutive expiries, the first and the last step —; B, the deep ids and seed,
     7 steps, expiries (3, 6): the walk ends inside the remainder block, below n_steps; C, 1 step.  Inputs F and N in
     both precisions, H in fp64 (under 82 % truncation fp32 paths diverge pathwise: tests/test_heston_cpu.py);
  2. the strike phase alone: node sums against sums formed in numpy from the returned spots (h in the path precision,
     summed in float64), (n_e, n_K) in {(1, 1), (3, 63), (32, 64)}, calls and puts, strikes geomspace(5, 2000, n_K) so
     that some nodes never pay, n_paths_local in {1, 63, 64, 65, 257, 4097}, and one job of 3 grid 256 + 77 paths at
     (32, 64) x 32 steps whose wavefronts make several trips; every job is run again after a mcamd_price_heston call and
     another smile have used the context's scratch buffer, and must not move by a bit;
  3. against the pricers it extends: with the last expiry at n_steps the last spots and variances are
     mcamd_price_heston's d_state bit for bit and every strike's sums are its sum and sumsq; with xi = 0 and kappa = 0
     the spots are mcamd_price_localvol_smile's on a flat 1 x 2 surface at sqrt(v0);
  4. the closed form: F, calls, 2^18 paths x 128 steps, expiries (32, 64, 96, 128), strikes (80, 90, 100, 110, 120),
     seed 20240611, every node within 4 SE of capi.heston_smile_prices, and the implied volatilities fall with the strike
     at every expiry (rho < 0).  The float64 restatement on the same Philox draws, on the CPU: worst node 2.12 SE (seeds
     5 and 77: 1.36 and 4.35, so the seed is not to be swapped without that check), input N 1.71 SE;
  5. shards (0..100), (100..101), (101..513); the same bits twice at 3000 paths; the enqueue record with its trailing n;
     eight calls enqueued back to back, alternating with mcamd_price_localvol_smile_enqueue; an empty shard; every
     refusal with a live context;
  6. three mistakes restated in numpy only (no mutated kernel is run), each refused by a case of test 1: the expiry
     taken one step late, z' read from block k instead of 2^63 + k, v recorded as v+.

Tolerance of 1 and of the flat-surface comparison of 3 (DESIGN section 23's rule, computed here from the restatements
alone): four times the largest difference between the float64 and longdouble restatements (fp64 kernels) or the float32
and float64 ones (fp32 kernels) over the cases A, B and C of that input, floored at 1e-11 S0 (fp64) / 2e-3 (fp32) for
the spots and at 1e-11 / 2e-5 for the variances.  No path is left out: the step map is continuous.  Tolerance of the
node sums (2, 3): 1e-11 (fp64) / 2e-5 (fp32) of the node's sum, exactly 0 where no path pays.  Shards: 1e-13 relative.

Measured on an x86-64 CPU, the restatement's spreads over A, B, C: S 3.5e-14 / 2.5e-5 (F), 3.3e-13 / 1.1e-4 (N),
2.2e-11 (H, fp64); v 8.9e-17 / 2.9e-8, 2.4e-15 / 6.0e-7, 1.5e-13: the floors decide everywhere.
Measured on an MI355X (each test prints its figures before it asserts), largest deviations of the kernels from the
restatement: S 5.7e-14 (F), 3.7e-13 (N), 8.9e-11 (H) in fp64 and 2.9e-5 (F), 6.2e-5 (N) in fp32; v 1.1e-16, 2.7e-15,
6.1e-13 and 4.2e-8, 1.9e-7.  Node sums against numpy sums of the returned spots: 3.5e-15 relative at most in fp64 (the
several-trip job, grid 512, 393 293 paths), equal in fp32.  Against mcamd_price_heston: d_state bit-equal in every case,
sums within 2.7e-16 (fp64) / 2.6e-7 (fp32) relative.  Against the flat surface's smile: 5.7e-14 / 1.5e-5.  Shards:
1.9e-16 / 3.6e-16 relative.  Closed form: worst node 2.12 SE (fp64), 1.26 SE (fp32).  The module runs in 3.3 s."""
import importlib

import numpy as np
import pytest

import heston_restate as hr
import heston_smile_restate as hs
import localvol_smile_restate as sm
from deep_inputs import DEEP, SHALLOW
from smile_cases import SUM_RTOL, check_result_fields, check_sums_from_spots, full_work, strikes_for

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

S0, T_, R, Q = hr.S0, hr.T_, hr.R, hr.Q_DIV
NP_T = {capi.F64: np.float64, capi.F32: np.float32}
WIDER = {capi.F64: np.longdouble, capi.F32: np.float64}
FLOOR = {capi.F64: {"S": 1e-11 * S0, "v": 1e-11}, capi.F32: {"S": 2e-3, "v": 2e-5}}
SHARD_RTOL = 1e-13
PRECS = [capi.F64, capi.F32]
PAYOFFS = [capi.PAYOFF_CALL, capi.PAYOFF_PUT]
N_LOCAL = 300
EVERY_SLOT = (1, 2, 3, 4, 5, 25, 26, 49, 50)
# name: (where, n_steps, expiry steps)
CASES = {"A": (SHALLOW, 50, EVERY_SLOT), "B": (DEEP, 7, (3, 6)), "C": (SHALLOW, 1, (1,))}
INPUTS = [("F", capi.F64), ("F", capi.F32), ("N", capi.F64), ("N", capi.F32), ("H", capi.F64)]


def option():
    # K, v and B are ignored by the call: leave something in them that any use would show
    return capi.make_option(S0=S0, K=float("nan"), r=R, T=T_, v=float("nan"), B=float("nan"))


def model(name, payoff=capi.PAYOFF_CALL, **changes):
    q, v0, kappa, theta, xi, rho = hr.params(name, **changes)
    return capi.make_heston(payoff, q, v0, kappa, theta, xi, rho)


_restated = {}


def restate(prec, name, case, dtype, mutate=None, n=N_LOCAL, **changes):
    """(S, v) of one restatement per (case, dtype), shared by every test that needs it and left unchanged"""
    key = (prec, name, case, np.dtype(dtype).name, mutate, n, tuple(sorted(changes.items())))
    if key not in _restated:
        (seed, first, _), n_steps, steps = CASES[case]
        z, zv = hr.draws(prec, seed, first, n, n_steps)
        _restated[key] = hs.states(z, zv, S0, T_, R, hr.params(name, **changes), n_steps, steps, dtype, mutate)
    return _restated[key]


_tolerance = {}


def tolerance(prec, name):
    """{"S", "v"}: 4 x the precision spread of the restatement over the cases A, B, C of that input, floored"""
    if (prec, name) not in _tolerance:
        worst = {"S": 0.0, "v": 0.0}
        for case in CASES:
            own, wide = restate(prec, name, case, NP_T[prec]), restate(prec, name, case, WIDER[prec])
            for k, a, b in (("S", own[0], wide[0]), ("v", own[1], wide[1])):
                worst[k] = max(worst[k], float(np.abs(a.astype(np.longdouble) - b.astype(np.longdouble)).max()))
        _tolerance[(prec, name)] = ({k: max(4.0 * worst[k], FLOOR[prec][k]) for k in worst}, worst)
    return _tolerance[(prec, name)][0]


def test_restatement_spread():
    """no kernel runs: what the tolerance of test 1 is made of"""
    for name, prec in INPUTS:
        tol = tolerance(prec, name)
        print(f"{name} fp{prec}: restatement spread {_tolerance[(prec, name)][1]}, tolerance {tol}")
        assert all(np.isfinite(x) for x in tol.values())
        if name != "H":   # the floors decide
            assert tol == FLOOR[prec]


# ---- 6. mistakes, restated in numpy only -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name,prec", INPUTS)
def test_mistakes_restated_in_numpy_are_beyond_the_tolerances(name, prec):
    """no kernel runs.  Each mistake moves the restated result of case A of test 1 by more than its tolerance, so test 1
    refuses a kernel that makes it."""
    tol = tolerance(prec, name)
    S, v = (a.astype(np.float64) for a in restate(prec, name, "A", np.float64))
    # an expiry taken one step late: nearly every path of every expiry but the last, which has no later step
    late_S, late_v = (a.astype(np.float64) for a in restate(prec, name, "A", np.float64, mutate=hs.LATE_EXPIRY))
    assert (np.abs(late_S - S)[:-1] > tol["S"]).mean() > 0.99 and (np.abs(late_v - v)[:-1] > tol["v"]).mean() > 0.95
    # z' read from the log-price's blocks: the variance of every path from the first step on
    same_S, same_v = (a.astype(np.float64) for a in restate(prec, name, "A", np.float64, mutate=hs.SAME_BLOCKS))
    # ... and through it the spot, from the second step on (at the last expiry: under H both variances are often below
    # zero together, and then a step moves both spots alike)
    assert (np.abs(same_v - v) > tol["v"]).mean() > 0.99 and (np.abs(same_S - S)[-1] > tol["S"]).mean() > 0.5
    # v recorded as v+: every entry at which the raw variance is below zero by more than the tolerance; N and H have some
    plus_S, plus_v = (a.astype(np.float64) for a in restate(prec, name, "A", np.float64, mutate=hs.V_PLUS))
    assert np.array_equal(plus_S, S)
    if name != "F":
        assert (v < -tol["v"]).any() and (np.abs(plus_v - v) > tol["v"]).sum() == (v < -tol["v"]).sum()


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
def flat(ctx):
    v0 = hr.MODELS["F"][0]
    with ctx.localvol_surface((1, 2, -1.0, 1.0), [[np.sqrt(v0), np.sqrt(v0)]]) as surface:
        yield surface


def run(ctx, sim, hs_model, steps, strikes, want_state=True):
    """(price, std_err, stats, res, S [n_e, n_local], v [n_e, n_local] in the path precision, or None)"""
    n, n_e = sim.n_paths_local, len(steps)
    st = None
    if want_state:
        st = torch.full((2 * n_e * max(n, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    price, se, stats, res = ctx.price_heston_smile(option(), sim, hs_model, steps, strikes, st)
    torch.cuda.synchronize()
    if not want_state:
        return price, se, stats, res, None, None
    a = st[:2 * n_e * n].cpu().numpy().reshape(2, n_e, n)
    return price, se, stats, res, a[0], a[1]


def shard(prec, case, n=N_LOCAL):
    (seed, first, n_job), n_steps, _ = CASES[case]
    return capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=n)


# ---- 1. spots and variances against the restatement -----------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name,prec", INPUTS)
def test_spots_and_variances_against_the_restatement(ctx, name, prec, case):
    _, n_steps, steps = CASES[case]
    tol = tolerance(prec, name)
    want_S, want_v = (a.astype(np.float64) for a in restate(prec, name, case, np.float64))
    strikes = [80.0, 100.0, 125.0]
    price, se, stats, res, S, v = run(ctx, shard(prec, case), model(name), steps, strikes)
    got_S, got_v = S.astype(np.float64), v.astype(np.float64)
    assert np.isfinite(got_S).all() and np.isfinite(got_v).all() and res.grid == 2
    err_S, err_v = np.abs(got_S - want_S), np.abs(got_v - want_v)
    print(f"{name} fp{prec} case {case} ({n_steps} steps, expiries {steps}): worst deviation S {err_S.max():.3e} "
          f"(tolerance {tol['S']:.1e}), v {err_v.max():.3e} (tolerance {tol['v']:.1e}), entries with v < 0 "
          f"{(got_v < 0).sum()} of {got_v.size}")
    assert (err_S <= tol["S"]).all(), np.unravel_index(int(np.argmax(err_S)), err_S.shape)
    assert (err_v <= tol["v"]).all(), np.unravel_index(int(np.argmax(err_v)), err_v.shape)
    if name == "H" and case == "A":
        assert (got_v < 0).any()   # the raw variance
    if case == "C":
        assert (got_v != hr.MODELS[name][0]).all()
    check_result_fields(res, stats, N_LOCAL, steps, len(strikes), n_steps, R, T_)
    check_sums_from_spots(prec, S, strikes, capi.PAYOFF_CALL, stats, f"{name} fp{prec} case {case}")
    want_price, want_se = sm.finalize(stats, N_LOCAL, R, T_, n_steps, steps, len(strikes))
    assert np.allclose(price, want_price, rtol=1e-13, atol=0) and np.allclose(se, want_se, rtol=1e-9, atol=0)


# ---- 2. the strike phase alone ---------------------------------------------------------------------------------------------

STRIKE_STEPS = 32
EXPIRIES = {1: (32,), 3: (1, 16, 31), 32: tuple(range(1, 33))}
SHAPES = [(1, 1), (3, 63), (32, 64)]
PATH_COUNTS = [1, 63, 64, 65, 257, 4097]


def pollute(ctx, sim, payoff, steps, strikes):
    """a mcamd_price_heston call, then another smile of the same shape whose every node pays, leave their numbers in the
    context's scratch buffer"""
    one = ctx.price_heston(capi.make_option(S0=S0, K=60.0, r=R, T=T_), sim, model("N", payoff))
    assert one.n == sim.n_paths_local
    other = [1e-3 * k for k in strikes] if payoff == capi.PAYOFF_CALL else [1e3 * k for k in strikes]
    far = capi.make_sim(sim.n_paths, sim.n_steps, sim.precision, seed=sim.seed + 1, n_paths_local=sim.n_paths_local)
    stats = run(ctx, far, model("N", payoff), steps, other, False)[2]
    assert (stats > 0).all()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("payoff", PAYOFFS)
@pytest.mark.parametrize("n_e,n_K", SHAPES)
def test_node_sums_from_the_returned_spots(ctx, prec, payoff, n_e, n_K):
    steps, strikes = EXPIRIES[n_e], strikes_for(n_K)
    for n in PATH_COUNTS:
        sim = capi.make_sim(20_000, STRIKE_STEPS, prec, seed=77, path_offset=5003, n_paths_local=n)
        _, _, stats, res, S, v = run(ctx, sim, model("F", payoff), steps, strikes)
        assert np.isfinite(S).all() and np.isfinite(v).all() and res.grid == -(-n // 256)
        want, paying = check_sums_from_spots(prec, S, strikes, payoff, stats,
                                             f"({n_e}, {n_K}) payoff {payoff} fp{prec} n {n}")
        if n_K > 1:
            assert (want == 0).any() and (paying == n).any()
        check_result_fields(res, stats, n, steps, n_K, STRIKE_STEPS, R, T_)
        # what the scratch buffer held before plays no part
        pollute(ctx, sim, payoff, steps, strikes)
        _, _, again, _, S_again, v_again = run(ctx, sim, model("F", payoff), steps, strikes)
        assert np.array_equal(again, stats) and np.array_equal(S_again, S) and np.array_equal(v_again, v)


@pytest.mark.parametrize("prec", PRECS)
def test_wavefronts_that_make_several_trips(ctx, prec):
    """32 x 64 nodes cap the grid lowest; 3 grid 256 + 77 paths then send every wavefront on three or four trips, the
    last of them partial: the read-modify-write of the records runs"""
    steps, strikes, payoff = EXPIRIES[32], strikes_for(64), capi.PAYOFF_CALL
    first = run(ctx, capi.make_sim(600_000, STRIKE_STEPS, prec, seed=5), model("F"), steps, strikes, False)[3]
    n = 3 * first.grid * 256 + 77
    assert first.grid < -(-600_000 // 256) and n > first.grid * 256
    sim = capi.make_sim(n, STRIKE_STEPS, prec, seed=5)
    _, _, stats, res, S, _ = run(ctx, sim, model("F"), steps, strikes)
    assert res.grid == first.grid and np.isfinite(S).all()
    check_sums_from_spots(prec, S, strikes, payoff, stats, f"several trips fp{prec} grid {res.grid} n {n}", threads=8)
    check_result_fields(res, stats, n, steps, 64, STRIKE_STEPS, R, T_)
    pollute(ctx, sim, payoff, steps, strikes)
    again = run(ctx, sim, model("F"), steps, strikes, False)[2]
    assert np.array_equal(again, stats)


# ---- 3. against the pricers it extends ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("payoff", PAYOFFS)
@pytest.mark.parametrize("name,prec", INPUTS + [("H", capi.F32)])
def test_the_last_step_is_the_heston_pricer(ctx, name, prec, payoff):
    """the last expiry at n_steps: mcamd_price_heston's S_T and v_n bit for bit (H in fp32 too: the same operations on
    the same draws, whatever the truncation), and its sums for every strike"""
    strikes = [70.0, 90.0, 100.0, 115.0, 140.0]
    for case, steps in (("A", (13, 50)), ("B", (2, 7)), ("C", (1,))):
        sim = shard(prec, case)
        _, _, stats, res, S, v = run(ctx, sim, model(name, payoff), steps, strikes)
        nodes, rt, worst = len(steps) * 5, SUM_RTOL[prec], 0.0
        for k, K in enumerate(strikes):
            state = torch.full((2 * N_LOCAL,), float("nan"), dtype=TORCH_T[prec], device="cuda")
            one = ctx.price_heston(capi.make_option(S0=S0, K=K, r=R, T=T_), sim, model(name, payoff), None, state)
            torch.cuda.synchronize()
            st = state.cpu().numpy()
            assert np.array_equal(S[-1], st[:N_LOCAL]) and np.array_equal(v[-1], st[N_LOCAL:])
            got, gotsq = stats[nodes - 5 + k], stats[2 * nodes - 5 + k]
            assert abs(got - one.sum) <= rt * one.sum and abs(gotsq - one.sumsq) <= rt * one.sumsq, (K, got, one.sum)
            if one.sum > 0:
                worst = max(worst, abs(got - one.sum) / one.sum)
        print(f"{name} fp{prec} payoff {payoff} case {case}: d_state bit-equal; worst relative deviation of a strike's "
              f"sum from mcamd_price_heston's {worst:.3e}")
        assert (res.work_steps, res.n) == (one.work_steps, one.n)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", list(CASES))
def test_constant_variance_against_the_localvol_smile(ctx, flat, prec, case):
    _, _, steps = CASES[case]
    v0, tol, sim = hr.MODELS["F"][0], tolerance(prec, "F"), shard(prec, case)
    strikes = [90.0, 100.0, 110.0]
    _, _, stats, _, S, v = run(ctx, sim, model("F", xi=0.0, kappa=0.0, theta=0.3), steps, strikes)
    spots = torch.full((len(steps) * N_LOCAL,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    lv = ctx.price_localvol_smile(capi.make_option(S0=S0, r=R, T=T_), sim, capi.make_smile(len(steps), 3, q=Q), steps,
                                  strikes, flat, spots)
    torch.cuda.synchronize()
    want = spots.cpu().numpy().reshape(len(steps), N_LOCAL).astype(np.float64)
    err = np.abs(S.astype(np.float64) - want).max()
    print(f"fp{prec} case {case}: worst deviation from mcamd_price_localvol_smile's spots {err:.3e} "
          f"(tolerance {tol['S']:.1e})")
    assert err <= tol["S"] and (v == NP_T[prec](v0)).all()
    assert stats.shape == lv[2].shape and (stats[:stats.size // 2] > 0).all()


# ---- 4. the closed form -------------------------------------------------------------------------------------------------------

CLOSED_STEPS, CLOSED_EXPIRIES, CLOSED_STRIKES = 128, (32, 64, 96, 128), [80.0, 90.0, 100.0, 110.0, 120.0]
CLOSED_PATHS, CLOSED_SEED = 1 << 18, 20240611


@pytest.mark.parametrize("prec", PRECS)
def test_closed_form_at_every_node_and_the_skew(ctx, prec):
    q, v0, kappa, theta, xi, rho = hr.params("F")
    sim = capi.make_sim(CLOSED_PATHS, CLOSED_STEPS, prec, seed=CLOSED_SEED)
    price, se, _, res, _, _ = run(ctx, sim, model("F"), CLOSED_EXPIRIES, CLOSED_STRIKES, False)
    times = [T_ * s / CLOSED_STEPS for s in CLOSED_EXPIRIES]
    want = capi.heston_smile_prices(S0, CLOSED_STRIKES, times, R, q, v0, kappa, theta, xi, rho, capi.PAYOFF_CALL)
    off = (price - want) / se
    vols = capi.implied_vols(S0, CLOSED_STRIKES, times, R, q, price, capi.PAYOFF_CALL)
    print(f"F fp{prec}: deviations from the closed form in SE (worst {np.abs(off).max():.2f})\n"
          f"{np.array2string(off, precision=2)}\nimplied volatilities\n{np.array2string(vols, precision=5)}\n"
          f"kernel {res.kernel_ms:.3f} ms, total {res.total_ms:.3f} ms")
    assert (se > 0).all() and (np.abs(price - want) <= 4.0 * se).all()
    assert np.isfinite(vols).all() and (np.diff(vols, axis=1) < 0).all()   # rho < 0: the skew falls with the strike
    assert res.grid == CLOSED_PATHS // 256 and res.work_steps == full_work(CLOSED_PATHS, 128)


# ---- 5. plumbing -----------------------------------------------------------------------------------------------------------

SOME_STEPS, SOME_STRIKES = (3, 8, 12), [60.0, 85.0, 100.0, 120.0, 170.0]


@pytest.mark.parametrize("prec", PRECS)
def test_three_shards_add_up_to_the_whole_job(ctx, prec):
    n, n_steps = 513, 12
    whole = run(ctx, capi.make_sim(n, n_steps, prec, seed=3), model("N", capi.PAYOFF_PUT), SOME_STEPS, SOME_STRIKES)
    assert whole[3].grid == 3 and (whole[2] > 0).sum() >= 20 and (whole[5] < 0).any()
    total, count = np.zeros_like(whole[2]), 0
    for lo, hi in ((0, 100), (100, 101), (101, 513)):
        sim = capi.make_sim(n, n_steps, prec, seed=3, path_offset=lo, n_paths_local=hi - lo)
        _, _, stats, res, S, v = run(ctx, sim, model("N", capi.PAYOFF_PUT), SOME_STEPS, SOME_STRIKES)
        assert np.array_equal(S, whole[4][:, lo:hi]) and np.array_equal(v, whole[5][:, lo:hi])
        total, count = total + stats, count + res.n
    worst = float(np.max(np.abs(total - whole[2]) / np.where(whole[2] > 0, whole[2], 1.0)))
    print(f"fp{prec}: worst relative deviation of the shards' total from the whole job {worst:.3e}")
    assert count == n and (np.abs(total - whole[2]) <= SHARD_RTOL * whole[2]).all()
    smile = capi.make_smile(3, 5)
    price, se = capi.finalize_smile(total, count, option(), n_steps, smile, SOME_STEPS)
    assert np.allclose(price, whole[0], rtol=1e-12, atol=0)


@pytest.mark.parametrize("prec", PRECS)
def test_same_bits_twice_and_from_the_enqueue_form(ctx, prec):
    n, n_steps = 3000, 12
    sim = capi.make_sim(n + 9, n_steps, prec, seed=4, path_offset=9, n_paths_local=n)
    hs_model = model("N")
    a = run(ctx, sim, hs_model, SOME_STEPS, SOME_STRIKES)
    b = run(ctx, sim, hs_model, SOME_STEPS, SOME_STRIKES)
    assert all(np.array_equal(a[i], b[i]) for i in (0, 1, 2, 4, 5)) and (a[2] > 0).sum() >= 20
    assert a[3].grid == -(-n // 256)
    stats = torch.full((31,), float("nan"), dtype=torch.float64, device="cuda")
    state = torch.full((6 * n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    ctx.price_heston_smile_enqueue(option(), sim, hs_model, SOME_STEPS, SOME_STRIKES, stats, state)
    ms = ctx.enqueued_kernel_ms(1)
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    assert np.array_equal(rec[:30], a[2]) and rec[30] == float(n)
    st = state.cpu().numpy().reshape(2, 3, n)
    assert np.array_equal(st[0], a[4]) and np.array_equal(st[1], a[5])
    price, se = capi.finalize_smile(rec, n, option(), n_steps, capi.make_smile(3, 5), SOME_STEPS)
    assert np.array_equal(price, a[0]) and np.array_equal(se, a[1]) and 0.0 < ms[0] < 1e4


@pytest.mark.parametrize("prec", PRECS)
def test_eight_enqueued_calls_alternating_with_the_localvol_smile(ctx, flat, prec):
    """enqueued without a wait between them, the smile's shape changing from call to call: each call sees its own job
    and its own records"""
    sim = capi.make_sim(10_000, 12, prec, seed=21)
    shapes = [(SOME_STEPS, SOME_STRIKES), ((12,), [100.0]), ((1, 2), strikes_for(64)), ((5, 11), [95.0, 105.0])]
    lv_opt = capi.make_option(S0=S0, r=R, T=T_)
    heston_turn = lambda i: (i + i // 4) % 2 == 0   # every shape goes to both families
    alone = []
    for i, (steps, strikes) in enumerate(shapes * 2):
        if heston_turn(i):
            alone.append(run(ctx, sim, model("N", capi.PAYOFF_PUT), steps, strikes, False)[2])
        else:
            alone.append(ctx.price_localvol_smile(lv_opt, sim, capi.make_smile(len(steps), len(strikes), capi.PAYOFF_PUT, Q),
                                                  steps, strikes, flat)[2])
    stats = [torch.full((2 * len(s) * len(k) + 1,), float("nan"), dtype=torch.float64, device="cuda") for s, k in shapes * 2]
    for i, (steps, strikes) in enumerate(shapes * 2):
        if heston_turn(i):
            ctx.price_heston_smile_enqueue(option(), sim, model("N", capi.PAYOFF_PUT), steps, strikes, stats[i])
        else:
            ctx.price_localvol_smile_enqueue(lv_opt, sim, capi.make_smile(len(steps), len(strikes), capi.PAYOFF_PUT, Q),
                                             steps, strikes, flat, stats[i])
    torch.cuda.synchronize()
    for i in range(8):
        rec = stats[i].cpu().numpy()
        assert np.array_equal(rec[:-1], alone[i]) and rec[-1] == 10_000.0 and rec[:-1].any(), i
    assert not np.array_equal(alone[0], alone[4])   # the same shape under the two models


def test_an_empty_shard_launches_nothing(ctx):
    sim = capi.make_sim(1000, 12, path_offset=10, n_paths_local=0)
    price, se, stats, res, _, _ = run(ctx, sim, model("F"), SOME_STEPS, SOME_STRIKES, False)
    assert all(v == 0 for v in res.as_dict().values()) and not stats.any() and not price.any() and not se.any()
    d_stats = torch.full((31,), float("nan"), dtype=torch.float64, device="cuda")
    ctx.price_heston_smile_enqueue(option(), sim, model("F"), SOME_STEPS, SOME_STRIKES, d_stats)
    torch.cuda.synchronize()
    assert not d_stats.cpu().numpy().any()   # zeros, n included, still ordered on the stream


def test_refusals_reach_no_device_and_leave_the_context_usable(ctx):
    import ctypes as C
    from test_heston_smile_cpu import price, refusals
    sim = capi.make_sim(1000, 12)
    before = run(ctx, sim, model("F"), SOME_STEPS, SOME_STRIKES)
    d_stats = torch.zeros(8193, dtype=torch.float64, device="cuda")
    n_cases = 0
    for stage, name, args, kw, words in refusals():
        if name == "no context":
            continue
        for rc, msg in price(ctx._L, *args, ctx=ctx._h, d_stats=C.c_void_p(d_stats.data_ptr()), **kw):
            assert rc == capi.ERR_INVALID and words in msg, (name, msg)
        n_cases += 1
    assert n_cases > 60
    torch.cuda.synchronize()
    assert not d_stats.cpu().numpy().any()
    after = run(ctx, sim, model("F"), SOME_STEPS, SOME_STRIKES)
    assert all(np.array_equal(after[i], before[i]) for i in (0, 1, 2, 4, 5)) and (before[2] > 0).sum() >= 20
