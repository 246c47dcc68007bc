"""CPU checks of what tests/test_gpu_window.py compares the kernels with: the restatement of tests/window_restate.py is
pinned to the oracle (which is pinned to the reference), the margin, tolerances and caps of tests/window_cases.py hold
on the chosen inputs, and each restated mistake lies beyond the tolerance the GPU test allows.  No kernel runs here.

Measured here (printed by the tests; pytest -s):
  * |ln S_t| between the two restatements: at most 4.6e-16 (float64 / longdouble) and 2.3e-7 (float32 / float64, the
    100-step cases), so MARGIN = 2e-5 is 89 times the fp32 figure where 4 are asked for; no case needs a margin of its own;
  * sample spreads: at most 6.4e-14 (fp64) and 3.8e-5 (fp32) on y, 6.4e-14 and 4.9e-5 on the control; the per-sample
    tolerance is then 1.6e-11 .. 1.1e-8 (fp64) and 2.3e-5 .. 2.4e-3 (fp32, the floor 2e-5 of a payoff of 120);
  * undecided samples: at most 1 of 256 in a case (0.4 %); non-zero samples: at least 19 of 256 (7 %);
  * nested MC on the oracle's rows: points without an undecided inner path 96 % (fp32 edges) .. 100 %, summed width
    at most 3.4e-4 of the summed hi, point tolerance 1.2e-9 .. 5.4e-9 (fp64) and 1.9e-4 .. 6.4e-4 (fp32).

The partial last block taking one step too few or too many (test_mistakes_...): against the older point tolerance of
tests/test_gpu_parity.py (rtol 5e-3, atol 2e-3 in fp32) the test prints, per case, how many of the affected paying
points that tolerance would have flagged, and for every price_paths mistake how far it moves the case's sum; the
figures are in the docstring of that test."""
import importlib
import math

import numpy as np
import pytest

import window_cases as wc
import window_restate as wr
from deep_inputs import check_deep_draws_differ

capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
BY = wc.CASE_BY_NAME
PINNED = ("w-7", "w-33", "w-100", "restart-100", "dt-33", "w-61-deep", "w-100-straddle")


def ref_paths(oracle, case, prec, **want):
    opt, sim = wc.option(case), wc.sim(case, prec)
    return oracle.mc_paths(wc.oracle_params(oracle, opt, sim), prec, sim.path_offset, wc.N_PATHS, **want)


@pytest.mark.parametrize("name", PINNED)
def test_float64_restatement_is_the_oracle(oracle, name):
    case = BY[name]
    opt = wc.option(case)
    ref = ref_paths(oracle, case, capi.F64, want_payoffs=True, want_traj=True, want_counts=True)
    got = wc.restated(case, capi.F64, "plain", np.float64)
    m = got.members[0]
    S_start = opt.Sk if opt.Sk != 0 else opt.S0
    assert np.allclose(S_start * np.exp(m.logs), ref["traj"].T, rtol=1e-12, atol=0)
    assert np.array_equal(opt.Ik + np.cumsum(m.below, axis=1), ref["counts"].T)
    assert np.array_equal(m.cnt, ref["counts"][-1])
    assert np.allclose(got.y, ref["payoffs"], rtol=1e-12, atol=0) and np.count_nonzero(got.y) >= 6
    assert ((got.y == 0) == (ref["payoffs"] == 0)).all()
    for form in ("anti", "cv", "anti-cv"):
        flags = wc.FORMS[form]
        s = wc.restated(case, capi.F64, form, np.float64)
        sim = wc.sim(case, capi.F64, flags)
        cm = wr.control_mean_of(opt, sim)
        want = oracle.mc_paths_vr(wc.oracle_params(oracle, opt, sim), capi.F64, sim.path_offset, wc.N_PATHS,
                                  bool(flags & wc.A), cm)
        c = s.ctrl - cm
        mine = [s.y.sum(), (s.y ** 2).sum(), c.sum(), (c ** 2).sum(), (s.y * c).sum()]
        scale = [np.abs(s.y).sum(), (s.y ** 2).sum(), np.abs(c).sum(), (c ** 2).sum(), np.abs(s.y * c).sum()]
        for a, b, sc in zip(mine, want, scale):
            assert abs(a - b) <= 1e-12 * sc, (form, mine, want)


@pytest.mark.parametrize("name", ["edges", "deep", "windowless"])
def test_float64_points_are_the_oracle(oracle, name):
    case = {c.name: c for c in wc.NMC_CASES}[name]
    opt, sim = wc.nmc_option(case), wc.nmc_inner_sim(case, capi.F64)
    St, cnt = wc.oracle_rows(oracle, case, capi.F64)
    got = wr.nmc_points(oracle, opt, sim, St, cnt, np.float64, wc.MARGIN)
    p = wc.oracle_params(oracle, opt, sim)
    for i in range(case.n_local):
        for step in range(case.n_steps):
            want = oracle.nmc_point(p, capi.F64, (case.first + i) * case.n_steps + step, step, float(St[i, step]),
                                    int(cnt[i, step]))
            assert math.isclose(got.price[i, step], want, rel_tol=1e-12, abs_tol=0), (i, step)
            if got.closed[i, step]:
                assert want == 0.0 and got.price[i, step] == 0.0
    assert (got.price > 0).sum() >= case.n_steps


@pytest.mark.parametrize("name", PINNED)
def test_float32_restatement_against_the_oracles_fp32_path(oracle, name):
    case = BY[name]
    opt = wc.option(case)
    ref = ref_paths(oracle, case, capi.F32, want_payoffs=True, want_traj=True, want_counts=True)
    m = wc.restated(case, capi.F32, "plain", np.float32).members[0]
    assert m.logs.dtype == np.float32 and m.S_T.dtype == np.float32
    S_start = np.float32(opt.Sk if opt.Sk != 0 else opt.S0)
    assert np.allclose(S_start * np.exp(m.logs), ref["traj"].T, rtol=2e-5, atol=0)
    clear = wc.restated(case, capi.F32, "plain", np.float64).members[0].min_abs_d >= wc.MARGIN
    assert clear.mean() > 0.98
    assert np.array_equal((opt.Ik + np.cumsum(m.below, axis=1))[clear], ref["counts"].T[clear])


def test_bulk_normals_are_the_per_block_calls(oracle):
    for prec, gen in ((capi.F32, oracle.normal4_f32), (capi.F64, oracle.normal2_f64)):
        for seed, first in ((77, 5003), (2 ** 40 + 77, 2 ** 32 - 2), (2 ** 40 + 77, (2 ** 33 + 12_345) * 7 * 70)):
            z = oracle.normals_of_subsequences(seed, first, 5, 3, prec)
            nb = wr.PER_BLOCK[prec]
            assert z.shape == (5, 3 * nb)
            for s in range(5):
                for b in range(3):
                    assert np.array_equal(z[s, b * nb:(b + 1) * nb], gen(seed, first + s, b))
            assert np.array_equal(wr.normals(oracle, prec, seed, first, 5, 2 * nb + 1), z.astype(np.float64))
            assert np.array_equal(wr.normals_of(oracle, prec, seed, range(first, first + 5), 3 * nb), z.astype(np.float64))


@pytest.mark.parametrize("prec", wc.PRECS)
def test_margin_spreads_and_caps_of_the_price_paths_cases(prec):
    worst_log = 0.0
    for case in wc.WINDOW_CASES + wc.WINDOWLESS_CASES:
        ls = wc.log_spread(case, prec)
        worst_log = max(worst_log, ls)
        assert wc.MARGIN >= 4.0 * ls, (case.name, ls)
        for form in (wc.FORMS if case.extra else wc.WINDOWLESS_FORMS):
            w = wc.wanted(case, prec, form)
            undecided, paying = np.count_nonzero(~w.want.decided), np.count_nonzero(w.want.y)
            lo, hi = w.want.cands.min(axis=1).astype(np.float64), w.want.cands.max(axis=1).astype(np.float64)
            print(f"f{prec} {case.name} {form}: ln S spread {ls:.2e}, spread y {w.spread_y:.2e} c {w.spread_c:.2e}, "
                  f"tolerance {w.tol_y.min():.1e} .. {w.tol_y.max():.1e}, undecided {undecided}, paying {paying}, "
                  f"width {(hi - lo).sum() / hi.sum():.1e}")
            assert undecided <= wc.MAX_UNDECIDED * wc.N_PATHS
            assert paying >= wc.MIN_PAYING * wc.N_PATHS
            assert (hi - lo).sum() <= wc.MAX_WIDTH * hi.sum(), (case.name, form)
            assert (w.tol_y > 0).all() and (w.tol_y <= max(4.0 * w.spread_y, wc.FLOOR[prec] * hi.max()) * 1.0000001).all()
            if not case.extra:
                assert w.want.decided.all()
    print(f"f{prec}: largest ln S spread {worst_log:.2e}, MARGIN / spread = {wc.MARGIN / worst_log:.0f}")


@pytest.mark.parametrize("prec", wc.PRECS)
def test_caps_of_the_nested_mc_cases(oracle, prec):
    for case in wc.NMC_CASES:
        St, cnt = wc.oracle_rows(oracle, case, prec)
        w = wc.nmc_wanted(oracle, case, prec, St, cnt)
        live = ~w.want.closed
        share = w.free.sum() / live.sum()
        width = (w.want.hi - w.want.lo).sum() / w.want.hi.sum()
        print(f"f{prec} {case.name}: {live.sum()} of {live.size} points priced, {share:.3f} of them without an undecided "
              f"inner path, width {width:.1e}, spread {w.spread:.2e}, tolerance {w.tol[live].min():.1e} .. {w.tol.max():.1e}")
        assert share >= wc.MIN_FREE and width <= wc.MAX_WIDTH
        assert (w.want.price[w.want.closed] == 0).all() and (w.tol[w.want.closed] == 0).all()
        for to_go in range(1, case.n_steps):
            assert (w.want.lo[:, case.n_steps - 1 - to_go] > 0).any(), (case.name, to_go)
        if not case.window["use_window"]:
            assert live.all() and w.free.all() and (w.want.lo == w.want.hi).all()
        # the last step's points are the discounted window payoff of the stored price itself
        opt = wc.nmc_option(case)
        last = np.maximum(St[:, -1].astype(np.float64) - opt.K, 0.0) * np.exp(-opt.r * opt.T)
        if opt.use_window:
            last = np.where((cnt[:, -1] >= opt.P1) & (cnt[:, -1] <= opt.P2), last, 0.0)
        assert np.allclose(w.want.price[:, -1], last, rtol=1e-15, atol=0)


def test_deep_draws_differ():
    from oracle import pyoracle
    for prec in wc.PRECS:
        check_deep_draws_differ(lambda seed, first: wr.normals(pyoracle, prec, seed, first, 64, 8))
        # inner streams: subsequence = (path * n_steps + step) * n_inner + j of the deep nested-MC case's first paths
        case = wc.NMC_DEEP
        check_deep_draws_differ(lambda seed, first: wr.normals(
            pyoracle, prec, seed, (first * case.n_steps + 2) * case.n_inner, case.n_inner, case.n_steps - 1))
    # and the deep case's own inner subsequences do not fit 32 bits, nor do its point ids
    assert case.first * case.n_steps > 2 ** 32 and case.first * case.n_steps * case.n_inner > 2 ** 40


def moved(case, prec, form, mutate):
    """kept samples that the mistake moves beyond the tolerance of the GPU test"""
    w = wc.wanted(case, prec, form)
    wrong = wc.restated(case, prec, form, np.float64, mutate)
    return wc.outside(wrong.y.astype(np.float64), w) & w.want.decided


def sum_shift(case, prec, form, mutate):
    """how far the mistake moves the case's sum of samples, relative to the sum: what a sum-level test would see"""
    right, wrong = (wc.restated(case, prec, form, np.float64, m).y.sum() for m in (0, mutate))
    return abs(float(wrong - right)) / float(right)


@pytest.mark.parametrize("prec", wc.PRECS)
def test_mistakes_restated_in_numpy_are_beyond_the_tolerances(oracle, prec):
    """no kernel runs.  Each mistake moves at least one kept sample (or one point without an undecided inner path) of a
    case of tests/test_gpu_window.py by more than the tolerance that test allows.

    The partial last block one step short or long, against the point tolerance tests/test_gpu_parity.py allows in fp32
    (rtol 5e-3, atol 2e-3), on the oracle's rows: of the paying points with a partial last block and no undecided inner
    path that tolerance flags 49 of 49 (short) and 48 of 49 (long) in the edges case, 69 and 66 of 73 in the compaction
    case — it sees a whole step in bulk and lets it pass on the points with many steps to go; the tolerance of this
    module flags every one of them.  On the sum of a price_paths case the same mistake moves 1.2e-3 (33 steps, one step
    long) to 1.0 of the sum in fp32; 2e-3 to 3e-3 is what the sum-level tests allow."""
    nb = wr.PER_BLOCK[prec]
    # 1. the partial last block: every remainder, price_paths and nested MC
    for mutate in (wr.LAST_BLOCK_SHORT, wr.LAST_BLOCK_LONG):
        seen = set()
        for name in ("w-1", "w-2", "w-3", "w-5", "w-6", "w-7", "w-33", "w-61"):
            case = BY[name]
            if case.n_steps % nb:
                seen.add(case.n_steps % nb)
                for form in ("plain", "anti"):
                    n = moved(case, prec, form, mutate).sum()
                    assert n >= 1, (name, form, mutate)
                    print(f"f{prec} {name} {form} mistake {mutate}: {n} samples beyond the tolerance, the sum moves by "
                          f"{sum_shift(case, prec, form, mutate):.1e} of itself")
            else:
                assert not moved(case, prec, "plain", mutate).any()
        assert seen == set(range(1, nb))
        for case in (wc.NMC_EDGES, wc.NMC_COMPACTION):
            St, cnt = wc.oracle_rows(oracle, case, prec)
            w = wc.nmc_wanted(oracle, case, prec, St, cnt)
            wrong = wr.nmc_points(oracle, wc.nmc_option(case), wc.nmc_inner_sim(case, prec), St, cnt, np.float64,
                                  wc.MARGIN, mutate)
            out = wc.nmc_outside(wrong.price, w) & w.free
            partial = (w.want.to_go % nb != 0) & w.free & (w.want.hi > 0)
            assert not (out & ~partial).any()
            for rem in range(1, nb):
                assert (out & (w.want.to_go % nb == rem)).any(), (case.name, rem)
            old = np.abs(wrong.price - w.want.price) > 5e-3 * np.abs(w.want.price) + 2e-3
            print(f"f{prec} {case.name} mistake {mutate}: {partial.sum()} paying points with a partial last block; beyond "
                  f"this module's tolerance {(out & partial).sum()}, beyond rtol 5e-3 + atol 2e-3 {(old & partial).sum()}")
            assert (out & partial).sum() == partial.sum()
    # 2. the window's ends
    for mutate, end in ((wr.P1_STRICT, "P1"), (wr.P2_STRICT, "P2")):
        for name in ("w-3", "w-7", "w-33"):
            case = BY[name]
            hit = moved(case, prec, "plain", mutate)
            at_end = wc.restated(case, prec, "plain", np.float64).members[0].cnt == case.extra[end]
            assert hit.any() and (at_end[hit]).all(), (name, end)
            print(f"f{prec} {name} {end} strict: {hit.sum()} samples beyond the tolerance, the sum moves by "
                  f"{sum_shift(case, prec, 'plain', mutate):.1e} of itself")
    # 3. the twin
    for mutate, names in ((wr.TWIN_DRIFT, ("w-3", "w-7", "nw-3", "nw-7")), (wr.TWIN_SHARES_COUNT, ("w-3", "w-7", "w-33"))):
        for name in names:
            n = moved(BY[name], prec, "anti", mutate).sum()
            assert n > (40 if mutate == wr.TWIN_DRIFT else 0), (name, mutate)
            print(f"f{prec} {name} anti mistake {mutate}: {n} samples beyond the tolerance, the sum moves by "
                  f"{sum_shift(BY[name], prec, 'anti', mutate):.1e} of itself")
    # 4. the control mean of a segment that is not the whole maturity
    for case in (wc.RESTART_CASE, wc.DT_CASE):
        w = wc.wanted(case, prec, "cv")
        wrong = wc.restated(case, prec, "cv", np.float64, wr.CONTROL_MEAN_AT_T)
        assert (np.abs(wrong.c - w.want.c) > w.tol_c).all()
        assert not moved(case, prec, "cv", wr.CONTROL_MEAN_AT_T).any()
    # 5. nested MC
    case = wc.NMC_EDGES
    St, cnt = wc.oracle_rows(oracle, case, prec)
    w = wc.nmc_wanted(oracle, case, prec, St, cnt)
    opt, sim = wc.nmc_option(case), wc.nmc_inner_sim(case, prec)
    for mutate in (wr.COUNT_FROM_ZERO, wr.DISCOUNT_TIME_TO_GO):
        wrong = wr.nmc_points(oracle, opt, sim, St, cnt, np.float64, wc.MARGIN, mutate)
        assert (wc.nmc_outside(wrong.price, w) & w.free).any(), mutate
    wrong = wr.nmc_points(oracle, opt, sim, St, cnt, np.float64, wc.MARGIN, wr.CLOSED_POINT_PRICED)
    assert w.want.closed.any() and (wrong.price[w.want.closed] > 0).any()     # the GPU test asserts == 0 there
    assert np.array_equal(wrong.price[~w.want.closed], w.want.price[~w.want.closed])
    one = [0]
    wrong = wr.nmc_points(oracle, opt, sim, St, cnt, np.float64, wc.MARGIN, wr.SUBSEQUENCE_STRIDED, paths=one)
    out = (wc.nmc_outside(wrong.price, w._replace(want=w.want._replace(lo=w.want.lo[one], hi=w.want.hi[one]), tol=w.tol[one]))
           & w.free[one])
    assert out.sum() >= (w.free[one] & (w.want.to_go[one] > 0) & (w.want.hi[one] > 0)).sum() - 1 and out.any()
