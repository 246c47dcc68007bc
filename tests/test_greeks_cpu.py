"""CPU-only checks of the Greeks entry points (include/mcamd.h, mcamd_*greeks*): the closed form against finite
differences of the closed-form price, the host finalization against numpy, the struct layout, and the refusals that
need no device.  No kernels are launched here."""
import ctypes as C
import importlib
import itertools
import math
import os

import numpy as np
import pytest

import greeks_cases as gc
import greeks_restate as gr
from deep_inputs import check_deep_draws_differ

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


GRID = list(itertools.product((80.0, 100.0, 125.0), (90.0, 110.0), (0.1, 1.0, 2.5), (0.0, 0.05), (0.15, 0.4)))


@pytest.mark.parametrize("S0,K,T,r,v", GRID)
def test_bs_greeks_match_central_differences_of_the_price(lib, S0, K, T, r, v):
    price = capi.bs_call_f64
    got = capi.bs_greeks_f64(S0, K, T, r, v)

    def d1(f, x, h):   # five-point central differences: truncation O(h^4)
        return (-f(x + 2 * h) + 8 * f(x + h) - 8 * f(x - h) + f(x - 2 * h)) / (12 * h)

    def d2(f, x, h):
        return (-f(x + 2 * h) + 16 * f(x + h) - 30 * f(x) + 16 * f(x - h) - f(x - 2 * h)) / (12 * h * h)

    want = [
        price(S0, K, T, r, v),
        d1(lambda s: price(s, K, T, r, v), S0, 1e-3 * S0),
        d2(lambda s: price(s, K, T, r, v), S0, 2e-3 * S0),
        d1(lambda x: price(S0, K, T, r, x), v, 1e-3),
        d1(lambda x: price(S0, K, T, x, v), r, 1e-3),
        -d1(lambda t: price(S0, K, t, r, v), T, 1e-3 * T),   # theta = -dV/dT
    ]
    p0 = want[0]
    # second differences lose ~eps * price / h^2 to rounding: an absolute allowance on gamma
    atol = [1e-12, 1e-9, 1e-7, 1e-8, 1e-8, 1e-8]
    for i, name in enumerate(capi.GREEK_NAMES):
        assert math.isclose(got[i], want[i], rel_tol=1e-6, abs_tol=atol[i]), (name, got[i], want[i])
    assert got[0] == p0 and 0.0 < got[1] < 1.0 and got[2] > 0.0 and got[3] > 0.0 and got[4] > 0.0


def test_bs_greeks_known_values(lib):
    # the benchmark option (S0 = K = 100, T = 1, r = 0.1, v = 0.2): d1 = 0.6, d2 = 0.4, restated with math
    N = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))
    phi = math.exp(-0.18) / math.sqrt(2.0 * math.pi)
    Kd = 100.0 * math.exp(-0.1)
    want = [100.0 * N(0.6) - Kd * N(0.4), N(0.6), phi / 20.0, 100.0 * phi, Kd * N(0.4), -10.0 * phi - 0.1 * Kd * N(0.4)]
    got = capi.bs_greeks_f64(100.0, 100.0, 1.0, 0.1, 0.2)
    np.testing.assert_allclose(got, want, rtol=1e-13)
    assert math.isclose(got[0], 13.269676584660893, rel_tol=1e-13)


def test_finalize_greeks_stats_matches_numpy(lib):
    rng = np.random.default_rng(7)
    n, r, T = 12_345, 0.07, 1.5
    q = rng.normal(size=(n, 6)) * np.array([10.0, 0.5, 0.02, 30.0, 50.0, 8.0]) + np.array([12, 0.6, 0.02, 35, 55, -9])
    stats = np.zeros(16)
    stats[0:12:2] = q.sum(axis=0)
    stats[1:12:2] = (q * q).sum(axis=0)
    stats[12] = n
    g = capi.finalize_greeks_stats(stats, r, T, theta_defined=True)
    D = math.exp(-r * T)
    assert g.n == n and g.method == 0 and g.grid == 0
    np.testing.assert_allclose(list(g.value), D * q.mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(list(g.std_err), D * q.std(axis=0, ddof=1) / math.sqrt(n), rtol=1e-8)
    np.testing.assert_array_equal(list(g.sum), stats[0:12:2])
    np.testing.assert_array_equal(list(g.sumsq), stats[1:12:2])
    h = capi.finalize_greeks_stats(stats, r, T, theta_defined=False)
    assert math.isnan(h.value[capi.GREEK_THETA]) and math.isnan(h.std_err[capi.GREEK_THETA])
    assert list(h.value)[:5] == list(g.value)[:5] and h.sum[capi.GREEK_THETA] == g.sum[capi.GREEK_THETA]
    # an empty record: zeros (and no division by zero)
    z = capi.finalize_greeks_stats(np.zeros(16), r, T)
    assert z.n == 0 and list(z.value) == [0.0] * 6 and list(z.std_err) == [0.0] * 6


def test_greeks_struct_size_matches_the_header(lib):
    # static_assert(sizeof(mcamd_greeks) == 224) in csrc/capi.cpp
    assert C.sizeof(capi.Greeks) == 224
    assert capi.Greeks.n.offset == 192 and capi.Greeks.method.offset == 200 and capi.Greeks.block.offset == 216


def test_greeks_refusals_without_a_device(lib):
    opt, bullet = capi.make_option(), capi.make_option(B=120.0, P1=10, P2=50, use_window=1)
    sim = capi.make_sim(1000, 12)
    out = capi.Greeks()
    L = lib
    assert L.mcamd_price_greeks(None, C.byref(opt), C.byref(sim), capi.GREEKS_AUTO, C.byref(out)) == capi.ERR_INVALID
    assert L.mcamd_price_greeks(None, C.byref(opt), C.byref(sim), capi.GREEKS_AUTO, None) == capi.ERR_INVALID
    assert L.mcamd_price_greeks(None, None, C.byref(sim), capi.GREEKS_AUTO, C.byref(out)) == capi.ERR_INVALID
    assert L.mcamd_price_greeks_enqueue(None, C.byref(opt), None, capi.GREEKS_AUTO, None) == capi.ERR_INVALID
    assert L.mcamd_group_price_greeks(None, C.byref(opt), C.byref(sim), capi.GREEKS_AUTO, C.byref(out)) == capi.ERR_INVALID
    assert L.mcamd_finalize_greeks_stats(None, 0.1, 1.0, 1, C.byref(out)) == capi.ERR_INVALID
    assert L.mcamd_finalize_greeks_stats((C.c_double * 16)(), 0.1, 1.0, 1, None) == capi.ERR_INVALID
    assert L.mcamd_bs_greeks_f64(100.0, 100.0, 1.0, 0.1, 0.2, None) == capi.ERR_INVALID
    for bad in ((0.0, 100.0, 1.0, 0.1, 0.2), (100.0, 100.0, 0.0, 0.1, 0.2), (100.0, 100.0, 1.0, 0.1, 0.0)):
        assert L.mcamd_bs_greeks_f64(*bad, (C.c_double * 6)()) == capi.ERR_INVALID
    # refused by the request alone, before any device is looked at
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_PRODUCT_FORM, capi.FLAG_SEPARATE_REDUCE,
                  capi.FLAG_LOG_SPACE | capi.FLAG_ANTITHETIC):
        s = capi.make_sim(1000, 12, flags=flags)
        assert L.mcamd_price_greeks(None, C.byref(opt), C.byref(s), capi.GREEKS_AUTO, C.byref(out)) == capi.ERR_INVALID
        assert b"flags" in L.mcamd_last_error()
        assert L.mcamd_price_greeks_enqueue(None, C.byref(opt), C.byref(s), capi.GREEKS_AUTO, None) == capi.ERR_INVALID
    assert L.mcamd_price_greeks(None, C.byref(bullet), C.byref(sim), capi.GREEKS_PATHWISE, C.byref(out)) == capi.ERR_INVALID
    assert b"pathwise" in L.mcamd_last_error()
    for method in (3, -1):
        assert L.mcamd_price_greeks(None, C.byref(opt), C.byref(sim), method, C.byref(out)) == capi.ERR_INVALID
        assert b"method" in L.mcamd_last_error()
    flat = capi.make_option(v=0.0)
    assert L.mcamd_price_greeks(None, C.byref(flat), C.byref(sim), capi.GREEKS_AUTO, C.byref(out)) == capi.ERR_INVALID
    assert b"v > 0" in L.mcamd_last_error()
    # the accepted flags pass these checks and stop at the missing context
    s = capi.make_sim(1000, 12, flags=capi.FLAG_LOG_SPACE)
    assert L.mcamd_price_greeks(None, C.byref(opt), C.byref(s), capi.GREEKS_PATHWISE, C.byref(out)) == capi.ERR_INVALID
    assert b"ctx" in L.mcamd_last_error()


# ---- the per-path inputs of tests/test_gpu_greeks.py (tests/greeks_cases.py): what their tolerance and their guards rest on --------


def test_restatement_spreads():
    """prints what the per-path tolerances are made of: per method, precision and estimator, the largest elementwise
    difference between the two restatements over the method's cases (greeks_cases.spreads)"""
    for method, name in ((gc.PW, "pathwise"), (gc.LR, "likelihood ratio")):
        for prec in gc.PRECS:
            s = gc.spreads(prec, method)
            print(f"{name} prec {prec}: " + "  ".join(f"{n} {x:.3e}" for n, x in zip(capi.GREEK_NAMES, s)))
            live = 6 if method == gc.PW else 5     # there is no LR theta
            assert (s[:live] > 0).all() and (s[live:] == 0).all()
            # the spread is rounding, not a flipped indicator: far below the estimator's own size in every case
            mean = np.min([np.abs(gc.wanted(c, prec)[0]).mean(axis=0) for c in gc.CASES if c.method == method], axis=0)
            assert (s[:5] < (1e-11 if prec == capi.F64 else 1e-4) * mean[:5]).all(), (s, mean)


def test_inputs_keep_clear_of_the_jumps():
    """the conditions under which a path may be left out, on the final case list: in fp32 at most MAX_LEFT_OUT of a case's
    paths lie within NEAR of a jump, in fp64 (where nothing is left out) every path is 1e-6 or more away — 10^8 times the
    rounding of an fp64 exponent — and both restatements of a precision agree on which of the compared paths pay.  The
    shards of the small-shard test are sums and can leave nothing out: none of their paths is near a jump."""
    for case in gc.CASES + gc.SHARD_CASES:
        n = gc.N_PATHS if case in gc.CASES else max(gc.shard_sizes(case))
        opt = gc.option(case)
        for prec in gc.PRECS:
            r = gc.restated(case, prec, np.float64, n)
            out = gc.left_out(case, prec, n).any(axis=1)
            to_strike = np.abs(r.S_T / opt.K - 1.0).min()
            to_barrier = np.abs(r.logs - math.log(opt.B / (opt.Sk or opt.S0))).min() if opt.use_window else math.inf
            print(f"{case.name} prec {prec}: left out {out.sum()} of {n}, closest S_T / K - 1 {to_strike:.2e}, "
                  f"closest ln(S_t / B) {to_barrier:.2e}, paying {(r.q[:, 0] != 0).mean():.3f}")
            assert out.sum() <= (gc.MAX_LEFT_OUT if case in gc.CASES else 0), case.name
            if prec == capi.F64:
                assert not out.any() and (case.method == gc.LR or to_strike > 1e-6) and to_barrier > 1e-6
            a, b = gc.restated(case, prec, gc.OWN[prec], n), gc.restated(case, prec, gc.OTHER[prec], n)
            assert ((a.q[:, 0] != 0) == (b.q[:, 0] != 0))[~out].all(), case.name
            if case.method == gc.PW:
                assert ((a.S_T > opt.K) == (b.S_T > opt.K))[~out].all(), case.name


def test_window_cases_pay_on_some_paths_and_not_on_others():
    """not a vacuous window: the restated payoff is non-zero on a fifth of the paths or more and zero on a fifth or more,
    and the window, not the strike alone, decides on some (but for the restart from 93.5, whose window shuts on no path:
    the case after it restarts from 110 with a window that shuts at both ends)"""
    for case in gc.WINDOW_CASES:
        opt = gc.option(case)
        for prec in gc.PRECS:
            r = gc.restated(case, prec, np.float64)
            paying = (r.q[:, 0] != 0).mean()
            shut = ((r.S_T > opt.K) & (r.q[:, 0] == 0)).mean()
            print(f"{case.name} prec {prec}: paying {paying:.3f}, in the money but outside the window {shut:.3f}")
            assert 0.2 <= paying <= 0.8 and (shut > 0.05 or case is gc.ALWAYS_OPEN), (case.name, prec, paying, shut)


@pytest.mark.parametrize("prec", gc.PRECS)
def test_deep_draws_are_those_of_neither_shallow_word(oracle, prec):
    """What makes the deep cases worth running: the deep normals share nothing with the streams a dropped high word of
    the path id or of the seed lands on (tests/deep_inputs.py)."""
    check_deep_draws_differ(lambda seed, first: gr.normals(oracle, prec, seed, range(first, first + 64), 7))


def test_one_path_shards_restate_the_shard(oracle):
    """restate() of a shard is restate() of its paths one by one: a path's samples depend on its global id alone"""
    case = gc.WINDOW_CASES[-1]
    whole = gc.restated(case, capi.F32, np.float64, 5)
    for i in range(5):
        one = gr.restate(oracle, gc.option(case), gc.sim(case, capi.F32, first=case.where[1] + i, n_local=1), case.method)
        assert np.array_equal(one.q[0], whole.q[i]) and one.S_T[0] == whole.S_T[i] and one.count[0] == whole.count[i]
