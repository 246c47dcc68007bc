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
