"""CPU tests of the smile calls (mcamd_price_localvol_smile, mcamd_finalize_smile, mcamd_bs_implied_vol_f64): the
declarations and the struct layout, every refusal that needs neither a surface nor a context, the host finalize against
a numpy restatement, the path restatement (tests/localvol_smile_restate.py) against tests/localvol_restate.py, and the
implied volatility.  No device is touched.

The round-trip bound of the implied volatility, 1e-8 relative, is derived, not tuned: at |d1| <= 3 the vega is at least
S0 e^{-qT} sqrt(T) phi(3), so a price wrong by a few ulp moves v by far less: four ulp of the largest term of a price
over that vega floor are at most 1.9e-11 of v on these inputs, whose strikes stay within a factor of ten of the spot
(test_round_trip_inputs_stay_where_the_bound_was_derived asserts all of this on the inputs; the measured worst round
trip is 7.3e-12)."""
import ctypes as C
import importlib
import itertools
import math
import os
import re

import numpy as np
import pytest

import localvol_restate as lv
import localvol_smile_restate as sm

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcamd_price_localvol_smile", "mcamd_price_localvol_smile_enqueue", "mcamd_finalize_smile",
         "mcamd_bs_implied_vol_f64")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


# ---- declarations ----------------------------------------------------------------------------------------------------

def test_header_declares_the_calls_and_the_struct(lib):
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert re.search(r"\}\s*mcamd_smile\s*;", header)
    assert re.search(r"#define\s+MCAMD_SMILE_MAX_STRIKES\s+64\b", header) and capi.SMILE_MAX_STRIKES == 64
    assert re.search(r"#define\s+MCAMD_SMILE_MAX_EXPIRIES\s+32\b", header) and capi.SMILE_MAX_EXPIRIES == 32
    assert re.search(r"#define\s+MCAMD_ABI_VERSION\s+5\b", header) and lib.mcamd_abi_version() == 5
    assert not re.search(r"mcamd_group_\w*smile", header)
    # the discount to the node's own expiry is stated where the price is defined
    assert "OWN expiry" in header and "not over the full T" in header


def test_struct_matches_the_header():
    # static_assert(sizeof(mcamd_smile) == 24) in csrc/capi_smile.cpp
    S = capi.Smile
    assert C.sizeof(S) == 24
    assert (S.payoff.offset, S.n_expiries.offset, S.n_strikes.offset, S.reserved.offset, S.q.offset) == (0, 4, 8, 12, 16)
    s = capi.make_smile(3, 5, capi.PAYOFF_PUT, 0.03)
    assert (s.payoff, s.n_expiries, s.n_strikes, s.reserved, s.q) == (1, 3, 5, 0, 0.03)
    d = capi.make_smile(1, 1)
    assert (d.payoff, d.n_expiries, d.n_strikes, d.reserved, d.q) == (0, 1, 1, 0, 0.0)


# ---- refusals that need neither a surface nor a context -----------------------------------------------------------------

BASE = dict(S0=100.0, K=float("nan"), r=0.1, v=float("nan"), T=1.0)   # v and K are ignored: NaN passes
REF = lambda x: None if x is None else C.byref(x)


def arrays(steps, strikes):
    return (None if steps is None else (C.c_uint32 * max(len(steps), 1))(*steps),
            None if strikes is None else (C.c_double * max(len(strikes), 1))(*strikes))


def price(lib, opt, sim, smile, steps, strikes, stats=True, res=True):
    """both forms with NULL surface and NULL context: ((rc, message) of the synchronous one, then of the enqueue one)"""
    e, k = arrays(steps, strikes)
    h_stats, out = (C.c_double * 8192)(), capi.Result()
    rc = lib.mcamd_price_localvol_smile(None, REF(opt), REF(sim), REF(smile), e, k, None, None,
                                        h_stats if stats else None, C.byref(out) if res else None)
    first = (rc, lib.mcamd_last_error().decode())
    rc = lib.mcamd_price_localvol_smile_enqueue(None, REF(opt), REF(sim), REF(smile), e, k, None, None,
                                                C.c_void_p(64) if stats and res else None)
    return first, (rc, lib.mcamd_last_error().decode())


def refusals():
    O, S, M = capi.make_option, capi.make_sim, capi.make_smile
    opt, sim = O(**BASE), S(1000, 50)
    one, e1, k1 = M(1, 1), [50], [100.0]
    nan, inf = float("nan"), float("inf")
    yield "no opt", (None, sim, one, e1, k1), {}, "non-NULL"
    yield "no sim", (opt, None, one, e1, k1), {}, "non-NULL"
    yield "no smile", (opt, sim, None, e1, k1), {}, "non-NULL"
    yield "no expiry steps", (opt, sim, one, None, k1), {}, "non-NULL"
    yield "no strikes", (opt, sim, one, e1, None), {}, "non-NULL"
    yield "no h_stats", (opt, sim, one, e1, k1), dict(stats=False), "NULL"
    yield "no res", (opt, sim, one, e1, k1), dict(res=False), "NULL"
    for p in (-1, 2):
        yield f"payoff {p}", (opt, sim, M(1, 1, payoff=p), e1, k1), {}, "payoff"
    bad = M(1, 1)
    bad.reserved = 1
    yield "reserved", (opt, sim, bad, e1, k1), {}, "reserved"
    yield "0 expiries", (opt, sim, M(0, 1), [], k1), {}, "n_expiries"
    yield "33 expiries", (opt, sim, M(33, 1), list(range(1, 34)), k1), {}, "n_expiries"
    yield "0 strikes", (opt, sim, M(1, 0), e1, []), {}, "n_strikes"
    yield "65 strikes", (opt, sim, M(1, 65), e1, [100.0] * 65), {}, "n_strikes"
    yield "expiries descend", (opt, sim, M(3, 1), [10, 30, 20], k1), {}, "strictly ascending"
    yield "expiry repeated", (opt, sim, M(3, 1), [10, 20, 20], k1), {}, "strictly ascending"
    yield "expiry 0", (opt, sim, M(2, 1), [0, 20], k1), {}, "strictly ascending"
    yield "expiry beyond n_steps", (opt, sim, M(2, 1), [20, 51], k1), {}, "strictly ascending"
    yield "first expiry beyond n_steps", (opt, sim, M(1, 1), [51], k1), {}, "strictly ascending"
    for K in (nan, inf, -100.0, 0.0):
        yield f"strike {K}", (opt, sim, M(1, 3), e1, [90.0, 100.0, K]), {}, "strike"
    for q in (nan, inf, -inf):
        yield f"q = {q}", (opt, sim, M(1, 1, q=q), e1, k1), {}, "dividend yield"
    yield "use_window", (O(**BASE, use_window=1), sim, one, e1, k1), {}, "window"
    yield "P1", (O(**BASE, P1=1), sim, one, e1, k1), {}, "window"
    yield "P2", (O(**BASE, P2=3), sim, one, e1, k1), {}, "window"
    yield "Ik", (O(**BASE, Ik=2), sim, one, e1, k1), {}, "window"
    yield "Sk", (O(**BASE, Sk=95.0), sim, one, e1, k1), {}, "Sk"
    yield "Tk", (O(**BASE, Tk=5), sim, one, e1, k1), {}, "Tk"
    yield "dt", (O(**BASE, dt=0.01), sim, one, e1, k1), {}, "dt"
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE, capi.FLAG_PRODUCT_FORM,
                  capi.FLAG_LOG_SPACE | capi.FLAG_ANTITHETIC, 32):
        yield f"flags {flags}", (opt, S(1000, 50, flags=flags), one, e1, k1), {}, "flags"
    yield "precision", (opt, S(1000, 50, precision=16), one, e1, k1), {}, "precision"
    yield "n_steps 0", (opt, S(1000, 0), one, e1, k1), {}, "n_steps"
    yield "shard overflow", (opt, S(1 << 63, 50, path_offset=(1 << 64) - 10, n_paths_local=100), one, e1, k1), {}, "overflows"
    yield "exponent range", (O(**dict(BASE, r=1000.0, T=100.0)), sim, one, e1, k1), {}, "exponent range"
    yield "S0 = 0", (O(**dict(BASE, S0=0.0)), sim, one, e1, k1), {}, "S0 > 0"
    yield "T = 0", (O(**dict(BASE, T=0.0)), sim, one, e1, k1), {}, "T > 0"
    yield "r nan", (O(**dict(BASE, r=nan)), sim, one, e1, k1), {}, "finite"


@pytest.mark.parametrize("case", list(refusals()), ids=lambda c: c[0])
def test_refusals_before_the_surface_and_the_context_are_looked_at(lib, case):
    _, args, kw, words = case
    for rc, msg in price(lib, *args, **kw):
        assert rc == capi.ERR_INVALID and words in msg, msg


@pytest.mark.parametrize("payoff", [capi.PAYOFF_CALL, capi.PAYOFF_PUT])
@pytest.mark.parametrize("flags,prec", [(0, capi.F64), (capi.FLAG_LOG_SPACE, capi.F32)])
@pytest.mark.parametrize("steps,strikes", [([50], [100.0]), ([1, 2, 49], [1e-3, 100.0, 1e6]),
                                           (list(range(1, 33)), [50.0 + k for k in range(64)])])
def test_accepted_requests_reach_the_missing_surface(lib, payoff, flags, prec, steps, strikes):
    """everything the request alone decides has passed when the missing surface is named; opt->v and opt->K are ignored"""
    for v, K in ((0.0, 0.0), (-1.0, -5.0), (float("nan"), float("nan"))):
        opt = capi.make_option(**dict(BASE, v=v, K=K))
        sim = capi.make_sim(1000, 50, prec, flags=flags, path_offset=3, n_paths_local=0)
        for rc, msg in price(lib, opt, sim, capi.make_smile(len(steps), len(strikes), payoff, 0.03), steps, strikes):
            assert rc == capi.ERR_INVALID and "surface" in msg and "non-NULL" in msg, msg


def test_python_arrays_must_match_the_smile():
    with pytest.raises(ValueError):
        capi._smile_arrays(capi.make_smile(2, 3), [1, 2, 3], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        capi._smile_arrays(capi.make_smile(2, 3), [1, 2], [1.0, 2.0])


# ---- mcamd_finalize_smile ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_e,n_K,n", [(1, 1, 1000), (3, 5, 77_777), (32, 64, 1 << 20), (2, 2, 1), (2, 2, 2)])
def test_finalize_against_the_restatement(lib, n_e, n_K, n):
    rng = np.random.default_rng(5)
    mean = rng.uniform(0.0, 30.0, n_e * n_K)
    mean[0] = 0.0
    std = rng.uniform(0.5, 20.0, n_e * n_K) * (mean > 0)
    stats = np.concatenate([n * mean, n * (mean * mean) + (n - 1) * std * std])
    r, T, n_steps = 0.07, 2.5, 252
    steps = sorted(rng.choice(np.arange(1, n_steps + 1), n_e, replace=False).tolist())
    opt = capi.make_option(**dict(BASE, r=r, T=T))
    price, se = capi.finalize_smile(stats, n, opt, n_steps, capi.make_smile(n_e, n_K), steps)
    want_price, want_se = sm.finalize(stats, n, r, T, n_steps, steps, n_K)
    assert price.shape == se.shape == (n_e, n_K)
    assert np.allclose(price, want_price, rtol=1e-14, atol=0) and np.allclose(se, want_se, rtol=1e-9, atol=1e-300)
    # each node is discounted to its own expiry, not over T: one node through mcamd_finalize with t_m
    for m, k in ((0, 0), (n_e - 1, n_K - 1)):
        one = capi.finalize(stats[m * n_K + k], stats[n_e * n_K + m * n_K + k], n, r, steps[m] * (T / n_steps))
        assert (price[m, k], se[m, k]) == (one.price, one.std_err)
    if n_e > 1 and steps[0] < n_steps:
        full = capi.finalize(stats[1], stats[n_e * n_K + 1], n, r, T)
        assert n_K == 1 or price[0, 1] > full.price > 0
    assert price[0, 0] == 0.0 and se[0, 0] == 0.0


def test_finalize_refusals(lib):
    opt, smile = capi.make_option(**BASE), capi.make_smile(1, 1)
    stats, steps, out = (C.c_double * 2)(1.0, 2.0), (C.c_uint32 * 1)(5), (C.c_double * 1)()
    fn = lib.mcamd_finalize_smile
    assert fn(stats, 10, C.byref(opt), 10, C.byref(smile), steps, out, out) == capi.OK
    assert fn(None, 10, C.byref(opt), 10, C.byref(smile), steps, out, out) == capi.ERR_INVALID
    assert fn(stats, 10, None, 10, C.byref(smile), steps, out, out) == capi.ERR_INVALID
    assert fn(stats, 10, C.byref(opt), 10, None, steps, out, out) == capi.ERR_INVALID
    assert fn(stats, 10, C.byref(opt), 10, C.byref(smile), None, out, out) == capi.ERR_INVALID
    assert fn(stats, 10, C.byref(opt), 10, C.byref(smile), steps, None, out) == capi.ERR_INVALID
    assert fn(stats, 10, C.byref(opt), 10, C.byref(smile), steps, out, None) == capi.ERR_INVALID
    assert fn(stats, 10, C.byref(opt), 0, C.byref(smile), steps, out, out) == capi.ERR_INVALID
    for bad in (capi.make_smile(0, 1), capi.make_smile(33, 1), capi.make_smile(1, 0), capi.make_smile(1, 65)):
        assert fn(stats, 10, C.byref(opt), 10, C.byref(bad), steps, out, out) == capi.ERR_INVALID


# ---- the restatement --------------------------------------------------------------------------------------------------

def skew(n_t, n_x, x_min, x_max):
    x = np.linspace(x_min, x_max, n_x)
    return np.array([(0.18 + 0.04 * j) * (1.0 + 0.5 * np.exp(-x)) / 1.5 for j in range(n_t)])


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.longdouble])
def test_the_last_step_is_the_pricer_restatement(dtype):
    """the inputs of tests/test_localvol_cpu.py::test_restatement_precisions_agree: at expiry n_steps the spots are
    S_T of localvol_restate.samples without a barrier, bit for bit, and the node samples are its h"""
    grid = (4, 65, -1.5, 1.5)
    sigma = skew(*grid)
    z = np.random.default_rng(3).standard_normal((50, 5000)).astype(np.float32).astype(np.float64)
    S = sm.spots(z, 100.0, 1.0, 0.1, 0.03, grid, sigma, 50, (1, 17, 50), dtype)
    for payoff in (lv.CALL, lv.PUT):
        want = lv.samples(z, 100.0, 100.0, 92.0, 1.0, 0.1, 0.03, grid, sigma, lv.NO_BARRIER, payoff, lv.DISCRETE, dtype)
        assert S.dtype == want["S_T"].dtype and np.array_equal(S[2], want["S_T"])
        h = sm.samples(S, [90.0, 100.0], payoff)
        assert np.array_equal(h[2, 1], want["h"]) and (h[2, 0] != h[2, 1]).any()
        total, totsq, paying = sm.node_sums(S, [90.0, 100.0], payoff)
        assert total[2, 1] == pytest.approx(float(want["y"].sum()), rel=1e-13)
    # an inner expiry is the same walk stopped early: rows and dt still run against the 50 steps
    inner = sm.spots(z[:17], 100.0, 1.0, 0.1, 0.03, grid, sigma, 50, (1, 17), dtype)
    assert np.array_equal(inner, S[:2])
    assert not np.array_equal(sm.spots(z, 100.0, 1.0, 0.1, 0.03, grid, sigma, 50, (17,), dtype, sm.LATE_EXPIRY)[0], S[1])


# ---- mcamd_bs_implied_vol_f64 -------------------------------------------------------------------------------------------

S0 = 100.0
VOLS, TIMES, RATES, D1S = (0.05, 0.2, 0.6, 1.5), (1.0 / 52.0, 1.0, 5.0), (0.0, 0.1, 0.03), (-2.999, -1.5, 0.0, 1.5, 2.999)


def strike_at(d1, v, T, r, q):
    return S0 * math.exp(-d1 * v * math.sqrt(T) + (r - q + 0.5 * v * v) * T)


# strikes at those d1, kept where they lie within a factor of ten of the spot: beyond that the price itself (a put's, of
# the size of K) has ulps that the vega floor no longer covers, and no smile is quoted there
ROUND_TRIP = [(v, T, r, q, K) for v, T, r, q, d1 in itertools.product(VOLS, TIMES, RATES, RATES, D1S)
              for K in (strike_at(d1, v, T, r, q),) if S0 / 10.0 <= K <= 10.0 * S0]


def bounds(K, T, r, q, payoff):
    D, F = math.exp(-r * T), S0 * math.exp((r - q) * T)
    lower = D * max(F - K if payoff == capi.PAYOFF_CALL else K - F, 0.0)
    return lower, (S0 * math.exp(-q * T) if payoff == capi.PAYOFF_CALL else K * D)


def test_round_trip_inputs_stay_where_the_bound_was_derived():
    """|d1| <= 3 on every input, hence vega >= S0 e^{-qT} sqrt(T) phi(3); four ulp of the price (or of the spot or the
    strike, which its terms are the size of) over that vega stay under a tenth of 1e-8 v.  Every (v, T, r, q) keeps a
    strike, and both wings are there."""
    assert {c[:4] for c in ROUND_TRIP} == set(itertools.product(VOLS, TIMES, RATES, RATES)) and len(ROUND_TRIP) > 400
    assert min(c[4] for c in ROUND_TRIP) < 0.2 * S0 and max(c[4] for c in ROUND_TRIP) > 5.0 * S0
    worst = 0.0
    for v, T, r, q, K in ROUND_TRIP:
        d1 = (math.log(S0 / K) + (r - q + 0.5 * v * v) * T) / (v * math.sqrt(T))
        assert abs(d1) <= 3.0
        vega_floor = S0 * math.exp(-q * T) * math.sqrt(T) * math.exp(-4.5) / math.sqrt(2.0 * math.pi)
        for payoff in (capi.PAYOFF_CALL, capi.PAYOFF_PUT):
            p = capi.bs_price_f64(S0, K, T, r, q, v, payoff)
            worst = max(worst, 4.0 * np.spacing(max(p, S0, K)) / vega_floor / v)
    print(f"4 ulp of the price (or of S0) over the vega floor, relative to v: at most {worst:.2e}")
    assert worst < 1e-9


@pytest.mark.parametrize("payoff", [capi.PAYOFF_CALL, capi.PAYOFF_PUT])
def test_implied_vol_round_trip(lib, payoff):
    worst = 0.0
    for v, T, r, q, K in ROUND_TRIP:
        p = capi.bs_price_f64(S0, K, T, r, q, v, payoff)
        lower, upper = bounds(K, T, r, q, payoff)
        assert lower < p < upper
        got = capi.bs_implied_vol(S0, K, T, r, q, p, payoff)
        worst = max(worst, abs(got - v) / v)
        assert abs(got - v) <= 1e-8 * v, (v, T, r, q, K, got)
    print(f"payoff {payoff}: worst relative round-trip error {worst:.2e} over {len(ROUND_TRIP)} inputs")


@pytest.mark.parametrize("payoff", [capi.PAYOFF_CALL, capi.PAYOFF_PUT])
@pytest.mark.parametrize("K,T,r,q", [(80.0, 1.0, 0.1, 0.03), (125.0, 1.0, 0.1, 0.03), (100.0, 5.0, 0.0, 0.0),
                                     (100.0 * math.exp(0.07 / 52.0), 1.0 / 52.0, 0.1, 0.03)])
def test_implied_vol_refuses_the_bounds_and_ends_just_inside_them(lib, payoff, K, T, r, q):
    lower, upper = bounds(K, T, r, q, payoff)
    vol = C.c_double(7.0)
    fn = lib.mcamd_bs_implied_vol_f64
    for p in (lower, upper, np.nextafter(lower, -np.inf), np.nextafter(upper, np.inf), -1.0, 2.0 * upper, float("nan"),
              float("inf")):
        vol.value = 7.0
        assert fn(S0, K, T, r, q, payoff, float(p), C.byref(vol)) == capi.ERR_INVALID, p
        assert math.isnan(vol.value)
    # one ulp inside either bound: admissible, and the iteration ends (its count is capped)
    for p in (np.nextafter(lower, np.inf), np.nextafter(upper, -np.inf)):
        assert fn(S0, K, T, r, q, payoff, float(p), C.byref(vol)) == capi.OK, p
        assert vol.value >= 0.0 and math.isfinite(vol.value)
    # in between, the answer reprices
    mid = 0.5 * (lower + upper)
    got = capi.bs_implied_vol(S0, K, T, r, q, mid, payoff)
    assert capi.bs_price_f64(S0, K, T, r, q, got, payoff) == pytest.approx(mid, rel=1e-12)


def test_implied_vol_refuses_bad_arguments(lib):
    vol = C.c_double(0)
    fn, nan, inf = lib.mcamd_bs_implied_vol_f64, float("nan"), float("inf")
    ok = [S0, 100.0, 1.0, 0.1, 0.03, capi.PAYOFF_CALL, 10.0]
    assert fn(*ok, C.byref(vol)) == capi.OK and 0.1 < vol.value < 0.5
    assert fn(*ok, None) == capi.ERR_INVALID
    for where, bads in ((0, (0.0, -1.0, nan, inf)), (1, (0.0, -1.0, nan, inf)), (2, (0.0, -1.0, nan, inf)),
                        (3, (nan, inf)), (4, (nan, -inf)), (5, (-1, 2)), (6, (nan, inf))):
        for bad in bads:
            args = list(ok)
            args[where] = bad
            vol.value = 1.0
            assert fn(*args, C.byref(vol)) == capi.ERR_INVALID and math.isnan(vol.value), (where, bad)


def test_implied_vols_maps_and_never_raises(lib):
    strikes, times = [80.0, 100.0, 125.0], [0.5, 1.0]
    prices = np.array([[capi.bs_price_f64(S0, K, t, 0.1, 0.03, 0.2 + 0.1 * m) for K in strikes] for m, t in enumerate(times)])
    vols = capi.implied_vols(S0, strikes, times, 0.1, 0.03, prices)
    assert vols.shape == (2, 3) and np.allclose(vols, [[0.2] * 3, [0.3] * 3], rtol=1e-8, atol=0)
    prices[0, 1], prices[1, 2] = 0.0, 1e9
    vols = capi.implied_vols(S0, strikes, times, 0.1, 0.03, prices)
    assert np.isnan(vols[0, 1]) and np.isnan(vols[1, 2]) and np.isfinite(vols).sum() == 4
