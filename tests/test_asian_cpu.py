"""CPU-only checks of the Asian entry points (include/mcamd.h, mcamd_price_asian): declarations and struct layout,
every refusal that depends on the request alone — each happens before the context is looked at, so ctx = NULL reaches
them — the host closed form against an independent restatement, the numpy restatement of the estimator against the
closed form, and the records in tests/asian_restate.py that the GPU tests take their tolerances from.  No kernels run
here."""
import ctypes as C
import importlib
import itertools
import math
import os
import re

import numpy as np
import pytest

import asian_restate as ar
from deep_inputs import check_deep_draws_differ

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


NAMES = ("mcamd_price_asian", "mcamd_price_asian_enqueue", "mcamd_asian_geometric_price_f64")


def test_header_declares_the_calls_and_the_struct(lib):
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert re.search(r"\}\s*mcamd_asian\s*;", header)
    for name, value in (("ASIAN_ARITHMETIC", 0), ("ASIAN_GEOMETRIC", 1), ("ASIAN_FIXED", 0), ("ASIAN_FLOATING", 1),
                        ("ASIAN_CONTROL_NONE", 0), ("ASIAN_CONTROL_GEOMETRIC", 1)):
        assert re.search(r"#define\s+MCAMD_" + name + r"\s+" + str(value) + r"\b", header), name
        assert getattr(capi, name) == value
    assert (capi.ASIAN_ARITHMETIC, capi.ASIAN_GEOMETRIC, capi.ASIAN_FIXED, capi.ASIAN_FLOATING, capi.PAYOFF_CALL,
            capi.PAYOFF_PUT) == (ar.ARITHMETIC, ar.GEOMETRIC, ar.FIXED, ar.FLOATING, ar.CALL, ar.PUT)
    assert re.search(r"#define\s+MCAMD_ABI_VERSION\s+5\b", header) and lib.mcamd_abi_version() == 5
    assert "first carried by the build that ships csrc/asian.hip" in header
    assert not re.search(r"mcamd_group_\w*asian", header)


def test_struct_matches_the_header():
    # static_assert(sizeof(mcamd_asian) == 24) in csrc/capi_pathdep.cpp
    A = capi.Asian
    assert C.sizeof(A) == 24
    assert (A.average.offset, A.strike.offset, A.payoff.offset, A.include_spot.offset, A.control.offset,
            A.reserved.offset) == (0, 4, 8, 12, 16, 20)
    a = capi.make_asian(capi.ASIAN_GEOMETRIC, capi.ASIAN_FLOATING, capi.PAYOFF_PUT, 1)
    assert (a.average, a.strike, a.payoff, a.include_spot, a.control, a.reserved) == (1, 1, 1, 1, 0, 0)
    d = capi.make_asian(control=capi.ASIAN_CONTROL_GEOMETRIC)
    assert (d.average, d.strike, d.payoff, d.include_spot, d.control, d.reserved) == (0, 0, 0, 0, 1, 0)


# ---- refusals ------------------------------------------------------------------------------------------------------

def price(lib, opt, sim, asian, res=True, ctx=None):
    out = capi.Result()
    ref = lambda x: None if x is None else C.byref(x)
    rc = lib.mcamd_price_asian(ctx, ref(opt), ref(sim), ref(asian), None, C.byref(out) if res else None)
    return rc, lib.mcamd_last_error().decode()


BASE = dict(ar.BASE, K=ar.K_ATM)


def refusals():
    O, S, A = capi.make_option, capi.make_sim, capi.make_asian
    opt, sim, asian = O(**BASE), S(1000, 50), A()
    floating = A(strike=capi.ASIAN_FLOATING)
    yield "no opt", (None, sim, asian), {}, "non-NULL"
    yield "no sim", (opt, None, asian), {}, "non-NULL"
    yield "no asian", (opt, sim, None), {}, "non-NULL"
    yield "no res", (opt, sim, asian), dict(res=False), "non-NULL"
    for k in (-1, 2):
        yield f"average {k}", (opt, sim, A(average=k)), {}, "average"
        yield f"strike {k}", (opt, sim, A(strike=k)), {}, "strike"
        yield f"payoff {k}", (opt, sim, A(payoff=k)), {}, "payoff"
        yield f"include_spot {k}", (opt, sim, A(include_spot=k)), {}, "include_spot"
        yield f"control {k}", (opt, sim, A(control=k)), {}, "control"
    bad = A()
    bad.reserved = 1
    yield "reserved", (opt, sim, bad), {}, "reserved"
    yield "control on a geometric job", (opt, sim, A(capi.ASIAN_GEOMETRIC, control=capi.ASIAN_CONTROL_GEOMETRIC)), {}, \
        "arithmetic jobs only"
    for K in (0.0, -90.0, float("nan"), float("inf")):
        yield f"fixed, K = {K}", (O(**dict(BASE, K=K)), sim, asian), {}, "finite K > 0"
    for who, a in (("fixed", asian), ("floating", floating)):
        yield f"{who} use_window", (O(**BASE, use_window=1), sim, a), {}, "window"
        yield f"{who} P1", (O(**BASE, P1=1), sim, a), {}, "window"
        yield f"{who} P2", (O(**BASE, P2=3), sim, a), {}, "window"
        yield f"{who} Ik", (O(**BASE, Ik=2), sim, a), {}, "window"
        yield f"{who} Sk", (O(**BASE, Sk=95.0), sim, a), {}, "Sk"
        yield f"{who} Tk", (O(**BASE, Tk=5), sim, a), {}, "Tk"
        yield f"{who} dt", (O(**BASE, dt=0.01), sim, a), {}, "dt"
        yield f"{who} v = 0", (O(**dict(BASE, v=0.0)), sim, a), {}, "v > 0"
        yield f"{who} v < 0", (O(**dict(BASE, v=-0.2)), sim, a), {}, "v > 0"
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE, capi.FLAG_PRODUCT_FORM,
                  capi.FLAG_LOG_SPACE | capi.FLAG_ANTITHETIC, capi.FLAG_LOG_SPACE | capi.FLAG_PRODUCT_FORM, 32):
        yield f"flags {flags}", (opt, S(1000, 50, flags=flags), asian), {}, "flags"
    # what mcamd_price_paths refuses on sim
    yield "precision", (opt, S(1000, 50, precision=16), asian), {}, "precision"
    yield "n_steps 0", (opt, S(1000, 0), asian), {}, "n_steps"
    yield "shard overflow", (opt, S(1 << 63, 50, path_offset=(1 << 64) - 10, n_paths_local=100), asian), {}, "overflows"
    yield "exponent range", (O(**dict(BASE, v=100.0, T=100.0)), S(1000, 50), asian), {}, "exponent range"
    yield "T = 0", (O(**dict(BASE, T=0.0)), sim, asian), {}, "T > 0"
    # the control's mean is a closed form of S0
    yield "controlled, S0 = 0", (O(**dict(BASE, S0=0.0)), sim, A(control=capi.ASIAN_CONTROL_GEOMETRIC)), {}, "S0"


@pytest.mark.parametrize("case", list(refusals()), ids=lambda c: c[0])
def test_refusals_before_the_context_is_looked_at(lib, case):
    _, args, kw, words = case
    rc, msg = price(lib, *args, **kw)
    assert rc == capi.ERR_INVALID and words in msg, msg
    if kw.get("res", True):   # the enqueue form shares the checks
        ref = lambda x: None if x is None else C.byref(x)
        rc = lib.mcamd_price_asian_enqueue(None, ref(args[0]), ref(args[1]), ref(args[2]), None, None)
        assert rc == capi.ERR_INVALID and words in lib.mcamd_last_error().decode()


@pytest.mark.parametrize("average,control", [(0, 0), (0, 1), (1, 0)])
@pytest.mark.parametrize("strike,payoff,spot", ar.PRODUCTS)
@pytest.mark.parametrize("flags,prec", [(0, capi.F64), (capi.FLAG_LOG_SPACE, capi.F32)])
def test_accepted_requests_reach_the_missing_context(lib, average, control, strike, payoff, spot, flags, prec):
    sim = capi.make_sim(1000, 50, prec, flags=flags, path_offset=3, n_paths_local=0)
    rc, msg = price(lib, capi.make_option(**BASE), sim, capi.make_asian(average, strike, payoff, spot, control))
    assert rc == capi.ERR_INVALID and "ctx" in msg, msg


def test_a_floating_strike_ignores_K_and_every_asian_ignores_B(lib):
    sim = capi.make_sim(1000, 50, n_paths_local=0)
    for K, control in itertools.product((0.0, -5.0, float("nan")), (0, 1)):
        rc, msg = price(lib, capi.make_option(**dict(BASE, K=K, B=-3.0)), sim,
                        capi.make_asian(strike=capi.ASIAN_FLOATING, control=control))
        assert rc == capi.ERR_INVALID and "ctx" in msg, msg
    rc, msg = price(lib, capi.make_option(**dict(BASE, B=float("nan"))), sim, capi.make_asian())
    assert rc == capi.ERR_INVALID and "ctx" in msg, msg


# ---- the closed form -----------------------------------------------------------------------------------------------

P = dict(S0=100.0, T=1.0, r=0.1, v=0.2)
CLOSED_STEPS = (1, 2, 12, 252)


@pytest.mark.parametrize("n_steps", CLOSED_STEPS)
def test_closed_form_against_the_restatement(lib, n_steps):
    """1e-12 relative, all eight strike x payoff x include_spot cases"""
    for (strike, payoff, spot), K in itertools.product(ar.PRODUCTS, (90.0, 100.0, 110.0)):
        got = capi.asian_geometric_price_f64(P["S0"], K, P["T"], P["r"], P["v"], n_steps, spot, strike, payoff)
        want = ar.closed_form(P["S0"], K, P["T"], P["r"], P["v"], n_steps, spot, strike, payoff)
        if strike == ar.FLOATING and n_steps == 1 and not spot:
            assert got == want == 0.0
        else:
            assert want > 0 and abs(got - want) <= 1e-12 * want, (n_steps, strike, payoff, spot, K, got, want)


def test_one_step_without_the_spot_is_the_european_call(lib):
    """1e-13 of the price.  Both sides are a difference of two terms of the spot's size, each good to a few 1e-16 of
    ITSELF, so a price of at least 1e-2 of the spot holds 1e-13 of its own size; a smaller one (far out of the money at
    a short maturity; chosen by mcamd_bs_call_f64's value) is checked to 1e-15 of the spot instead.  At least 40 of the
    54 cases must remain on the relative bound."""
    n = 0
    for K, T, r, v in itertools.product((80.0, 100.0, 125.0), (0.25, 1.0, 3.0), (-0.02, 0.0, 0.1), (0.1, 0.4)):
        got = capi.asian_geometric_price_f64(100.0, K, T, r, v, 1, 0, ar.FIXED, ar.CALL)
        want = capi.bs_call_f64(100.0, K, T, r, v)
        if want >= 1.0:
            n += 1
            assert abs(got - want) <= 1e-13 * want, (K, T, r, v, got, want)
        else:
            assert abs(got - want) <= 1e-13, (K, T, r, v, got, want)
    assert n >= 40, n


def test_put_call_parity(lib):
    """fixed: C - P = e^{-rT} (E[G] - K); floating: C - P = e^{-rT} (S0 e^{rT} - E[G]); E[G] from the restated moments"""
    f = capi.asian_geometric_price_f64
    for n, spot, K in itertools.product(CLOSED_STEPS, (0, 1), (90.0, 100.0, 110.0)):
        m = n + spot
        mean = math.log(P["S0"]) + (P["r"] - 0.5 * P["v"] ** 2) * (P["T"] / n) * n * (n + 1) / (2.0 * m)
        var = P["v"] ** 2 * (P["T"] / n) * n * (n + 1) * (2 * n + 1) / (6.0 * m * m)
        EG, D = math.exp(mean + 0.5 * var), math.exp(-P["r"] * P["T"])
        args = (P["S0"], K, P["T"], P["r"], P["v"], n, spot)
        assert abs(f(*args, ar.FIXED, ar.CALL) - f(*args, ar.FIXED, ar.PUT) - D * (EG - K)) <= 1e-12 * P["S0"]
        if n == 1 and not spot:
            assert f(*args, ar.FLOATING, ar.CALL) == f(*args, ar.FLOATING, ar.PUT) == 0.0
        else:
            gap = f(*args, ar.FLOATING, ar.CALL) - f(*args, ar.FLOATING, ar.PUT)
            assert abs(gap - (P["S0"] - D * EG)) <= 1e-12 * P["S0"]
        # K is ignored for a floating strike
        assert f(P["S0"], float("nan"), P["T"], P["r"], P["v"], n, spot, ar.FLOATING, ar.PUT) == f(*args, ar.FLOATING, ar.PUT)


def test_closed_form_refusals(lib):
    p = C.c_double(7.0)
    fn = lib.mcamd_asian_geometric_price_f64
    ok = (100.0, 100.0, 1.0, 0.1, 0.2, 12, 1, ar.FIXED, ar.CALL)
    assert fn(*ok, C.byref(p)) == capi.OK and p.value > 0
    assert fn(*ok, None) == capi.ERR_INVALID
    nan, inf = float("nan"), float("inf")
    for i, value in ((0, 0.0), (0, -1.0), (0, nan), (0, inf), (1, 0.0), (1, -5.0), (1, nan), (1, inf), (2, 0.0),
                     (2, -1.0), (2, inf), (3, nan), (3, inf), (4, 0.0), (4, -0.2), (4, nan), (5, 0), (6, 2), (6, -1),
                     (7, 2), (7, -1), (8, 2), (8, -1)):
        args = list(ok)
        args[i] = value
        assert fn(*args, C.byref(p)) == capi.ERR_INVALID, (i, value)
        assert p.value == 0.0
    args = list(ok)
    args[3] = 0.0   # r = 0 is covered
    assert fn(*args, C.byref(p)) == capi.OK and p.value > 0


# ---- the restated estimator against the closed form ---------------------------------------------------------------------

MC_SEED, MC_PATHS = 20261018, 400_000   # committed: every |MC - closed form| below lies within 4 SE with these


@pytest.mark.parametrize("n_steps", [1, 4])
def test_restated_estimator_converges_to_the_closed_form(lib, n_steps):
    """the discrete geometric average is lognormal at every n_steps"""
    z = np.random.default_rng(MC_SEED + n_steps).standard_normal((n_steps, MC_PATHS))
    disc = math.exp(-P["r"] * P["T"])
    for strike, payoff, spot in ar.PRODUCTS:
        s = ar.samples(z, P["S0"], 100.0, P["T"], P["r"], P["v"], ar.GEOMETRIC, strike, payoff, spot)
        got, se = disc * s["y"].mean(), disc * s["y"].std(ddof=1) / math.sqrt(MC_PATHS)
        both = (ar.closed_form(P["S0"], 100.0, P["T"], P["r"], P["v"], n_steps, spot, strike, payoff),
                capi.asian_geometric_price_f64(P["S0"], 100.0, P["T"], P["r"], P["v"], n_steps, spot, strike, payoff))
        print(f"n_steps {n_steps} strike {strike} payoff {payoff} spot {spot}: closed {both[1]:.5f} MC {got:.5f} "
              f"SE {se:.5f}")
        if strike == ar.FLOATING and n_steps == 1 and not spot:
            assert not s["y"].any() and both == (0.0, 0.0)
            continue
        for want in both:
            assert se > 0 and abs(got - want) <= 4.0 * se, (strike, payoff, spot, got, want, se)
        assert (s["y"] >= 0).all() and np.array_equal(s["y"], s["g"])


def test_restatement_identities():
    """one step without the spot: A = G = S_T, so the arithmetic and the geometric sample are the European payoff and
    the floating strike pays nothing; with more steps A >= G path by path (the inequality of the means)"""
    z = np.random.default_rng(5).standard_normal((1, 10_000))
    for dtype in (np.float32, np.float64, np.longdouble):
        a = ar.restate(z, ar.ARITHMETIC, ar.FIXED, ar.CALL, 0, dtype)
        assert np.array_equal(a["A"], a["S_T"]) and np.array_equal(a["G"], a["S_T_log"])
        assert np.array_equal(a["y"], np.maximum(a["S_T"].astype(a["y"].dtype) - 100, 0))
        for payoff in (ar.CALL, ar.PUT):
            assert not ar.restate(z, ar.GEOMETRIC, ar.FLOATING, payoff, 0, dtype)["y"].any()
    z = np.random.default_rng(6).standard_normal((12, 10_000))
    for spot in (0, 1):
        s = ar.restate(z, ar.ARITHMETIC, ar.FIXED, ar.CALL, spot)
        assert (s["A"] >= s["G"] * (1 - 1e-14)).all() and (s["y"] >= s["g"] - 1e-11).all()
        assert abs(s["S_T"] / s["S_T_log"] - 1).max() < 1e-13


# ---- the records the GPU tests read -------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [64, 32])
def test_recorded_restatement_spread(bits):
    got = ar.measure_spread(bits)
    print(f"fp{bits}: largest restatement difference {got:.4e}, record {ar.RECORD['spread'][bits]:.4e}")
    assert 0 < got <= ar.RECORD["spread"][bits]


@pytest.mark.parametrize("bits", [64, 32])
def test_recorded_restatement_spread_of_the_added_inputs(bits):
    """5 steps, and 7 steps on the deep inputs: measured as the record above is, recorded beside it, and below it —
    which is why GPU test 1 holds these cases to the tolerance made of RECORD["spread"]"""
    got = ar.measure_spread(bits, ar.MORE_INPUTS)
    print(f"fp{bits}: largest restatement difference {got:.4e}, record {ar.RECORD['spread_more'][bits]:.4e}")
    assert 0 < got <= ar.RECORD["spread_more"][bits] <= ar.RECORD["spread"][bits]


@pytest.mark.parametrize("bits", [64, 32])
def test_deep_normals_are_those_of_neither_shallow_word(bits):
    """What makes the deep cases worth running: the deep normals share nothing with the streams a dropped high word
    of the path id or of the seed lands on (tests/deep_inputs.py)."""
    check_deep_draws_differ(lambda seed, first: ar.oracle_normals(bits, seed, first, 64, 7))


def test_recorded_correlation():
    got = ar.measure_rho_min()
    print(f"smallest rho(y, g) {got:.6f}, record {ar.RECORD['rho_min']:.6f}")
    assert ar.RECORD["rho_min"] <= got < 1.0
    assert ar.RECORD["rho_min"] >= 0.999   # what makes the control worth carrying: the SE shrinks 22 times and more


def test_recorded_controlled_prices():
    """the record is this very computation: it must come out again (to rounding of the libm in use), the controlled
    price must agree with the plain one and its standard error must be 25 times smaller and more"""
    got = ar.measure_controlled()
    assert set(got) == set(ar.RECORD["controlled"]) == set(ar.PRODUCTS)
    z = np.random.default_rng(ar.CV_SEED).standard_normal((ar.CV_STEPS, ar.CV_PATHS))
    disc = math.exp(-ar.BASE["r"] * ar.BASE["T"])
    for key, (price_, se) in got.items():
        rec_price, rec_se = ar.RECORD["controlled"][key]
        print(key, f"price {price_:.9f} SE {se:.3e}")
        assert abs(price_ - rec_price) <= 1e-9 * rec_price and abs(se - rec_se) <= 1e-6 * rec_se
        y = ar.restate(z, ar.ARITHMETIC, *key)["y"]
        plain, plain_se = disc * y.mean(), disc * y.std(ddof=1) / math.sqrt(y.size)
        assert abs(price_ - plain) <= 4.0 * plain_se and se < plain_se / 25.0, (key, price_, plain, se, plain_se)
