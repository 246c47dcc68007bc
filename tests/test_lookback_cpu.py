"""CPU-only checks of the lookback entry points (include/mcamd.h, mcamd_price_lookback): declarations and struct
layout, every refusal that depends on the request alone — each happens before the context is looked at, so
ctx = NULL reaches them — the host closed form against an independent restatement, and the numpy restatement of the
continuous estimator against the closed form.  No kernels run here."""
import ctypes as C
import importlib
import itertools
import math
import os
import re

import numpy as np
import pytest

import lookback_restate as lr

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


NAMES = ("mcamd_price_lookback", "mcamd_price_lookback_enqueue", "mcamd_lookback_price_f64")


def test_header_declares_the_calls_and_the_struct(lib):
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert re.search(r"\}\s*mcamd_lookback\s*;", header)
    for name, value in (("LOOKBACK_FLOATING", 0), ("LOOKBACK_FIXED", 1)):
        assert re.search(r"#define\s+MCAMD_" + name + r"\s+" + str(value) + r"\b", header), name
        assert getattr(capi, name) == value == getattr(lr, name.split("_", 1)[1])
    assert (capi.PAYOFF_CALL, capi.PAYOFF_PUT, capi.MONITOR_DISCRETE, capi.MONITOR_CONTINUOUS) == \
        (lr.CALL, lr.PUT, lr.DISCRETE, lr.CONTINUOUS)
    assert re.search(r"#define\s+MCAMD_ABI_VERSION\s+5\b", header) and lib.mcamd_abi_version() == 5
    assert not re.search(r"mcamd_group_\w*lookback", header)


def test_struct_matches_the_header():
    # static_assert(sizeof(mcamd_lookback) == 16) in csrc/capi_pathdep.cpp
    Lb = capi.Lookback
    assert C.sizeof(Lb) == 16
    assert (Lb.strike.offset, Lb.payoff.offset, Lb.monitoring.offset, Lb.reserved.offset) == (0, 4, 8, 12)
    b = capi.make_lookback(capi.LOOKBACK_FIXED, capi.PAYOFF_PUT, capi.MONITOR_DISCRETE)
    assert (b.strike, b.payoff, b.monitoring, b.reserved) == (1, 1, 0, 0)
    d = capi.make_lookback()
    assert (d.strike, d.payoff, d.monitoring, d.reserved) == (0, 0, 1, 0)


# ---- refusals ------------------------------------------------------------------------------------------------------

def price(lib, opt, sim, lb, res=True, ctx=None):
    out = capi.Result()
    ref = lambda x: None if x is None else C.byref(x)
    rc = lib.mcamd_price_lookback(ctx, ref(opt), ref(sim), ref(lb), None, C.byref(out) if res else None)
    return rc, lib.mcamd_last_error().decode()


BASE = dict(S0=100.0, K=100.0, r=0.1, v=0.2, T=1.0)


def refusals():
    O, S, Lm = capi.make_option, capi.make_sim, capi.make_lookback
    opt, sim, lb = O(**BASE), S(1000, 50), Lm()
    fixed = Lm(strike=capi.LOOKBACK_FIXED)
    yield "no opt", (None, sim, lb), {}, "non-NULL"
    yield "no sim", (opt, None, lb), {}, "non-NULL"
    yield "no lookback", (opt, sim, None), {}, "non-NULL"
    yield "no res", (opt, sim, lb), dict(res=False), "non-NULL"
    for k in (-1, 2):
        yield f"strike {k}", (opt, sim, Lm(strike=k)), {}, "strike"
    for p in (-1, 2):
        yield f"payoff {p}", (opt, sim, Lm(payoff=p)), {}, "payoff"
    for m in (-1, 2):
        yield f"monitoring {m}", (opt, sim, Lm(monitoring=m)), {}, "monitoring"
    bad = Lm()
    bad.reserved = 1
    yield "reserved", (opt, sim, bad), {}, "reserved"
    for K in (0.0, -90.0, float("nan"), float("inf")):
        yield f"fixed, K = {K}", (O(**dict(BASE, K=K)), sim, fixed), {}, "finite K > 0"
    yield "use_window", (O(**BASE, use_window=1), sim, lb), {}, "window"
    yield "P1", (O(**BASE, P1=1), sim, lb), {}, "window"
    yield "P2", (O(**BASE, P2=3), sim, lb), {}, "window"
    yield "Ik", (O(**BASE, Ik=2), sim, lb), {}, "window"
    yield "Sk", (O(**BASE, Sk=95.0), sim, lb), {}, "Sk"
    yield "Tk", (O(**BASE, Tk=5), sim, lb), {}, "Tk"
    yield "dt", (O(**BASE, dt=0.01), sim, lb), {}, "dt"
    yield "v = 0", (O(**dict(BASE, v=0.0)), sim, lb), {}, "v > 0"
    yield "v < 0", (O(**dict(BASE, v=-0.2)), sim, lb), {}, "v > 0"
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE, capi.FLAG_PRODUCT_FORM,
                  capi.FLAG_LOG_SPACE | capi.FLAG_ANTITHETIC, 32):
        yield f"flags {flags}", (opt, S(1000, 50, flags=flags), lb), {}, "flags"
    # what mcamd_price_paths refuses on sim
    yield "precision", (opt, S(1000, 50, precision=16), lb), {}, "precision"
    yield "n_steps 0", (opt, S(1000, 0), lb), {}, "n_steps"
    yield "shard overflow", (opt, S(1 << 63, 50, path_offset=(1 << 64) - 10, n_paths_local=100), lb), {}, "overflows"
    yield "exponent range", (O(**dict(BASE, v=100.0, T=100.0)), S(1000, 50), lb), {}, "exponent range"


@pytest.mark.parametrize("case", list(refusals()), ids=lambda c: c[0])
def test_refusals_before_the_context_is_looked_at(lib, case):
    _, args, kw, words = case
    rc, msg = price(lib, *args, **kw)
    assert rc == capi.ERR_INVALID and words in msg, msg
    if kw.get("res", True):   # the enqueue form shares the checks
        ref = lambda x: None if x is None else C.byref(x)
        rc = lib.mcamd_price_lookback_enqueue(None, ref(args[0]), ref(args[1]), ref(args[2]), None, None)
        assert rc == capi.ERR_INVALID and words in lib.mcamd_last_error().decode()


@pytest.mark.parametrize("strike,payoff", lr.PRODUCTS)
@pytest.mark.parametrize("monitoring", [capi.MONITOR_DISCRETE, capi.MONITOR_CONTINUOUS])
@pytest.mark.parametrize("flags,prec", [(0, capi.F64), (capi.FLAG_LOG_SPACE, capi.F32)])
def test_accepted_requests_reach_the_missing_context(lib, strike, payoff, monitoring, flags, prec):
    sim = capi.make_sim(1000, 50, prec, flags=flags, path_offset=3, n_paths_local=0)
    rc, msg = price(lib, capi.make_option(**BASE), sim, capi.make_lookback(strike, payoff, monitoring))
    assert rc == capi.ERR_INVALID and "ctx" in msg, msg


def test_a_floating_strike_ignores_K_and_every_lookback_ignores_B(lib):
    sim = capi.make_sim(1000, 50, n_paths_local=0)
    for K in (0.0, -5.0, float("nan")):
        rc, msg = price(lib, capi.make_option(**dict(BASE, K=K, B=-3.0)), sim, capi.make_lookback())
        assert rc == capi.ERR_INVALID and "ctx" in msg, msg
    rc, msg = price(lib, capi.make_option(**dict(BASE, B=float("nan"))), sim,
                    capi.make_lookback(strike=capi.LOOKBACK_FIXED))
    assert rc == capi.ERR_INVALID and "ctx" in msg, msg


# ---- the closed form -----------------------------------------------------------------------------------------------

def closed_form_grid():
    """S0 / K on both sides of 1 x three maturities x five rates of both signs (|r| >= 0.01) x three volatilities x the
    four products: 5 * 3 * 5 * 3 * 4 = 900 cases"""
    for ratio, T, r, v in itertools.product((0.8, 0.9, 1.0, 1.1, 1.25), (0.25, 1.0, 3.0),
                                            (-0.05, -0.01, 0.01, 0.05, 0.1), (0.1, 0.2, 0.4)):
        for strike, payoff in lr.PRODUCTS:
            yield 100.0, 100.0 / ratio, T, r, v, strike, payoff


def test_closed_form_against_the_restatement(lib):
    """1e-12 relative to the price.  The formulas add terms as large as S0 (1 + v^2 / 2|r|) — up to 9 S0 on this grid —
    each good to a few 1e-16 of ITSELF, and the quadrature of the restatement adds 1536 terms of either sign the
    same way; a price of at least 1e-3 of the spot therefore holds 1e-12 of its own size with an order of magnitude to
    spare, and a smaller one (a fixed strike far out of the money at a short maturity; chosen by the restated price,
    not by the library's) is checked to 1e-15 of the spot per unit of (1 + v^2 / 2|r|) instead.  At least 800 cases
    must remain on the relative bound."""
    worst, worst_small, n = 0.0, 0.0, 0
    for S0, K, T, r, v, strike, payoff in closed_form_grid():
        got = capi.lookback_price_f64(S0, K, T, r, v, strike, payoff)
        want = lr.closed_form(S0, K, T, r, v, strike, payoff)
        if want >= 1e-3 * S0:
            worst = max(worst, abs(got - want) / want)
            n += 1
        else:
            worst_small = max(worst_small, abs(got - want) / (S0 * (1.0 + v * v / (2.0 * abs(r)))))
    print(f"{n} cases, worst relative deviation {worst:.2e}; prices below 1e-3 S0: worst {worst_small:.2e} of "
          "S0 (1 + v^2 / 2|r|)")
    assert n >= 800 and worst <= 1e-12 and worst_small <= 1e-15, (n, worst, worst_small)


def test_fixed_strikes_the_extremum_has_passed_are_floating_plus_a_forward(lib):
    f = capi.lookback_price_f64
    for S0, K, T, r, v, strike, payoff in closed_form_grid():
        if strike != lr.FIXED:
            continue
        fwd = K * math.exp(-r * T)
        if payoff == lr.CALL and K <= S0:
            want = f(S0, K, T, r, v, lr.FLOATING, lr.PUT) + S0 - fwd
        elif payoff == lr.PUT and K >= S0:
            want = f(S0, K, T, r, v, lr.FLOATING, lr.CALL) + fwd - S0
        else:
            continue
        assert abs(f(S0, K, T, r, v, strike, payoff) - want) <= 1e-13 * (S0 + K), (K, T, r, v, payoff)
    # and the two branches of a fixed strike meet at K = S0 (the formula for K beyond the spot, evaluated just there)
    for payoff in (lr.CALL, lr.PUT):
        at = f(100.0, 100.0, 1.0, 0.1, 0.2, lr.FIXED, payoff)
        beside = f(100.0, 100.0 * (1 + (1e-9 if payoff == lr.CALL else -1e-9)), 1.0, 0.1, 0.2, lr.FIXED, payoff)
        assert abs(at - beside) <= 1e-6


def test_monotone_in_the_strike(lib):
    strikes = [60.0 + 2.5 * i for i in range(33)]   # 60 .. 140, through S0 = 100
    for T, r, v in ((0.5, 0.1, 0.2), (2.0, -0.02, 0.35)):
        calls = [capi.lookback_price_f64(100.0, K, T, r, v, lr.FIXED, lr.CALL) for K in strikes]
        puts = [capi.lookback_price_f64(100.0, K, T, r, v, lr.FIXED, lr.PUT) for K in strikes]
        assert all(a > b > 0 for a, b in zip(calls, calls[1:]))
        assert all(0 < a < b for a, b in zip(puts, puts[1:]))
        # a lookback dominates the vanilla option of the same strike, and the floating ones are positive
        for K, c in zip(strikes, calls):
            assert c >= capi.bs_call_f64(100.0, K, T, r, v)
        flo = [capi.lookback_price_f64(100.0, K, T, r, v, lr.FLOATING, p) for K in (1.0, 500.0) for p in (0, 1)]
        assert flo[0] == flo[2] > 0 and flo[1] == flo[3] > 0   # K is ignored


def test_closed_form_refusals(lib):
    p = C.c_double(7.0)
    fn = lib.mcamd_lookback_price_f64
    ok = (100.0, 100.0, 1.0, 0.1, 0.2, lr.FIXED, lr.CALL)
    assert fn(*ok, C.byref(p)) == capi.OK and p.value > 0
    assert fn(*ok, None) == capi.ERR_INVALID
    nan, inf = float("nan"), float("inf")
    for i, value in ((0, 0.0), (0, -1.0), (0, nan), (0, inf), (1, 0.0), (1, -5.0), (1, nan), (1, inf), (2, 0.0),
                     (2, -1.0), (2, inf), (3, 0.0), (3, -0.0), (3, nan), (3, inf), (4, 0.0), (4, -0.2), (4, nan),
                     (5, 2), (5, -1), (6, 2), (6, -1)):
        args = list(ok)
        args[i] = value
        assert fn(*args, C.byref(p)) == capi.ERR_INVALID, (i, value)
        assert p.value == 0.0
    args = list(ok)
    args[3] = 0.0
    assert fn(*args, C.byref(p)) == capi.ERR_INVALID and "r == 0" in lib.mcamd_last_error().decode()
    # a floating strike takes any K
    for K in (0.0, -1.0, nan):
        assert fn(100.0, K, 1.0, 0.1, 0.2, lr.FLOATING, lr.PUT, C.byref(p)) == capi.OK and p.value > 0


# ---- the restated estimator against the closed form ---------------------------------------------------------------------

MC_SEED, MC_PATHS = 20261017, 400_000   # committed: every |MC - closed form| below lies within 4 SE with these
PARAMS = dict(S0=100.0, T=1.0, r=0.1, v=0.2)


def draws(n_steps, n=MC_PATHS):
    rng = np.random.default_rng(MC_SEED + n_steps)
    z = rng.standard_normal((n_steps, n))
    u = 1.0 - rng.random((n_steps, n))   # (0, 1]
    return z, u


@pytest.mark.parametrize("n_steps", [1, 4])
def test_restated_estimator_converges_to_the_closed_form(lib, n_steps):
    """unbiased at every n_steps: one step and four steps both reproduce the continuously monitored price"""
    z, u = draws(n_steps)
    disc = math.exp(-PARAMS["r"] * PARAMS["T"])
    for (strike, payoff), K in itertools.product(lr.PRODUCTS, (90.0, 100.0, 110.0)):
        s = lr.samples(z, u, PARAMS["S0"], K, PARAMS["T"], PARAMS["r"], PARAMS["v"], strike, payoff, lr.CONTINUOUS)
        got, se = disc * s["y"].mean(), disc * s["y"].std(ddof=1) / math.sqrt(s["y"].size)
        for want in (lr.closed_form(PARAMS["S0"], K, PARAMS["T"], PARAMS["r"], PARAMS["v"], strike, payoff),
                     capi.lookback_price_f64(PARAMS["S0"], K, PARAMS["T"], PARAMS["r"], PARAMS["v"], strike, payoff)):
            assert abs(got - want) <= 4.0 * se, (strike, payoff, K, got, want, se)
        print(f"n_steps {n_steps} strike {strike} payoff {payoff} K {K}: closed {want:.5f} MC {got:.5f} SE {se:.5f} "
              f"({(got - want) / se:+.2f} SE), live {s['live'].mean() / n_steps:.3f}")
        # the Q rule drops no bridge extremum that would have moved E
        assert not s["dropped"].any()
        assert (s["y"] >= 0).all()


def test_the_q_rule_drops_nothing_where_it_bites():
    """50 steps, where a good part of the lane-steps have q >= Q; and float32, whose Q is lower and whose uniforms
    are the generator's own 2^-32 lattice"""
    n_steps, n = 50, 40_000
    z, u = draws(n_steps, n)
    rng = np.random.default_rng(MC_SEED)
    words = rng.integers(0, 1 << 32, size=(n_steps, n), dtype=np.uint64)
    u32 = (words.astype(np.float32) * np.float32(2.0 ** -32) + np.float32(2.0 ** -32))
    for (strike, payoff), (dtype, uu) in itertools.product(lr.PRODUCTS, ((np.float64, u), (np.float32, u32))):
        s = lr.samples(z, uu, 100.0, 100.0, 1.0, 0.1, 0.2, strike, payoff, lr.CONTINUOUS, dtype)
        skipped = 1.0 - s["live"].sum() / (n_steps * n)
        print(f"strike {strike} payoff {payoff} {np.dtype(dtype).name}: {skipped:.3f} of the lane-steps have q >= Q")
        assert 0.1 < skipped < 0.9, skipped
        assert not s["dropped"].any()


def test_continuous_extremum_lies_beyond_the_discrete_one():
    n_steps = 12
    z, u = draws(n_steps, 100_000)
    for strike, payoff in lr.PRODUCTS:
        d = lr.samples(z, None, 100.0, 100.0, 1.0, 0.1, 0.2, strike, payoff, lr.DISCRETE)
        c = lr.samples(z, u, 100.0, 100.0, 1.0, 0.1, 0.2, strike, payoff, lr.CONTINUOUS)
        assert np.array_equal(d["S_T"], c["S_T"]) and not d["live"].any()
        if lr.wants_maximum(strike, payoff):
            assert (c["S_E"] >= d["S_E"]).all() and (d["S_E"] >= np.maximum(100.0, d["S_T"])).all()
        else:
            assert (c["S_E"] <= d["S_E"]).all() and (d["S_E"] <= np.minimum(100.0, d["S_T"])).all()
        assert (c["y"] >= d["y"]).all() and c["y"].mean() > d["y"].mean()
    # one discrete step: the floating call is the European call struck at the spot
    z1 = z[:1]
    y = lr.samples(z1, None, 100.0, 0.0, 1.0, 0.1, 0.2, lr.FLOATING, lr.CALL, lr.DISCRETE)
    assert np.array_equal(y["y"], np.maximum(y["S_T"] - 100.0, 0.0))


def test_restatement_precisions_agree():
    """the three dtypes walk the same paths; the sample is continuous in every input, so no path is left out"""
    n_steps = 50
    rng = np.random.default_rng(3)
    z = rng.standard_normal((n_steps, 5000)).astype(np.float32).astype(np.float64)
    u = (1.0 - rng.random((n_steps, 5000))).astype(np.float32).astype(np.float64)
    u = np.maximum(u, 2.0 ** -32)
    for strike, payoff in lr.PRODUCTS:
        y64 = lr.samples(z, u, 100.0, 95.0, 1.0, 0.1, 0.2, strike, payoff, lr.CONTINUOUS)["y"]
        yld = lr.samples(z, u, 100.0, 95.0, 1.0, 0.1, 0.2, strike, payoff, lr.CONTINUOUS, np.longdouble)["y"]
        y32 = lr.samples(z, u, 100.0, 95.0, 1.0, 0.1, 0.2, strike, payoff, lr.CONTINUOUS, np.float32)["y"]
        assert np.abs(y64 - yld.astype(np.float64)).max() <= 1e-11
        assert np.abs(y64 - y32).max() <= 2e-3
