"""CPU-only checks of the single-barrier entry points (include/mcamd.h, mcamd_price_barrier): declarations and struct
layout, every refusal that depends on the request alone — each happens before the context is looked at, so
ctx = NULL reaches them — the host closed form against an independent restatement, and the numpy restatement of the
estimator against the closed form.  No kernels run here."""
import ctypes as C
import importlib
import itertools
import math
import os
import re

import numpy as np
import pytest

import barrier_restate as br

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


NAMES = ("mcamd_price_barrier", "mcamd_price_barrier_enqueue", "mcamd_barrier_price_f64")


def test_header_declares_the_calls_and_the_struct(lib):
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert re.search(r"\}\s*mcamd_barrier\s*;", header)
    for name, value in (("BARRIER_DOWN_OUT", 0), ("BARRIER_DOWN_IN", 1), ("BARRIER_UP_OUT", 2), ("BARRIER_UP_IN", 3),
                        ("MONITOR_DISCRETE", 0), ("MONITOR_CONTINUOUS", 1)):
        assert re.search(r"#define\s+MCAMD_" + name + r"\s+" + str(value) + r"\b", header), name
        assert getattr(capi, name) == value == getattr(br, name.split("_", 1)[1])
    assert re.search(r"#define\s+MCAMD_ABI_VERSION\s+5\b", header) and lib.mcamd_abi_version() == 5
    assert not re.search(r"mcamd_group_\w*barrier", header)


def test_struct_matches_the_header():
    # static_assert(sizeof(mcamd_barrier) == 16) in csrc/capi_pathdep.cpp
    Bq = capi.Barrier
    assert C.sizeof(Bq) == 16
    assert (Bq.kind.offset, Bq.payoff.offset, Bq.monitoring.offset, Bq.reserved.offset) == (0, 4, 8, 12)
    b = capi.make_barrier(capi.BARRIER_UP_IN, capi.PAYOFF_PUT, capi.MONITOR_DISCRETE)
    assert (b.kind, b.payoff, b.monitoring, b.reserved) == (3, 1, 0, 0)


# ---- refusals ------------------------------------------------------------------------------------------------------

def price(lib, opt, sim, bar, res=True, ctx=None):
    out = capi.Result()
    ref = lambda x: None if x is None else C.byref(x)
    rc = lib.mcamd_price_barrier(ctx, ref(opt), ref(sim), ref(bar), None, C.byref(out) if res else None)
    return rc, lib.mcamd_last_error().decode()


DOWN = dict(S0=100.0, K=100.0, B=90.0, r=0.1, v=0.2, T=1.0)


def refusals():
    O, S, Bm = capi.make_option, capi.make_sim, capi.make_barrier
    opt, sim, bar = O(**DOWN), S(1000, 50), Bm()
    yield "no opt", (None, sim, bar), {}, "non-NULL"
    yield "no sim", (opt, None, bar), {}, "non-NULL"
    yield "no barrier", (opt, sim, None), {}, "non-NULL"
    yield "no res", (opt, sim, bar), dict(res=False), "non-NULL"
    for k in (-1, 4):
        yield f"kind {k}", (opt, sim, Bm(kind=k)), {}, "kind"
    for p in (-1, 2):
        yield f"payoff {p}", (opt, sim, Bm(payoff=p)), {}, "payoff"
    for m in (-1, 2):
        yield f"monitoring {m}", (opt, sim, Bm(monitoring=m)), {}, "monitoring"
    bad = Bm()
    bad.reserved = 1
    yield "reserved", (opt, sim, bad), {}, "reserved"
    for B in (0.0, -90.0, float("nan")):
        yield f"B = {B}", (O(**dict(DOWN, B=B)), sim, bar), {}, "B must be positive"
    yield "down, S0 below B", (O(**dict(DOWN, B=110.0)), sim, bar), {}, "live side"
    yield "down, S0 on B", (O(**dict(DOWN, B=100.0)), sim, Bm(kind=capi.BARRIER_DOWN_IN)), {}, "live side"
    yield "up, S0 above B", (opt, sim, Bm(kind=capi.BARRIER_UP_OUT)), {}, "live side"
    yield "up, S0 on B", (O(**dict(DOWN, B=100.0)), sim, Bm(kind=capi.BARRIER_UP_IN)), {}, "live side"
    yield "use_window", (O(**DOWN, use_window=1), sim, bar), {}, "window"
    yield "P1", (O(**DOWN, P1=1), sim, bar), {}, "window"
    yield "P2", (O(**DOWN, P2=3), sim, bar), {}, "window"
    yield "Ik", (O(**DOWN, Ik=2), sim, bar), {}, "window"
    yield "Sk", (O(**DOWN, Sk=95.0), sim, bar), {}, "Sk"
    yield "Tk", (O(**DOWN, Tk=5), sim, bar), {}, "Tk"
    yield "dt", (O(**DOWN, dt=0.01), sim, bar), {}, "dt"
    yield "v = 0", (O(**dict(DOWN, v=0.0)), sim, bar), {}, "v > 0"
    yield "v < 0", (O(**dict(DOWN, v=-0.2)), sim, bar), {}, "v > 0"
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE, capi.FLAG_PRODUCT_FORM,
                  capi.FLAG_LOG_SPACE | capi.FLAG_ANTITHETIC, 32):
        yield f"flags {flags}", (opt, S(1000, 50, flags=flags), bar), {}, "flags"
    # what mcamd_price_paths refuses on sim
    yield "precision", (opt, S(1000, 50, precision=16), bar), {}, "precision"
    yield "n_steps 0", (opt, S(1000, 0), bar), {}, "n_steps"
    yield "shard overflow", (opt, S(1 << 63, 50, path_offset=(1 << 64) - 10, n_paths_local=100), bar), {}, "overflows"
    yield "exponent range", (O(**dict(DOWN, v=100.0, T=100.0)), S(1000, 50), bar), {}, "exponent range"


@pytest.mark.parametrize("case", list(refusals()), ids=lambda c: c[0])
def test_refusals_before_the_context_is_looked_at(lib, case):
    _, args, kw, words = case
    rc, msg = price(lib, *args, **kw)
    assert rc == capi.ERR_INVALID and words in msg, msg
    if kw.get("res", True):   # the enqueue form shares the checks
        ref = lambda x: None if x is None else C.byref(x)
        rc = lib.mcamd_price_barrier_enqueue(None, ref(args[0]), ref(args[1]), ref(args[2]), None, None)
        assert rc == capi.ERR_INVALID and words in lib.mcamd_last_error().decode()


@pytest.mark.parametrize("kind", br.KINDS)
@pytest.mark.parametrize("payoff", [capi.PAYOFF_CALL, capi.PAYOFF_PUT])
@pytest.mark.parametrize("monitoring", [capi.MONITOR_DISCRETE, capi.MONITOR_CONTINUOUS])
@pytest.mark.parametrize("flags,prec", [(0, capi.F64), (capi.FLAG_LOG_SPACE, capi.F32)])
def test_accepted_requests_reach_the_missing_context(lib, kind, payoff, monitoring, flags, prec):
    opt = capi.make_option(**dict(DOWN, B=110.0 if br.is_up(kind) else 90.0))
    sim = capi.make_sim(1000, 50, prec, flags=flags, path_offset=3, n_paths_local=0)
    rc, msg = price(lib, opt, sim, capi.make_barrier(kind, payoff, monitoring))
    assert rc == capi.ERR_INVALID and "ctx" in msg, msg


# ---- the closed form -----------------------------------------------------------------------------------------------

def closed_form_grid():
    """8 types x K on both sides of B x short and long T x two (r, v): 8 * 7 * 3 * 2 = 336 cases"""
    for kind, payoff in itertools.product(br.KINDS, (br.CALL, br.PUT)):
        B = 120.0 if br.is_up(kind) else 85.0
        for K in (80.0, 90.0, 95.0, 100.0, 105.0, 110.0, 125.0):
            for T in (0.5, 1.0, 2.0):
                for r, v in ((0.1, 0.2), (0.03, 0.35)):
                    yield 100.0, K, B, T, r, v, kind, payoff


def test_closed_form_against_the_restatement(lib):
    """1e-12 relative to the price.  Both forms are sums of terms as large as S0 and K, each good to a few 1e-16 of
    ITSELF, so a price that is a leftover of less than 1e-3 of the spot cannot hold 1e-12 of its own size in either
    form: those cases of the grid (chosen by the restated price, not by the library's) are checked to 1e-15 of the
    spot instead, and at least 200 cases must remain on the relative bound.  A price that is exactly 0 (strike beyond
    the barrier of a knock-out) must come out exactly 0."""
    worst, worst_small, n = 0.0, 0.0, 0
    for S0, K, B, T, r, v, kind, payoff in closed_form_grid():
        got = capi.barrier_price_f64(S0, K, B, T, r, v, kind, payoff)
        want = br.closed_form(S0, K, B, T, r, v, kind, payoff)
        if want == 0.0:
            assert got == 0.0, (kind, payoff, K, T)
            n += 1
        elif want >= 1e-3 * S0:
            worst = max(worst, abs(got - want) / want)
            n += 1
        else:
            worst_small = max(worst_small, abs(got - want) / S0)
    print(f"{n} cases, worst relative deviation {worst:.2e}; prices below 1e-3 S0: worst {worst_small:.2e} of S0")
    assert n >= 200 and worst <= 1e-12 and worst_small <= 1e-15, (n, worst, worst_small)


def test_in_plus_out_is_the_vanilla_price(lib):
    for S0, K, B, T, r, v, kind, payoff in closed_form_grid():
        if not br.is_out(kind):
            continue
        call = capi.bs_call_f64(S0, K, T, r, v)
        van = call if payoff == br.CALL else call - S0 + K * math.exp(-r * T)   # the put by parity
        both = (capi.barrier_price_f64(S0, K, B, T, r, v, kind, payoff)
                + capi.barrier_price_f64(S0, K, B, T, r, v, kind + 1, payoff))
        assert abs(both - van) <= 1e-12 * max(call, K), (kind, payoff, K, T, both, van)


@pytest.mark.parametrize("payoff", [br.CALL, br.PUT])
def test_a_far_barrier_leaves_the_vanilla_price(lib, payoff):
    S0, K, T, r, v = 100.0, 105.0, 1.0, 0.1, 0.2
    call = capi.bs_call_f64(S0, K, T, r, v)
    van = call if payoff == br.CALL else call - S0 + K * math.exp(-r * T)
    for kind, B in ((br.DOWN_OUT, 1e-3), (br.UP_OUT, 1e7)):
        assert abs(capi.barrier_price_f64(S0, K, B, T, r, v, kind, payoff) - van) <= 1e-12 * max(call, K)
        assert abs(capi.barrier_price_f64(S0, K, B, T, r, v, kind + 1, payoff)) <= 1e-12 * max(call, K)


def test_closed_form_refusals(lib):
    p = C.c_double(7.0)
    fn = lib.mcamd_barrier_price_f64
    ok = (100.0, 100.0, 90.0, 1.0, 0.1, 0.2, br.DOWN_OUT, br.CALL)
    assert fn(*ok, C.byref(p)) == capi.OK and p.value > 0
    assert fn(*ok, None) == capi.ERR_INVALID
    for i, value in ((0, 0.0), (0, -1.0), (1, 0.0), (2, 0.0), (2, -5.0), (3, 0.0), (5, 0.0), (5, -0.2), (6, 4), (6, -1),
                     (7, 2), (7, -1), (0, 80.0), (0, 90.0)):
        args = list(ok)
        args[i] = value
        assert fn(*args, C.byref(p)) == capi.ERR_INVALID, (i, value)
        assert p.value == 0.0
    up = list(ok)
    up[6] = br.UP_IN   # S0 = 100 above B = 90: knocked side of an up-barrier
    assert fn(*up, C.byref(p)) == capi.ERR_INVALID and "live side" in lib.mcamd_last_error().decode()


# ---- the restated estimator against the closed form ---------------------------------------------------------------------

MC_SEED, MC_PATHS = 20240607, 400_000   # committed: every |MC - closed form| below lies within 4 SE with these


def mc_price(z, S0, K, B, T, r, v, kind, payoff, monitoring):
    y = br.samples(z, S0, K, B, T, r, v, kind, payoff, monitoring)["y"]
    disc = math.exp(-r * T)
    return disc * y.mean(), disc * y.std(ddof=1) / math.sqrt(y.size)


@pytest.mark.parametrize("n_steps", [1, 12])
def test_restated_estimator_converges_to_the_closed_form(n_steps):
    S0, K, T, r, v = 100.0, 100.0, 1.0, 0.1, 0.2
    z = np.random.default_rng(MC_SEED + n_steps).standard_normal((n_steps, MC_PATHS))
    for kind, payoff in itertools.product(br.KINDS, (br.CALL, br.PUT)):
        B = 115.0 if br.is_up(kind) else 88.0
        want = br.closed_form(S0, K, B, T, r, v, kind, payoff)
        got, se = mc_price(z, S0, K, B, T, r, v, kind, payoff, br.CONTINUOUS)
        print(f"n_steps {n_steps} kind {kind} payoff {payoff}: closed {want:.5f} MC {got:.5f} SE {se:.5f} "
              f"({(got - want) / se:+.2f} SE)")
        assert abs(got - want) <= 4.0 * se, (kind, payoff, got, want, se)


def test_discrete_knock_out_lies_above_the_continuous_one():
    S0, K, T, r, v, n_steps = 100.0, 100.0, 1.0, 0.1, 0.2, 12
    z = np.random.default_rng(MC_SEED).standard_normal((n_steps, 100_000))
    for kind, payoff in itertools.product((br.DOWN_OUT, br.UP_OUT), (br.CALL, br.PUT)):
        B = 115.0 if br.is_up(kind) else 88.0
        d = br.samples(z, S0, K, B, T, r, v, kind, payoff, br.DISCRETE)
        c = br.samples(z, S0, K, B, T, r, v, kind, payoff, br.CONTINUOUS)
        assert (d["w"] >= c["w"]).all() and (d["y"] >= c["y"]).all()
        assert d["y"].mean() > c["y"].mean()
        assert set(np.unique(d["w"])) <= {0.0, 1.0}
        # the knock-in is the complement, sample for sample
        both = d["y"] + br.samples(z, S0, K, B, T, r, v, kind + 1, payoff, br.DISCRETE)["y"]
        assert np.array_equal(both, d["h"])


def test_restatement_precisions_agree():
    """the three dtypes walk the same paths: float32 and longdouble against float64 away from the barrier"""
    S0, K, B, T, r, v, n_steps = 100.0, 100.0, 90.0, 1.0, 0.1, 0.2, 50
    z = np.random.default_rng(3).standard_normal((n_steps, 5000)).astype(np.float32).astype(np.float64)
    y64 = br.samples(z, S0, K, B, T, r, v, br.DOWN_OUT, br.CALL, br.CONTINUOUS)
    keep = y64["min_abs_d"] >= 1e-4
    yld = br.samples(z, S0, K, B, T, r, v, br.DOWN_OUT, br.CALL, br.CONTINUOUS, np.longdouble)["y"]
    y32 = br.samples(z, S0, K, B, T, r, v, br.DOWN_OUT, br.CALL, br.CONTINUOUS, np.float32)["y"]
    assert keep.mean() > 0.9
    assert np.abs(y64["y"][keep] - yld[keep].astype(np.float64)).max() <= 1e-9
    assert np.abs(y64["y"][keep] - y32[keep]).max() <= 2e-3
