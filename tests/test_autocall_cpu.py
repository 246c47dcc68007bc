"""CPU-only checks of the autocallable entry points (include/mcamd.h, mcamd_price_autocall): declarations and struct
layout, every refusal that depends on the request alone — each happens before the context is looked at, so ctx = NULL
reaches them — the host closed form of the one-asset one-date note against a numpy quadrature and against the numpy
restatement of the estimator, and the records in tests/autocall_restate.py that the GPU tests take their tolerances
from.  No kernels run here."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import autocall_restate as ar
from deep_inputs import check_deep_draws_differ

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


NAMES = ("mcamd_price_autocall", "mcamd_price_autocall_enqueue", "mcamd_autocall_single_date_price_f64")


def test_header_declares_the_calls_and_the_structs(lib):
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert re.search(r"\}\s*mcamd_autocall\s*;", header) and re.search(r"\}\s*mcamd_autocall_result\s*;", header)
    for name, value in (("AUTOCALL_MAX_DATES", 64), ("AUTOCALL_KI_NONE", 0), ("AUTOCALL_KI_AT_MATURITY", 1),
                        ("AUTOCALL_KI_EVERY_STEP", 2)):
        assert re.search(r"#define\s+MCAMD_" + name + r"\s+" + str(value) + r"\b", header), name
        assert getattr(capi, name) == value
    assert (capi.AUTOCALL_KI_NONE, capi.AUTOCALL_KI_AT_MATURITY, capi.AUTOCALL_KI_EVERY_STEP, capi.AUTOCALL_MAX_DATES) == \
        (ar.KI_NONE, ar.KI_AT_MATURITY, ar.KI_EVERY_STEP, ar.MAX_DATES)
    assert re.search(r"#define\s+MCAMD_ABI_VERSION\s+5\b", header) and lib.mcamd_abi_version() == 5
    assert "first carried by the build that ships csrc/autocall.hip" in header
    assert not re.search(r"mcamd_group_\w*autocall", header)
    for words in ("memory or conditional coupons", "continuous knock-in", "Greeks", "mcamd_group_* form", "shim name"):
        assert words in header, words   # what the header comment declares out of scope


def test_structs_match_the_header():
    # static_assert(sizeof(mcamd_autocall) == 632 && sizeof(mcamd_autocall_result) == 112) in csrc/capi_multi.cpp
    A, R = capi.Autocall, capi.AutocallResult
    assert C.sizeof(A) == 632 and C.sizeof(R) == 112
    assert (A.n_assets.offset, A.ki_monitoring.offset, A.observe_every.offset, A.first_call_date.offset,
            A.reserved.offset, A.call_level.offset, A.call_step_down.offset, A.coupon.offset, A.ki_level.offset,
            A.v.offset, A.corr.offset) == (0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 120)
    assert [getattr(R, k).offset for k, _ in R._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 100, 104,
                                                             108]
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        body = re.search(r"typedef struct mcamd_autocall_result \{(.*?)\}", f.read(), re.S).group(1)
    assert re.findall(r"(\w+);", body) == [k for k, _ in R._fields_]   # the same fields in the same order
    v, corr = ar.inputs(3)
    a = capi.make_autocall(v, corr, 3, 1.02, 0.04, 0.65, capi.AUTOCALL_KI_EVERY_STEP, 0.01, 2)
    assert (a.n_assets, a.ki_monitoring, a.observe_every, a.first_call_date, a.reserved[0], a.reserved[1]) == \
        (3, 2, 3, 2, 0, 0)
    assert (a.call_level, a.call_step_down, a.coupon, a.ki_level) == (1.02, 0.01, 0.04, 0.65)
    assert list(a.v)[:4] == [*v, 0.0] and a.corr[8 * 2 + 1] == corr[2][1] and a.corr[3] == 0.0
    with pytest.raises(ValueError):
        capi.make_autocall([0.2] * 9, np.eye(9))


# ---- refusals ------------------------------------------------------------------------------------------------------

def price(lib, opt, sim, autocall, res=True, ctx=None):
    out = capi.AutocallResult()
    ref = lambda x: None if x is None else C.byref(x)
    rc = lib.mcamd_price_autocall(ctx, ref(opt), ref(sim), ref(autocall), None, C.byref(out) if res else None)
    return rc, lib.mcamd_last_error().decode()


BASE = dict(S0=0.0, v=0.0, K=0.0, r=ar.R, T=ar.T_)   # opt->S0, v, K and B are ignored
NAN, INF = float("nan"), float("inf")


def note(d=3, **kw):
    v, corr = ar.inputs(d)
    v, corr = kw.pop("v", v), kw.pop("corr", corr)
    args = dict(observe_every=3, call_level=1.0, coupon=0.02, ki_level=0.7, ki_monitoring=capi.AUTOCALL_KI_EVERY_STEP)
    return capi.make_autocall(v, corr, **dict(args, **kw))


def refusals():
    O, S = capi.make_option, capi.make_sim
    opt, sim, ac = O(**BASE), S(1000, 12), note()
    yield "no opt", (None, sim, ac), {}, "non-NULL"
    yield "no sim", (opt, None, ac), {}, "non-NULL"
    yield "no autocall", (opt, sim, None), {}, "non-NULL"
    yield "no res", (opt, sim, ac), dict(res=False), "non-NULL"
    # what mcamd_price_basket refuses of n_assets, v and corr
    for n in (0, -1, 9):
        bad = note()
        bad.n_assets = n
        yield f"n_assets {n}", (opt, sim, bad), {}, "n_assets"
    for value in (0.0, -0.2, NAN, INF):
        yield f"v = {value}", (opt, sim, note(v=[0.2, value, 0.3])), {}, "v > 0"
    corr = np.array(ar.inputs(3)[1])
    for name, change, words in (("diagonal", ((1, 1, 0.99),), "exactly 1"), ("asymmetric", ((2, 0, 0.3),), "symmetric"),
                                ("beyond 1", ((2, 0, 1.5), (0, 2, 1.5)), "beyond"),
                                ("nan", ((1, 0, NAN), (0, 1, NAN)), "symmetric"),
                                ("rho = 1", ((1, 0, 1.0), (0, 1, 1.0)), "positive definite"),
                                ("indefinite", ((1, 0, 0.9), (0, 1, 0.9), (2, 1, 0.9), (1, 2, 0.9), (2, 0, -0.9),
                                                (0, 2, -0.9)), "positive definite")):
        c = corr.copy()
        for j, k, value in change:
            c[j, k] = value
        yield f"corr {name}", (opt, sim, note(corr=c)), {}, words
    for k in (0, 1):
        bad = note()
        bad.reserved[k] = 1
        yield f"reserved[{k}]", (opt, sim, bad), {}, "reserved"
    # the shape rules
    yield "observe_every 0", (opt, sim, note(observe_every=0)), {}, "observe_every"
    yield "observe_every 5 of 12", (opt, sim, note(observe_every=5)), {}, "observe_every"
    yield "observe_every 24 of 12", (opt, sim, note(observe_every=24)), {}, "observe_every"
    yield "65 dates", (opt, S(1000, 65), note(observe_every=1)), {}, "MCAMD_AUTOCALL_MAX_DATES"
    yield "first_call_date 0", (opt, sim, note(first_call_date=0)), {}, "first_call_date"
    yield "first_call_date 5 of 4", (opt, sim, note(first_call_date=5)), {}, "first_call_date"
    for k in (-1, 3):
        yield f"ki_monitoring {k}", (opt, sim, note(ki_monitoring=k)), {}, "ki_monitoring"
    # the terms
    for value in (-0.01, NAN, INF):
        yield f"coupon {value}", (opt, sim, note(coupon=value)), {}, "coupon"
    for value in (-0.01, NAN):
        yield f"call_step_down {value}", (opt, sim, note(call_step_down=value)), {}, "call_step_down"
    for value in (NAN, INF):
        yield f"call_level {value}", (opt, sim, note(call_level=value)), {}, "call_level"
    yield "L_M = 0", (opt, sim, note(call_level=0.75, call_step_down=0.25, ki_monitoring=0)), {}, "last date"
    yield "L_M < 0", (opt, sim, note(call_level=-1.0, ki_monitoring=0)), {}, "last date"
    for ki in (capi.AUTOCALL_KI_AT_MATURITY, capi.AUTOCALL_KI_EVERY_STEP):
        for value in (0.0, -0.5, 1.01, NAN):
            yield f"ki {ki}, ki_level {value}", (opt, sim, note(ki_level=value, ki_monitoring=ki)), {}, "ki_level"
        yield f"ki {ki}, ki_level = L_M", (opt, sim, note(call_level=1.0, call_step_down=0.125, ki_level=0.625,
                                                           ki_monitoring=ki)), {}, "ki_level"
        yield f"ki {ki}, ki_level > L_M", (opt, sim, note(call_level=0.6, ki_monitoring=ki)), {}, "ki_level"
    # the other opt fields must be 0, as for mcamd_price_basket
    yield "use_window", (O(**BASE, use_window=1), sim, ac), {}, "window"
    yield "P1", (O(**BASE, P1=1), sim, ac), {}, "window"
    yield "P2", (O(**BASE, P2=3), sim, ac), {}, "window"
    yield "Ik", (O(**BASE, Ik=2), sim, ac), {}, "window"
    yield "Sk", (O(**BASE, Sk=95.0), sim, ac), {}, "Sk"
    yield "Tk", (O(**BASE, Tk=5), sim, ac), {}, "Tk"
    yield "dt", (O(**BASE, dt=0.01), sim, ac), {}, "dt"
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE, capi.FLAG_PRODUCT_FORM,
                  capi.FLAG_LOG_SPACE | capi.FLAG_ANTITHETIC, capi.FLAG_LOG_SPACE | capi.FLAG_PRODUCT_FORM, 32):
        yield f"flags {flags}", (opt, S(1000, 12, flags=flags), ac), {}, "flags"
    # what mcamd_price_paths refuses on sim
    yield "precision", (opt, S(1000, 12, precision=16), ac), {}, "precision"
    yield "n_steps 0", (opt, S(1000, 0), ac), {}, "n_steps"
    yield "shard overflow", (opt, S(1 << 63, 12, path_offset=(1 << 64) - 10, n_paths_local=100), ac), {}, "overflows"
    yield "exponent range", (O(**dict(BASE, T=100.0)), S(1000, 12), note(v=[0.2, 100.0, 0.3])), {}, "exponent range"
    yield "T = 0", (O(**dict(BASE, T=0.0)), sim, ac), {}, "T > 0"
    yield "r = nan", (O(**dict(BASE, r=NAN)), sim, ac), {}, "finite"


@pytest.mark.parametrize("case", list(refusals()), ids=lambda c: c[0])
def test_refusals_before_the_context_is_looked_at(lib, case):
    _, args, kw, words = case
    rc, msg = price(lib, *args, **kw)
    assert rc == capi.ERR_INVALID and words in msg, msg
    if kw.get("res", True):   # the enqueue form shares the checks
        ref = lambda x: None if x is None else C.byref(x)
        rc = lib.mcamd_price_autocall_enqueue(None, ref(args[0]), ref(args[1]), ref(args[2]), None, None)
        assert rc == capi.ERR_INVALID and words in lib.mcamd_last_error().decode()


@pytest.mark.parametrize("d", ar.DS)
@pytest.mark.parametrize("ki", (ar.KI_NONE,) + ar.KI_MODES)
@pytest.mark.parametrize("flags,prec", [(0, capi.F64), (capi.FLAG_LOG_SPACE, capi.F32)])
def test_accepted_requests_reach_the_missing_context(lib, d, ki, flags, prec):
    sim = capi.make_sim(1000, 12, prec, flags=flags, path_offset=3, n_paths_local=0)
    for kw in (dict(), dict(observe_every=1, first_call_date=12), dict(observe_every=12), dict(call_step_down=0.05)):
        rc, msg = price(lib, capi.make_option(**BASE), sim, note(d, ki_monitoring=ki, **kw))
        assert rc == capi.ERR_INVALID and "ctx" in msg, msg
    rc, msg = price(lib, capi.make_option(**BASE), capi.make_sim(1000, 64, prec, n_paths_local=0),
                    note(d, ki_monitoring=ki, observe_every=1))
    assert rc == capi.ERR_INVALID and "ctx" in msg, msg   # MCAMD_AUTOCALL_MAX_DATES dates are taken


def test_ignored_fields(lib):
    """opt->S0, v, K and B; ki_level without a knock-in; v and corr beyond n_assets"""
    sim = capi.make_sim(1000, 12, n_paths_local=0)
    for S0, v, K, B in ((NAN, NAN, NAN, NAN), (-1.0, -1.0, -1.0, -1.0), (0.0, 0.0, INF, INF)):
        rc, msg = price(lib, capi.make_option(**dict(BASE, S0=S0, v=v, K=K, B=B)), sim, note())
        assert rc == capi.ERR_INVALID and "ctx" in msg, msg
    for ki_level in (NAN, -1.0, 5.0):
        rc, msg = price(lib, capi.make_option(**BASE), sim, note(ki_level=ki_level, ki_monitoring=ar.KI_NONE))
        assert rc == capi.ERR_INVALID and "ctx" in msg, msg
    ac = note(2)
    ac.v[2], ac.corr[2], ac.corr[8 * 2 + 2] = NAN, 7.0, -1.0
    rc, msg = price(lib, capi.make_option(**BASE), sim, ac)
    assert rc == capi.ERR_INVALID and "ctx" in msg, msg


# ---- the closed form -----------------------------------------------------------------------------------------------

CLOSED = [(T, r, v, L, c, B, ki) for T in (0.5, 1.0, 3.0) for r in (0.0, 0.05) for v in (0.15, 0.4)
          for L, c in ((1.05, 0.03), (0.9, 0.1), (1.0, 0.0)) for B, ki in ((0.0, ar.KI_NONE), (0.7, ar.KI_AT_MATURITY),
                                                                              (0.85, ar.KI_AT_MATURITY))]


def test_closed_form_against_the_quadrature(lib):
    """1e-12: the integrand is smooth between the kinks, which lie on panel edges"""
    for T, r, v, L, c, B, ki in CLOSED:
        got = capi.autocall_single_date_price_f64(T, r, v, L, c, B, ki)
        want = ar.single_date_by_quadrature(T, r, v, L, c, B, ki)
        assert 0.5 < want < 1.2 and abs(got - want) <= 1e-12, (T, r, v, L, c, B, ki, got, want)
    # without a coupon and a knock-in the note is a bond
    assert abs(capi.autocall_single_date_price_f64(2.0, 0.04, 0.3, 1.1, 0.0) - math.exp(-0.08)) <= 1e-15
    # a level of 1 with the knock-in level at 1 too is refused (ki_level < L_M); just below, the note is the bond less the at-the-money put
    near = capi.autocall_single_date_price_f64(1.0, 0.05, 0.2, 1.0 + 1e-9, 0.0, 1.0, ar.KI_AT_MATURITY)
    put = capi.bs_call_f64(1.0, 1.0, 1.0, 0.05, 0.2) - 1.0 + math.exp(-0.05)   # parity
    assert abs(near - (math.exp(-0.05) - put)) <= 1e-14


def test_closed_form_refusals(lib):
    p = C.c_double(7.0)
    fn = lib.mcamd_autocall_single_date_price_f64
    ok = (1.0, 0.05, 0.2, 1.05, 0.03, 0.7, ar.KI_AT_MATURITY)
    assert fn(*ok, C.byref(p)) == capi.OK and p.value > 0
    assert fn(*ok, None) == capi.ERR_INVALID
    for i, value in ((0, 0.0), (0, -1.0), (0, NAN), (0, INF), (1, NAN), (1, INF), (2, 0.0), (2, -0.2), (2, NAN), (2, INF),
                     (3, 0.0), (3, -1.0), (3, NAN), (3, INF), (3, 0.7), (3, 0.5), (4, -0.01), (4, NAN), (4, INF),
                     (5, 0.0), (5, -0.1), (5, 1.01), (5, NAN), (6, -1), (6, 3), (6, ar.KI_EVERY_STEP)):
        args = list(ok)
        args[i] = value
        assert fn(*args, C.byref(p)) == capi.ERR_INVALID, (i, value)
        assert p.value == 0.0
    args = list(ok)
    args[5], args[6] = NAN, ar.KI_NONE   # ki_level is ignored without a knock-in
    assert fn(*args, C.byref(p)) == capi.OK and p.value > 0


MC_SEED, MC_PATHS = 20261018, 1_000_000   # committed: every |MC - closed form| below lies within 4 SE with these


@pytest.mark.parametrize("n_steps", [1, 4])
@pytest.mark.parametrize("ki,B", [(ar.KI_NONE, 0.0), (ar.KI_AT_MATURITY, 0.8)])
def test_restated_estimator_converges_to_the_closed_form(lib, n_steps, ki, B):
    """one asset, one date: the steps in between change nothing but the draws"""
    T, r, v, L, c = 1.0, 0.05, 0.25, 1.02, 0.06
    z = np.random.default_rng(MC_SEED + n_steps).standard_normal((n_steps, MC_PATHS))
    s = ar.samples(z, n_steps, [v], [[1.0]], T, r, n_steps, L, c, B, ki)
    disc = math.exp(-r * T)
    got, se = disc * s["y"].mean(), disc * s["y"].std(ddof=1) / math.sqrt(MC_PATHS)
    want = capi.autocall_single_date_price_f64(T, r, v, L, c, B, ki)
    print(f"n_steps {n_steps} ki {ki}: closed {want:.6f} MC {got:.6f} SE {se:.6f}, called {(s['date'] > 0).mean():.3f}, "
          f"knocked in {(s['knocked'] & (s['date'] == 0)).mean():.3f}")
    assert se > 0 and abs(got - want) <= 4.0 * se, (got, want, se)
    assert 0.3 < (s["date"] > 0).mean() < 0.7 and set(np.unique(s["date"])) == {0, 1}
    assert (ki == ar.KI_NONE) == (not s["knocked"].any())


def test_restatement_identities():
    """what the definitions imply whatever the draws: a called path is paid the table's entry and is live up to its
    date; a level nobody reaches calls nobody, and then every sample is 1 less the worst-of knock-in put of
    basket_restate; a level everybody reaches calls everybody at first_call_date; a path knocked in on the way and called later is paid the call"""
    d, n_steps, every = 3, 12, 3
    v, corr = ar.inputs(d)
    z = np.random.default_rng(5).standard_normal((n_steps * d, 20_000))
    for dtype in (np.float32, np.float64, np.longdouble):
        s = ar.samples(z, n_steps, v, corr, ar.T_, ar.R, every, 1.0, 0.02, 0.7, ar.KI_EVERY_STEP, 0.01, dtype=dtype)
        _, pay, t = ar.tables(n_steps, every, ar.T_, ar.R, 1.0, 0.02, 0.01)
        called = s["date"] > 0
        assert 0.2 < called.mean() < 0.9 and (s["knocked"] & ~called).mean() > 0.05
        assert np.array_equal(s["y"][called], pay[s["date"][called] - 1]) and (s["y"][~called] <= 1).all()
        assert np.array_equal(s["live"], np.where(called, s["date"] * every, n_steps))
        assert np.array_equal(s["y"][~called] < 1, (s["knocked"] & (s["l_n"] < 0))[~called])
        never = ar.samples(z, n_steps, v, corr, ar.T_, ar.R, every, 1e6, 0.02, 0.7, ar.KI_EVERY_STEP, dtype=dtype)
        put = ar.br.samples(z, n_steps, np.ones(d), v, np.ones(d), corr, 1.0, ar.T_, ar.R, ar.br.WORST_OF, ar.br.PUT,
                            ar.br.DOWN_IN, 0.7, dtype)
        assert not never["date"].any() and np.array_equal(never["knocked"], put["hit"])
        assert np.abs(never["y"] - (1 - put["y"])).max() <= 2.0 ** -52
        for first in (1, 2, 4):
            always = ar.samples(z, n_steps, v, corr, ar.T_, ar.R, every, 1e-6, 0.02, 1e-7, ar.KI_EVERY_STEP,
                                first_call_date=first, dtype=dtype)
            assert (always["date"] == first).all() and (always["y"] == pay_of(first, n_steps, every)).all()
    late = ar.samples(z, n_steps, v, corr, ar.T_, ar.R, every, 0.9, 0.02, 0.7, ar.KI_EVERY_STEP)
    both = (late["date"] > 0) & late["knocked"]
    assert both.any() and (late["y"][both] > 1).all()   # knocked in on the way, called later: paid the call


def pay_of(q, n_steps, every):
    return ar.tables(n_steps, every, ar.T_, ar.R, 1e-6, 0.02)[1][q - 1]


# ---- the records the GPU tests read -------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [ar.F64, ar.F32])
def test_recorded_spread_and_excluded_share(prec):
    """Over the GPU test's own cases: the two restatements agree on the call date and the knock-in flag of every kept
    path, differ by at most the recorded SPREAD, and leave out at most the recorded share — which lies below the cap.
    Each case has more than 5 % of its paths called and more than 5 % not called."""
    spread = excluded = 0.0
    for d, ki, shape, where in ar.CASES:
        own, other, keep, s = ar.compare(prec, d, ki, shape, where)
        assert np.array_equal(own["date"][keep], other["date"][keep]), (d, ki, shape)
        assert np.array_equal(own["knocked"][keep], other["knocked"][keep]), (d, ki, shape)
        called = (own["date"] > 0).mean()
        assert 0.05 < called < 0.95, (d, ki, shape, called)
        spread, excluded = max(spread, s), max(excluded, 1.0 - keep.mean())
    print(f"prec {prec}: largest restatement difference {spread:.4e}, record {ar.SPREAD[prec]:.4e}; largest left-out "
          f"share {excluded:.5f}, record {ar.EXCLUDED[prec]:.5f}, cap {ar.CAP}")
    assert 0 < spread <= ar.SPREAD[prec]
    assert 0 < excluded <= ar.EXCLUDED[prec] <= ar.CAP
    # some case exercises each branch of a path not called: not knocked in (1), knocked in below 1, knocked in above 1
    d, ki, shape, where = 8, ar.KI_EVERY_STEP, (50, 10), ar.SHALLOW
    own = ar.compare(prec, d, ki, shape, where)[0]
    free = own["date"] == 0
    assert (free & ~own["knocked"]).any() and (free & own["knocked"] & (own["y"] < 1)).any()


@pytest.mark.parametrize("prec", [ar.F64, ar.F32])
def test_deep_normals_are_those_of_neither_shallow_word(prec):
    check_deep_draws_differ(lambda seed, first: ar.br.stream(prec, seed, first, 64, 7))


def test_recorded_note_price():
    """the record is this very computation: it must come out again (to rounding of the libm in use)"""
    got, se = ar.price_note()
    print(f"3-asset note: price {got:.9f} SE {se:.3e}")
    rec, rec_se = ar.NOTE_RECORD
    assert abs(got - rec) <= 1e-9 * rec and abs(se - rec_se) <= 1e-6 * rec_se
    assert 0.8 < rec < 1.1 and 0 < rec_se < 1e-3
