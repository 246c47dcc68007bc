"""CPU-only checks of the autocallable under local-volatility surfaces (include/mcamd.h, mcamd_price_autocall_localvol):
declarations and struct layout; every refusal that needs neither a surface nor the context, in the stated order, and
then the NULL surface array and the NULL entry (a surface cannot exist without a context, so the surface refusals
themselves are the GPU module's); the numpy restatement (tests/autocall_localvol_restate.py) against the two restatements
it collapses onto — autocall_restate on flat surfaces with q = 0 and localvol_restate at d = 1 — and the records the GPU
tests take their tolerances from.  No kernels run here."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import autocall_localvol_restate as alr
import autocall_restate as ar
import localvol_restate as lr

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcamd_price_autocall_localvol", "mcamd_price_autocall_localvol_enqueue")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


def test_header_declares_the_calls_and_the_struct(lib):
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert re.search(r"\}\s*mcamd_autocall_localvol\s*;", header)
    assert re.search(r"#define\s+MCAMD_ABI_VERSION\s+5\b", header) and lib.mcamd_abi_version() == 5
    assert "first carried by the build that ships csrc/autocall_localvol.hip" in header
    assert not re.search(r"mcamd_group_\w*autocall", header)
    for words in ("Greeks", "continuous knock-in", "lane compaction", "calibration", "mcamd_group_* form", "shim name"):
        assert words in header.split("mcamd_autocall_localvol {")[0].split("per-asset local-volatility surfaces")[-1], words
    build = importlib.import_module("monte-carlo-project-cuda_amd.build")
    assert {"autocall_localvol.hip", "autocall_localvol_f32.hip"} <= set(build.SOURCES)
    assert {"autocall_localvol.hpp", "autocall_localvol_impl.hpp"} <= set(build.HEADERS)


def test_struct_matches_the_header():
    # static_assert(sizeof(mcamd_autocall_localvol) == 632) in csrc/capi_localvol.cpp
    A, B = capi.AutocallLocalVol, capi.Autocall
    assert C.sizeof(A) == 632 == C.sizeof(B)
    assert [(k if k != "q" else "v", getattr(A, k).offset) for k, _ in A._fields_] == \
        [(k, getattr(B, k).offset) for k, _ in B._fields_]   # mcamd_autocall with q[] in the place of v[]
    assert (A.q.offset, A.corr.offset) == (56, 120)
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        body = re.search(r"typedef struct mcamd_autocall_localvol \{(.*?)\}", f.read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", body) == [k for k, _ in A._fields_]   # the same fields in the same order
    a = capi.make_autocall_localvol(alr.Q[:3], alr.corr(3), 3, 1.02, 0.04, 0.65, capi.AUTOCALL_KI_EVERY_STEP, 0.01, 2)
    assert (a.n_assets, a.ki_monitoring, a.observe_every, a.first_call_date, a.reserved[0], a.reserved[1]) == \
        (3, 2, 3, 2, 0, 0)
    assert (a.call_level, a.call_step_down, a.coupon, a.ki_level) == (1.02, 0.01, 0.04, 0.65)
    assert list(a.q)[:4] == [*alr.Q[:3], 0.0] and a.corr[8 * 2 + 1] == alr.corr(3)[2][1] and a.corr[3] == 0.0
    with pytest.raises(ValueError):
        capi.make_autocall_localvol([0.0] * 9, np.eye(9))
    assert capi.surface_array(None) is None and capi.surface_array([None, None])[1] is None


# ---- refusals ------------------------------------------------------------------------------------------------------

NO_ARRAY, NULL_ENTRY = "no array", "null entry"


def price(lib, opt, sim, note_, res=True, surfaces=NO_ARRAY, enqueue=False):
    out = capi.AutocallResult()
    ref = lambda x: None if x is None else C.byref(x)
    arr = None if surfaces == NO_ARRAY else (C.c_void_p * 8)()   # eight NULL entries
    if enqueue:
        rc = lib.mcamd_price_autocall_localvol_enqueue(None, ref(opt), ref(sim), ref(note_), arr, None, None)
    else:
        rc = lib.mcamd_price_autocall_localvol(None, ref(opt), ref(sim), ref(note_), arr, None,
                                               C.byref(out) if res else None)
    return rc, lib.mcamd_last_error().decode()


BASE = dict(S0=0.0, v=0.0, K=0.0, r=alr.R, T=alr.T_)   # opt->S0, v, K and B are ignored
NAN, INF = float("nan"), float("inf")


def note(d=3, **kw):
    q, corr = kw.pop("q", alr.Q[:d]), kw.pop("corr", alr.corr(d))
    args = dict(observe_every=3, call_level=1.0, coupon=0.02, ki_level=0.7, ki_monitoring=capi.AUTOCALL_KI_EVERY_STEP)
    return capi.make_autocall_localvol(q, corr, **dict(args, **kw))


def refusals():
    O, S = capi.make_option, capi.make_sim
    opt, sim, ac = O(**BASE), S(1000, 12), note()
    yield "no opt", (None, sim, ac), {}, "non-NULL"
    yield "no sim", (opt, None, ac), {}, "non-NULL"
    yield "no autocall", (opt, sim, None), {}, "non-NULL"
    yield "no res", (opt, sim, ac), dict(res=False), "non-NULL"
    for k in (0, 1):
        bad = note()
        bad.reserved[k] = 1
        yield f"reserved[{k}]", (opt, sim, bad), {}, "reserved"
    # what mcamd_price_basket refuses of n_assets and corr
    for n in (0, -1, 9):
        bad = note()
        bad.n_assets = n
        yield f"n_assets {n}", (opt, sim, bad), {}, "n_assets"
    corr = np.array(alr.corr(3))
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
    for value in (NAN, INF, -INF):
        yield f"q = {value}", (opt, sim, note(q=[0.0, value, 0.01])), {}, "dividend yield"
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
    # the other opt fields must be 0
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
    yield "exponent range", (O(**dict(BASE, T=100.0)), S(1000, 12), note(q=[0.0, -1e4, 0.01])), {}, "exponent range"
    yield "T = 0", (O(**dict(BASE, T=0.0)), sim, ac), {}, "T > 0"
    yield "r = nan", (O(**dict(BASE, r=NAN)), sim, ac), {}, "finite"
    # then the surfaces: the array, then its entries
    yield "no surfaces", (opt, sim, ac), {}, "surfaces must be non-NULL"
    yield "a NULL entry", (opt, sim, ac), dict(surfaces=NULL_ENTRY), "surfaces[0] is NULL"


@pytest.mark.parametrize("case", list(refusals()), ids=lambda c: c[0])
def test_refusals_before_surfaces_and_context_are_looked_at(lib, case):
    """Every case but the last two is wrong in one way only and is given an array of NULL entries and no context: the
    message names the request's fault, so the refusal came before the surfaces and the context."""
    _, args, kw, words = case
    kw = dict(dict(surfaces=NULL_ENTRY), **kw) if case[0] != "no surfaces" else kw
    rc, msg = price(lib, *args, **kw)
    assert rc == capi.ERR_INVALID and words in msg, msg
    if kw.get("res", True):   # the enqueue form shares the checks
        rc, msg = price(lib, *args, enqueue=True, **kw)
        assert rc == capi.ERR_INVALID and words in msg, msg


def test_refusals_come_in_the_stated_order(lib):
    """a request wrong in several ways reports the first fault of the header's list"""
    O, S = capi.make_option, capi.make_sim
    # what is wrong -> the words of its refusal, in the header's order; request k has fault k and every later one
    words = dict(reserved="reserved", n_assets="n_assets", q="dividend yield", observe_every="observe_every",
                 first_call_date="first_call_date", coupon="coupon", r="finite", Sk="Sk", flags="flags",
                 precision="precision")
    order = list(words)
    for first in range(len(order)):
        on = set(order[first:])
        kw = {}
        if "q" in on:
            kw["q"] = [0.0, NAN, 0.01]
        if "observe_every" in on:
            kw["observe_every"] = 5
        elif "first_call_date" in on:
            kw["first_call_date"] = 9          # of 4 dates (observe_every = 3 divides 12)
        if "coupon" in on:
            kw["coupon"] = -1.0
        ac = note(**kw)
        if "reserved" in on:
            ac.reserved[0] = 1
        if "n_assets" in on:
            ac.n_assets = 9
        opt = O(**dict(BASE, r=NAN if "r" in on else alr.R, Sk=95.0 if "Sk" in on else 0.0))
        sim = S(1000, 12, precision=16 if "precision" in on else capi.F64,
                flags=capi.FLAG_ANTITHETIC if "flags" in on else 0)
        rc, msg = price(lib, opt, sim, ac)   # and no surfaces, and no context
        assert rc == capi.ERR_INVALID and words[order[first]] in msg, (order[first], msg)
    # with nothing wrong in the request: the surfaces, then (with a surface only a context can make) the context
    rc, msg = price(lib, O(**BASE), S(1000, 12), note())
    assert rc == capi.ERR_INVALID and "surfaces" in msg and "ctx" not in msg, msg


def test_both_autocall_calls_refuse_a_schedule_in_the_same_words(lib):
    """Each defect of the schedule — the run from "observe_every must be >= 1" through the refusals of the terms — on a
    note of 2 assets and 12 steps (65 steps where 65 dates are the defect), without a context: mcamd_price_autocall and
    mcamd_price_autocall_localvol return the same code and leave the same text."""
    KI_M, KI_S = capi.AUTOCALL_KI_AT_MATURITY, capi.AUTOCALL_KI_EVERY_STEP
    defects = [(12, dict(observe_every=0), "observe_every"), (12, dict(observe_every=5), "observe_every"),
               (65, dict(observe_every=1), "MCAMD_AUTOCALL_MAX_DATES"),
               (12, dict(first_call_date=0), "first_call_date"), (12, dict(first_call_date=5), "first_call_date"),
               (12, dict(call_level=0.75, call_step_down=0.25, ki_monitoring=0), "last date"),
               (12, dict(call_level=-1.0, ki_monitoring=0), "last date"),
               (12, dict(ki_monitoring=-1), "ki_monitoring"), (12, dict(ki_monitoring=3), "ki_monitoring"),
               (12, dict(coupon=-0.01), "coupon"), (12, dict(coupon=NAN), "coupon"),
               (12, dict(call_level=INF), "call_level"), (12, dict(call_level=NAN), "call_level"),
               (12, dict(call_step_down=-0.01), "call_step_down"), (12, dict(call_step_down=NAN), "call_step_down")]
    defects += [(12, dict(ki_monitoring=ki, **kw), "ki_level") for ki in (KI_M, KI_S)
                for kw in (dict(ki_level=0.0), dict(ki_level=1.01), dict(ki_level=NAN), dict(call_level=0.6),
                           dict(call_level=1.0, call_step_down=0.125, ki_level=0.625))]
    args = dict(observe_every=3, call_level=1.0, coupon=0.02, ki_level=0.7, ki_monitoring=KI_S)
    opt, corr = capi.make_option(**dict(BASE, v=0.2)), alr.corr(2)
    for n_steps, kw, words in defects:
        sim, kw = capi.make_sim(1000, n_steps), dict(args, **kw)
        out = capi.AutocallResult()
        plain = capi.make_autocall([0.2, 0.25], corr, **kw)
        rc_a = lib.mcamd_price_autocall(None, C.byref(opt), C.byref(sim), C.byref(plain), None, C.byref(out))
        msg_a = lib.mcamd_last_error().decode()
        rc_b, msg_b = price(lib, opt, sim, capi.make_autocall_localvol(alr.Q[:2], corr, **kw), surfaces=NULL_ENTRY)
        assert rc_a == rc_b == capi.ERR_INVALID and words in msg_a, (kw, msg_a)
        assert msg_a == msg_b, (kw, msg_a, msg_b)


@pytest.mark.parametrize("d", alr.DS)
@pytest.mark.parametrize("ki", (alr.KI_NONE,) + alr.KI_MODES)
@pytest.mark.parametrize("flags,prec", [(0, capi.F64), (capi.FLAG_LOG_SPACE, capi.F32)])
def test_accepted_requests_reach_the_surfaces(lib, d, ki, flags, prec):
    sim = capi.make_sim(1000, 12, prec, flags=flags, path_offset=3, n_paths_local=0)
    for kw in (dict(), dict(observe_every=1, first_call_date=12), dict(observe_every=12), dict(call_step_down=0.05)):
        rc, msg = price(lib, capi.make_option(**BASE), sim, note(d, ki_monitoring=ki, **kw))
        assert rc == capi.ERR_INVALID and "surfaces must be non-NULL" in msg, msg
        rc, msg = price(lib, capi.make_option(**BASE), sim, note(d, ki_monitoring=ki, **kw), surfaces=NULL_ENTRY)
        assert rc == capi.ERR_INVALID and "surfaces[0] is NULL" in msg, msg
    # opt->S0, v, K and B are ignored; so are ki_level without a knock-in and q and corr beyond n_assets
    for S0, v, K, B in ((NAN, NAN, NAN, NAN), (-1.0, -1.0, -1.0, -1.0), (0.0, 0.0, INF, INF)):
        rc, msg = price(lib, capi.make_option(**dict(BASE, S0=S0, v=v, K=K, B=B)), sim, note(d, ki_monitoring=ki))
        assert rc == capi.ERR_INVALID and "surfaces must be non-NULL" in msg, msg
    ac = note(d, ki_level=NAN, ki_monitoring=alr.KI_NONE)
    if d < 8:
        ac.q[d], ac.corr[d], ac.corr[8 * d + d] = NAN, 7.0, -1.0
    rc, msg = price(lib, capi.make_option(**BASE), sim, ac)
    assert rc == capi.ERR_INVALID and "surfaces must be non-NULL" in msg, msg


# ---- the restatement against the restatements it collapses onto -------------------------------------------------------

@pytest.mark.parametrize("prec", [alr.F64, alr.F32])
def test_flat_surfaces_without_dividends_are_the_constant_volatility_note(prec):
    """Flat surfaces at sigma_j = v_j with q = 0 against autocall_restate.samples at v_j, on the GPU test's own streams:
    the same call date and knock-in flag on every path kept by both, y within the elementwise tolerance.  The two
    differ in where they round: v_j sqrt(dt) l_jk narrowed once there, l_jk narrowed and s_j sqrt(dt) rounded here."""
    worst = 0.0
    for d in alr.DS:
        for ki in alr.KI_MODES:
            for shape in alr.SHAPES:
                own, _, keep_a, _ = ar.compare(prec, d, ki, shape)
                grids, sig = alr.surfaces(d, alr.flat)
                got = alr.samples(alr.stream_of(prec, alr.SHALLOW), shape[0], grids, sig, [0.0] * d, alr.corr(d), alr.T_,
                                  alr.R, dtype=alr.NP_T[prec], **alr.terms(d, shape, ki))
                keep = keep_a & (got["min_abs_d"] >= alr.MARGIN)
                assert keep.mean() >= 1.0 - 2.0 * alr.CAP
                assert np.array_equal(got["date"][keep], own["date"][keep]), (d, ki, shape)
                assert np.array_equal(got["knocked"][keep], own["knocked"][keep]), (d, ki, shape)
                want = np.asarray(own["y"], dtype=np.float64)
                err = np.abs(np.asarray(got["y"], dtype=np.float64) - want)
                assert (err[keep] <= alr.elementwise_tolerance(prec, want)[keep]).all(), (d, ki, shape, err[keep].max())
                worst = max(worst, float(err[keep].max()))
    print(f"prec {prec}: largest difference from the constant-volatility restatement {worst:.3e}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("j,n_steps", [(0, 5), (0, 50), (3, 5), (3, 50)])
def test_one_asset_walks_the_local_volatility_path(dtype, j, n_steps):
    """d = 1: S_T = e^{X_n} of localvol_restate.samples, to rounding.  That restatement multiplies and adds where this
    one fuses, and forms dt and sqrt(dt) in the dtype: a few roundings of terms below 1 per step, bounded by 8 n eps."""
    z = np.random.default_rng(31 + n_steps).standard_normal((n_steps, 20_000))
    grid, sigma, q = alr.grid(j), alr.skewed(j), 0.03
    got = alr.samples(z, n_steps, [grid], [sigma], [q], [[1.0]], alr.T_, alr.R, n_steps, 1e6, 0.0, dtype=dtype)
    want = lr.samples(z, 1.0, 1.0, 0.0, alr.T_, alr.R, q, grid, sigma, lr.NO_BARRIER, lr.PUT, lr.DISCRETE, dtype=dtype)
    S_T = np.exp(got["X"][0].astype(np.float64))
    err = np.abs(S_T - want["S_T"].astype(np.float64)) / S_T
    bound = 8.0 * n_steps * float(np.finfo(dtype).eps)
    print(f"{np.dtype(dtype).name} grid {grid} n_steps {n_steps}: largest relative difference {err.max():.3e}, bound {bound:.3e}")
    assert not got["date"].any() and err.max() <= bound and S_T.std() > 0.05


# ---- the records the GPU tests read -------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [alr.F64, alr.F32])
def test_recorded_spread_and_excluded_share(prec):
    """Over the GPU test's own cases, deep ones included: the two restatements agree on the call date and the knock-in
    flag of every kept path, differ by at most the recorded SPREAD, and leave out at most the recorded share — which
    lies below the cap.  Each case has more than 5 % of its paths called and more than 5 % not called."""
    spread = excluded = 0.0
    for d, ki, shape, where in alr.CASES:
        own, other, keep, s = alr.compare(prec, d, ki, shape, where)
        assert np.array_equal(own["date"][keep], other["date"][keep]), (d, ki, shape)
        assert np.array_equal(own["knocked"][keep], other["knocked"][keep]), (d, ki, shape)
        called = (own["date"] > 0).mean()
        assert 0.05 < called < 0.95, (d, ki, shape, called)
        spread, excluded = max(spread, s), max(excluded, 1.0 - keep.mean())
    print(f"prec {prec}: largest restatement difference {spread:.4e}, record {alr.SPREAD[prec]:.4e}; largest left-out "
          f"share {excluded:.5f}, record {alr.EXCLUDED[prec]:.5f}, cap {alr.CAP}")
    assert 0 < spread <= alr.SPREAD[prec]
    assert 0 < excluded <= alr.EXCLUDED[prec] <= alr.CAP
    assert sum(n_t * n_x for n_t, n_x, _, _ in (alr.grid(j) for j in range(8))) == 496
    # some case exercises each branch of a path not called: not knocked in (1), knocked in below 1
    own = alr.compare(prec, 8, alr.KI_EVERY_STEP, (50, 10), alr.SHALLOW)[0]
    free = own["date"] == 0
    assert (free & ~own["knocked"]).any() and (free & own["knocked"] & (own["y"] < 1)).any()


def test_recorded_note_price():
    """the record is this very computation: it must come out again (to rounding of the libm in use)"""
    got, se = alr.price_note()
    print(f"3-asset note under the skewed surfaces: price {got:.9f} SE {se:.3e}")
    rec, rec_se = alr.NOTE_RECORD
    assert abs(got - rec) <= 1e-9 * rec and abs(se - rec_se) <= 1e-6 * rec_se
    assert 0.8 < rec < 1.1 and 0 < rec_se < 1e-3
    # the skew is worth something: the constant-volatility note of tests/autocall_restate.py is priced elsewhere
    assert abs(rec - ar.NOTE_RECORD[0]) > 4.0 * (rec_se + ar.NOTE_RECORD[1])
