"""CPU-only checks of the basket entry points (include/mcamd.h, mcamd_price_basket): declarations and struct layout,
every refusal that depends on the request alone — each happens before the context is looked at, so ctx = NULL reaches
them — the two host closed forms against independent restatements, the numpy restatement of the estimator against
the closed forms, and the measurement the GPU test's tolerance is taken from.  No kernels run here."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import basket_restate as br
from deep_inputs import check_deep_draws_differ

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


NAMES = ("mcamd_price_basket", "mcamd_price_basket_enqueue", "mcamd_basket_geometric_price_f64",
         "mcamd_exchange_price_f64")


def test_header_declares_the_calls_and_the_struct(lib):
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert re.search(r"\}\s*mcamd_basket\s*;", header)
    for name, value in (("MAX_ASSETS", 8), ("ARITHMETIC", 0), ("GEOMETRIC", 1), ("BEST_OF", 2), ("WORST_OF", 3),
                        ("NO_BARRIER", 0), ("DOWN_OUT", 1), ("DOWN_IN", 2), ("UP_OUT", 3), ("UP_IN", 4)):
        assert re.search(r"#define\s+MCAMD_BASKET_" + name + r"\s+" + str(value) + r"\b", header), name
        assert getattr(capi, "BASKET_" + name) == value
        assert name == "MAX_ASSETS" or getattr(br, name) == value
    assert re.search(r"#define\s+MCAMD_ABI_VERSION\s+5\b", header) and lib.mcamd_abi_version() == 5
    assert not re.search(r"mcamd_group_\w*basket", header)


def test_struct_matches_the_header():
    # static_assert(sizeof(mcamd_basket) == 728) in csrc/capi_multi.cpp
    Bk = capi.Basket
    assert C.sizeof(Bk) == 728
    assert (Bk.n_assets.offset, Bk.kind.offset, Bk.payoff.offset, Bk.barrier.offset, Bk.reserved.offset, Bk.S0.offset,
            Bk.v.offset, Bk.w.offset, Bk.corr.offset) == (0, 4, 8, 12, 16, 24, 88, 152, 216)
    S0, v, corr = br.inputs(3)
    b = capi.make_basket(S0, v, [1, 2, 3], corr, capi.BASKET_WORST_OF, capi.PAYOFF_PUT, capi.BASKET_DOWN_IN)
    assert (b.n_assets, b.kind, b.payoff, b.barrier, list(b.reserved)) == (3, 3, 1, 2, [0, 0])
    assert list(b.S0)[:4] == [80.0, 90.0, 100.0, 0.0] and list(b.w)[:3] == [1.0, 2.0, 3.0]
    assert b.corr[8 * 2 + 1] == 0.6 and b.corr[8 * 2 + 0] == 0.6 ** 2 and b.corr[3] == 0.0
    with pytest.raises(ValueError):
        capi.make_basket([1.0] * 9, [1.0] * 9, [1.0] * 9, np.eye(9))


# ---- refusals ------------------------------------------------------------------------------------------------------

OPT = dict(S0=0.0, v=0.0, K=1.0, r=br.R, T=br.T_, B=0.8)    # opt->S0 and opt->v are ignored


def basket(d=3, kind=capi.BASKET_WORST_OF, payoff=capi.PAYOFF_PUT, barrier=capi.BASKET_NO_BARRIER, **edit):
    S0, v, corr = br.inputs(d)
    w = br.weights(kind, d)[0]
    b = capi.make_basket(S0, v, w, corr, kind, payoff, barrier)
    for name, (index, value) in edit.items():
        getattr(b, name)[index] = value
    return b


def price(lib, opt, sim, bk, res=True, ctx=None):
    out = capi.Result()
    ref = lambda x: None if x is None else C.byref(x)
    rc = lib.mcamd_price_basket(ctx, ref(opt), ref(sim), ref(bk), None, C.byref(out) if res else None)
    return rc, lib.mcamd_last_error().decode()


def refusals():
    O, S = capi.make_option, capi.make_sim
    opt, sim, bk = O(**OPT), S(1000, 50), basket()
    nan, inf = float("nan"), float("inf")
    yield "no opt", (None, sim, bk), {}, "non-NULL"
    yield "no sim", (opt, None, bk), {}, "non-NULL"
    yield "no basket", (opt, sim, None), {}, "non-NULL"
    yield "no res", (opt, sim, bk), dict(res=False), "non-NULL"
    for d in (0, -1, 9):
        b = basket()
        b.n_assets = d
        yield f"n_assets {d}", (opt, sim, b), {}, "n_assets"
    for k in (-1, 4):
        b = basket()
        b.kind = k
        yield f"kind {k}", (opt, sim, b), {}, "kind"
    for p in (-1, 2):
        yield f"payoff {p}", (opt, sim, basket(payoff=p)), {}, "payoff"
    for x in (-1, 5):
        yield f"barrier {x}", (opt, sim, basket(barrier=x)), {}, "barrier"
    for i in (0, 1):
        yield f"reserved[{i}]", (opt, sim, basket(reserved=(i, 1))), {}, "reserved"
    for x in (0.0, -80.0, nan, inf):
        yield f"S0 {x}", (opt, sim, basket(S0=(1, x))), {}, "S0 > 0"
        yield f"v {x}", (opt, sim, basket(v=(2, x))), {}, "v > 0"
    for x in (nan, inf, -inf):
        yield f"w {x}", (opt, sim, basket(kind=capi.BASKET_ARITHMETIC, w=(1, x))), {}, "not finite"
    for kind in (capi.BASKET_BEST_OF, capi.BASKET_WORST_OF):
        for x in (0.0, -0.01):
            yield f"kind {kind} w {x}", (opt, sim, basket(kind=kind, w=(2, x))), {}, "weight > 0"
    for kind in (capi.BASKET_ARITHMETIC, capi.BASKET_GEOMETRIC):
        b = basket(kind=kind)
        for j in range(3):
            b.w[j] = 0.0
        yield f"kind {kind} all weights 0", (opt, sim, b), {}, "weight is 0"
    for K in (nan, inf, -1.0):
        yield f"K {K}", (O(**dict(OPT, K=K)), sim, bk), {}, "finite K >= 0"
    yield "diagonal", (opt, sim, basket(corr=(9, 1.0 + 2.0 ** -52))), {}, "exactly 1"
    yield "asymmetric", (opt, sim, basket(corr=(8 * 2 + 1, 0.6 + 2.0 ** -53))), {}, "symmetric"
    b = basket()
    b.corr[1] = b.corr[8] = 1.5
    yield "beyond 1", (opt, sim, b), {}, "beyond"
    b = basket()
    b.corr[1] = b.corr[8] = nan
    yield "nan", (opt, sim, b), {}, "symmetric"
    for rho in (1.0, -1.0):
        b = basket(d=2)
        b.corr[1] = b.corr[8] = rho
        yield f"rho {rho}", (opt, sim, b), {}, "positive definite"
    b = basket()   # every entry within +-1, no such three variables
    for j, k, rho in ((0, 1, 0.9), (0, 2, 0.9), (1, 2, -0.9)):
        b.corr[8 * j + k] = b.corr[8 * k + j] = rho
    yield "indefinite", (opt, sim, b), {}, "positive definite"
    for kind in (capi.BASKET_ARITHMETIC, capi.BASKET_GEOMETRIC):
        yield f"barrier with kind {kind}", (opt, sim, basket(kind=kind, barrier=capi.BASKET_DOWN_OUT)), {}, "barrier needs"
    for B in (0.0, -1.0, nan):
        yield f"B {B}", (O(**dict(OPT, B=B)), sim, basket(barrier=capi.BASKET_DOWN_IN)), {}, "B must be positive"
    for barrier, B in ((capi.BASKET_DOWN_OUT, 1.0), (capi.BASKET_DOWN_IN, 1.2), (capi.BASKET_UP_OUT, 1.0),
                       (capi.BASKET_UP_IN, 0.8)):
        yield f"barrier {barrier} at {B}", (O(**dict(OPT, B=B)), sim, basket(barrier=barrier)), {}, "live side"
    yield "use_window", (O(**OPT, use_window=1), sim, bk), {}, "window"
    yield "P1", (O(**OPT, P1=1), sim, bk), {}, "window"
    yield "P2", (O(**OPT, P2=3), sim, bk), {}, "window"
    yield "Ik", (O(**OPT, Ik=2), sim, bk), {}, "window"
    yield "Sk", (O(**OPT, Sk=95.0), sim, bk), {}, "Sk"
    yield "Tk", (O(**OPT, Tk=5), sim, bk), {}, "Tk"
    yield "dt", (O(**OPT, dt=0.01), sim, bk), {}, "dt"
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE, capi.FLAG_PRODUCT_FORM,
                  capi.FLAG_LOG_SPACE | capi.FLAG_ANTITHETIC, 32):
        yield f"flags {flags}", (opt, S(1000, 50, flags=flags), bk), {}, "flags"
    # what mcamd_price_paths refuses on sim (and on T and r)
    yield "precision", (opt, S(1000, 50, precision=16), bk), {}, "precision"
    yield "n_steps 0", (opt, S(1000, 0), bk), {}, "n_steps"
    yield "shard overflow", (opt, S(1 << 63, 50, path_offset=(1 << 64) - 10, n_paths_local=100), bk), {}, "overflows"
    yield "T = 0", (O(**dict(OPT, T=0.0)), sim, bk), {}, "T > 0"
    yield "r nan", (O(**dict(OPT, r=nan)), sim, bk), {}, "finite"
    yield "exponent range", (O(**dict(OPT, T=100.0)), S(1000, 50), basket(v=(2, 100.0))), {}, "exponent range"


@pytest.mark.parametrize("case", list(refusals()), ids=lambda c: c[0])
def test_refusals_before_the_context_is_looked_at(lib, case):
    _, args, kw, words = case
    rc, msg = price(lib, *args, **kw)
    assert rc == capi.ERR_INVALID and words in msg and "ctx" not in msg, msg
    if kw.get("res", True):   # the enqueue form shares the checks
        ref = lambda x: None if x is None else C.byref(x)
        rc = lib.mcamd_price_basket_enqueue(None, ref(args[0]), ref(args[1]), ref(args[2]), None, None)
        assert rc == capi.ERR_INVALID and words in lib.mcamd_last_error().decode()


ACCEPTED = [(kind, capi.BASKET_NO_BARRIER, 0.0) for kind in br.KINDS] + \
           [(kind, barrier, br.LEVEL[barrier]) for kind in (br.BEST_OF, br.WORST_OF) for barrier in br.BARRIERS]


@pytest.mark.parametrize("kind,barrier,B", ACCEPTED)
@pytest.mark.parametrize("d,flags,prec", [(1, 0, capi.F64), (8, capi.FLAG_LOG_SPACE, capi.F32)])
def test_accepted_requests_reach_the_missing_context(lib, kind, barrier, B, d, flags, prec):
    sim = capi.make_sim(1000, 50, prec, flags=flags, path_offset=3, n_paths_local=0)
    for payoff in (capi.PAYOFF_CALL, capi.PAYOFF_PUT):
        # opt->S0 and opt->v are ignored whatever they hold, opt->B without a barrier, K = 0 is allowed
        opt = capi.make_option(**dict(OPT, S0=-5.0, v=float("nan"), B=B if barrier else -3.0, K=0.0 if d == 8 else 1.0))
        rc, msg = price(lib, opt, sim, basket(d, kind, payoff, barrier))
        assert rc == capi.ERR_INVALID and "ctx" in msg, msg


def test_entries_beyond_n_assets_are_ignored(lib):
    b = basket(d=2)
    for q in range(64):
        if q // 8 >= 2 or q % 8 >= 2:
            b.corr[q] = float("nan")
    for j in range(2, 8):
        b.S0[j] = b.v[j] = b.w[j] = float("nan")
    rc, msg = price(lib, capi.make_option(**OPT), capi.make_sim(1000, 5), b)
    assert rc == capi.ERR_INVALID and "ctx" in msg, msg


# ---- the closed forms ----------------------------------------------------------------------------------------------------

def test_geometric_closed_form(lib):
    for K in (70.0, 80.0, 95.0):     # one asset with w = 1: Black and Scholes
        b = capi.make_basket([80.0], [0.15], [1.0], [[1.0]], capi.BASKET_GEOMETRIC)
        want = capi.bs_call_f64(80.0, K, br.T_, br.R, 0.15)
        assert abs(capi.basket_geometric_price_f64(b, K, br.T_, br.R) - want) <= 1e-13 * want
    for d in range(2, 9):
        S0, v, corr = br.inputs(d)
        for w in (np.full(d, 1.0 / d), np.linspace(-0.5, 1.5, d)):
            for K in (60.0, 100.0, 140.0):
                call = capi.basket_geometric_price_f64(capi.make_basket(S0, v, w, corr, capi.BASKET_GEOMETRIC), K, br.T_, br.R)
                put = capi.basket_geometric_price_f64(
                    capi.make_basket(S0, v, w, corr, capi.BASKET_GEOMETRIC, capi.PAYOFF_PUT), K, br.T_, br.R)
                for got, is_put in ((call, False), (put, True)):
                    want = br.geometric_lognormal(S0, v, w, corr, K, br.T_, br.R, is_put)
                    assert abs(got - want) <= 1e-12 * max(want, 1.0), (d, K, is_put, got, want)
                # put-call parity: C - P = e^{-rT} (E[A_T] - K), and K = 0 is that forward
                fwd = capi.basket_geometric_price_f64(capi.make_basket(S0, v, w, corr, capi.BASKET_GEOMETRIC), 0.0, br.T_, br.R)
                assert abs((call - put) - (fwd - K * math.exp(-br.R * br.T_))) <= 1e-11 * max(fwd, K)


def test_exchange_closed_form(lib):
    S0, v, corr = br.inputs(2)
    for a1, a2, rho, T in ((80.0, 90.0, 0.6, 1.0), (90.0, 80.0, 0.6, 1.0), (1.0, 1.0, -0.5, 0.25), (100.0, 95.0, 0.0, 2.0)):
        got = capi.exchange_price_f64(a1, a2, T, v[0], v[1], rho)
        # max(A1, A2) = A2 + (A1 - A2)+, and e^{-rT} E[A2] = a2: the best-of-two call struck at 0, by quadrature
        best = br.rainbow2_by_quadrature(a1, a2, v[0], v[1], rho, 0.0, T, br.R, True, False)
        assert abs(got - (best - a2)) <= 1e-9 * a1, (a1, a2, rho, got, best - a2)
        # parity: (A1 - A2)+ - (A2 - A1)+ = A1 - A2
        back = capi.exchange_price_f64(a2, a1, T, v[1], v[0], rho)
        assert abs((got - back) - (a1 - a2)) <= 1e-13 * max(a1, a2)
    # best + worst = A1 + A2 whatever K = 0: the worst-of-two by quadrature is a2 less the exchange the other way
    worst = br.rainbow2_by_quadrature(80.0, 90.0, v[0], v[1], 0.6, 0.0, 1.0, br.R, False, False)
    assert abs(worst - (80.0 - capi.exchange_price_f64(80.0, 90.0, 1.0, v[0], v[1], 0.6))) <= 1e-7


def test_closed_form_refusals(lib):
    p = C.c_double(7.0)
    S0, v, corr = br.inputs(2)
    ok = capi.make_basket(S0, v, [0.5, 0.5], corr, capi.BASKET_GEOMETRIC)
    assert lib.mcamd_basket_geometric_price_f64(C.byref(ok), 100.0, 1.0, 0.05, C.byref(p)) == capi.OK and p.value > 0
    assert lib.mcamd_basket_geometric_price_f64(None, 100.0, 1.0, 0.05, C.byref(p)) == capi.ERR_INVALID
    assert lib.mcamd_basket_geometric_price_f64(C.byref(ok), 100.0, 1.0, 0.05, None) == capi.ERR_INVALID
    for K, T, r in ((-1.0, 1.0, 0.05), (float("nan"), 1.0, 0.05), (100.0, 0.0, 0.05), (100.0, 1.0, float("inf"))):
        assert lib.mcamd_basket_geometric_price_f64(C.byref(ok), K, T, r, C.byref(p)) == capi.ERR_INVALID and p.value == 0
    for edit in (dict(S0=(0, -1.0)), dict(v=(1, 0.0)), dict(w=(0, float("nan"))), dict(corr=(1, 0.7)), dict(corr=(0, 0.99))):
        bad = basket(d=2, kind=capi.BASKET_GEOMETRIC, **edit)
        assert lib.mcamd_basket_geometric_price_f64(C.byref(bad), 100.0, 1.0, 0.05, C.byref(p)) == capi.ERR_INVALID
    for n, payoff in ((0, 0), (9, 0), (2, 2)):
        bad = basket(d=2, kind=capi.BASKET_GEOMETRIC, payoff=payoff)
        bad.n_assets = n
        assert lib.mcamd_basket_geometric_price_f64(C.byref(bad), 100.0, 1.0, 0.05, C.byref(p)) == capi.ERR_INVALID
    rho1 = basket(d=2, kind=capi.BASKET_GEOMETRIC)
    rho1.corr[1] = rho1.corr[8] = 1.0
    assert lib.mcamd_basket_geometric_price_f64(C.byref(rho1), 100.0, 1.0, 0.05, C.byref(p)) == capi.ERR_INVALID
    nan = float("nan")
    for args in ((0.0, 1, 1, .2, .2, .5), (1, -1.0, 1, .2, .2, .5), (1, 1, 0.0, .2, .2, .5), (1, 1, 1, 0.0, .2, .5),
                 (1, 1, 1, .2, nan, .5), (1, 1, 1, .2, .2, 1.0), (1, 1, 1, .2, .2, -1.0), (1, 1, 1, .2, .2, nan),
                 (float("inf"), 1, 1, .2, .2, .5)):
        assert lib.mcamd_exchange_price_f64(*[float(x) for x in args], C.byref(p)) == capi.ERR_INVALID and p.value == 0
    assert lib.mcamd_exchange_price_f64(1.0, 1.0, 1.0, 0.2, 0.2, 0.5, None) == capi.ERR_INVALID


# ---- the restated estimator against the closed forms ---------------------------------------------------------------------

MC_SEED, MC_PATHS = 20261018, 400_000   # committed: every |MC - closed form| below lies within 4 SE with these


@pytest.fixture(scope="module")
def normals():
    """[32, MC_PATHS] normals of the oracle's Philox generator: enough for 4 steps of 8 assets"""
    from oracle import pyoracle as o
    return o.generate_normals(MC_SEED, 32 * MC_PATHS, 64).reshape(32, MC_PATHS)


@pytest.mark.parametrize("n_steps", [1, 4])
def test_restated_estimator_converges_to_the_closed_forms(lib, normals, n_steps):
    """the exact law at the step ends: one step and four steps both reproduce the terminal closed forms"""
    disc = math.exp(-br.R * br.T_)
    rows = []
    for d in (2, 5, 8):
        S0, v, corr = br.inputs(d)
        w, K = br.weights(br.GEOMETRIC, d)
        for payoff in (br.CALL, br.PUT):
            want = capi.basket_geometric_price_f64(capi.make_basket(S0, v, w, corr, br.GEOMETRIC, payoff), K, br.T_, br.R)
            rows.append((f"geometric d {d} payoff {payoff}", want,
                         br.samples(normals, n_steps, S0, v, w, corr, K, br.T_, br.R, br.GEOMETRIC, payoff)))
    S0, v, corr = br.inputs(2)
    rows.append(("exchange", capi.exchange_price_f64(S0[0], S0[1], br.T_, v[0], v[1], corr[0][1]),
                 br.samples(normals, n_steps, S0, v, [1.0, -1.0], corr, 0.0, br.T_, br.R, br.ARITHMETIC, br.CALL)))
    w, K = br.weights(br.BEST_OF, 2)
    for kind in (br.BEST_OF, br.WORST_OF):
        for payoff in (br.CALL, br.PUT):
            want = br.rainbow2_by_quadrature(1.0, 1.0, v[0], v[1], corr[0][1], K, br.T_, br.R, kind == br.BEST_OF,
                                             payoff == br.PUT)
            rows.append((f"kind {kind} payoff {payoff}", want,
                         br.samples(normals, n_steps, S0, v, w, corr, K, br.T_, br.R, kind, payoff)))
    for name, want, s in rows:
        y = s["y"]
        got, se = disc * y.mean(), disc * y.std(ddof=1) / math.sqrt(y.size)
        print(f"n_steps {n_steps} {name}: closed {want:.6f} MC {got:.6f} SE {se:.6f} ({(got - want) / se:+.2f} SE)")
        assert se > 0 and abs(got - want) <= 4.0 * se, (name, got, want, se)


def test_restatement_precisions_agree():
    """the three dtypes walk the same paths; a terminal sample is continuous in every input, so no path is left out"""
    rng = np.random.default_rng(3)
    z = rng.standard_normal((8 * 12, 5000)).astype(np.float32).astype(np.float64)
    for d in (1, 3, 8):
        S0, v, corr = br.inputs(d)
        for kind in br.KINDS:
            w, K = br.weights(kind, d)
            y = {t: br.samples(z, 12, S0, v, w, corr, K, br.T_, br.R, kind, br.PUT, dtype=t)["y"]
                 for t in (np.float64, np.longdouble, np.float32)}
            assert np.abs(y[np.float64] - y[np.longdouble].astype(np.float64)).max() <= 1e-11
            assert np.abs(y[np.float64] - y[np.float32]).max() <= 2e-3
            assert (y[np.float64] > 0).any()


def test_in_plus_out_is_the_unmonitored_sample():
    z = br.stream(br.F64)
    S0, v, corr = br.inputs(3)
    w, K = br.weights(br.WORST_OF, 3)
    plain = br.samples(z, 50, S0, v, w, corr, K, br.T_, br.R, br.WORST_OF, br.PUT)["y"]
    out = br.samples(z, 50, S0, v, w, corr, K, br.T_, br.R, br.WORST_OF, br.PUT, br.DOWN_OUT, 0.8)
    inn = br.samples(z, 50, S0, v, w, corr, K, br.T_, br.R, br.WORST_OF, br.PUT, br.DOWN_IN, 0.8)
    assert np.array_equal(out["y"] + inn["y"], plain) and np.array_equal(out["live"], inn["live"])
    assert 0.05 < out["hit"].mean() < 0.95 and (out["y"][out["hit"]] == 0).all() and (inn["y"][~inn["hit"]] == 0).all()


# ---- what the GPU test's tolerance and exclusions are made of ------------------------------------------------------------

def measure(prec, cases, where=br.SHALLOW):
    """(largest restatement difference, its case, largest share of paths left out) over the cases, each checked for the
    cap, for no path left out without a barrier and for samples that are finite and not all zero"""
    worst, worst_case, left_out = 0.0, None, 0.0
    for case in cases:
        want, own, keep, spread = br.compare(prec, *case, where)
        if spread > worst:
            worst, worst_case = spread, case
        left_out = max(left_out, 1.0 - keep.mean())
        assert 1.0 - keep.mean() <= br.CAP, (prec, case, 1.0 - keep.mean())
        assert case[2] != br.NO_BARRIER or keep.all()
        assert np.isfinite(want).all() and (want != 0).any(), (prec, case)
    return worst, worst_case, left_out


def test_elementwise_spread_and_exclusions_of_the_gpu_cases():
    """Restatement against restatement on the inputs and the 480 cases of test 1 of tests/test_gpu_basket.py with d in
    {1, 2, 3, 5, 8}: the recorded spreads (basket_restate.SPREAD) bound what is measured here, and no
    barrier case leaves out more than CAP of its paths within MARGIN of the barrier."""
    for prec in (br.F64, br.F32):
        worst, worst_case, left_out = measure(prec, br.PLAIN_CASES + br.BARRIER_CASES)
        print(f"prec {prec}: largest restatement difference {worst:.3e} at {worst_case} (recorded {br.SPREAD[prec]:.1e}), "
              f"largest share left out {left_out:.4f} (cap {br.CAP})")
        assert 0.0 < worst <= br.SPREAD[prec] <= 2.0 * worst, (prec, worst, br.SPREAD[prec])


@pytest.mark.parametrize("prec", [br.F64, br.F32])
@pytest.mark.parametrize("name", ["more widths", "deep"])
def test_elementwise_spread_and_exclusions_of_the_added_gpu_cases(prec, name):
    """The same measurement on the other cases of test 1 — d in {4, 6, 7} on the same inputs, and every d at 7 steps
    on the deep inputs: they stay below the record, which is why they take its tolerance.
    Measured on an x86-64 CPU (80-bit longdouble): 3.11e-13 / 1.99e-4 (fp64 / fp32) on the widths, 3.39e-13 / 2.12e-4 on
    the deep inputs; at most 0.46 % and 0.12 % of a case's paths left out."""
    cases, where = (br.MORE_CASES, br.SHALLOW) if name == "more widths" else (br.DEEP_CASES, br.DEEP)
    worst, worst_case, left_out = measure(prec, cases, where)
    print(f"prec {prec} {name}: largest restatement difference {worst:.3e} at {worst_case} (record {br.SPREAD[prec]:.1e}), "
          f"largest share left out {left_out:.4f} (cap {br.CAP})")
    assert 0.0 < worst <= br.SPREAD[prec], (prec, name, worst, br.SPREAD[prec])


@pytest.mark.parametrize("prec", [br.F64, br.F32])
def test_deep_normals_are_those_of_neither_shallow_word(prec):
    """What makes the deep cases worth running: the deep normals share nothing with the streams a dropped high word
    of the path id or of the seed lands on (tests/deep_inputs.py)."""
    check_deep_draws_differ(lambda seed, first: br.stream(prec, seed, first, 64, max(br.DS) * br.DEEP_STEPS))
