"""CPU-only checks of the cliquet call (include/mcamd.h, mcamd_price_cliquet): declarations and struct layout; every
refusal that needs neither the surface nor the context, given no surface and no context; and the host closed form
mcamd_cliquet_price_f64 against the float64 restatement (tests/cliquet_restate.py) on numpy normals within 4 SE, against
a Gauss-Legendre quadrature of the one-period payoff with panel edges on the kinks, and against mcamd_bs_price_f64 for a
single period with one bound.  No kernels run here."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import cliquet_restate as cr

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcamd_price_cliquet", "mcamd_price_cliquet_enqueue", "mcamd_cliquet_price_f64")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


def header():
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        return f.read()


def test_header_declares_the_calls_and_the_structs(lib):
    text = header()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert re.search(r"\}\s*mcamd_cliquet\s*;", text) and re.search(r"\}\s*mcamd_cliquet_result\s*;", text)
    assert re.search(r"#define\s+MCAMD_ABI_VERSION\s+5\b", text) and lib.mcamd_abi_version() == 5
    assert "first carried by the build that ships csrc/cliquet.hip" in text
    assert not re.search(r"mcamd_group_\w*cliquet", text)
    for k, name in enumerate(("SUM", "COMPOUND", "VARIANCE")):
        assert re.search(rf"#define\s+MCAMD_CLIQUET_{name}\s+{k}\b", text) and getattr(capi, "CLIQUET_" + name) == k
    build = importlib.import_module("monte-carlo-project-cuda_amd.build")
    assert "cliquet.hip" in build.SOURCES and "cliquet.hpp" in build.HEADERS


def test_structs_match_the_header():
    # static_assert(sizeof(mcamd_cliquet) == 56 && sizeof(mcamd_cliquet_result) == 96) in csrc/capi_localvol.cpp
    Q, R = capi.Cliquet, capi.CliquetResult
    assert C.sizeof(Q) == 56 and C.sizeof(R) == 96
    assert [(k, getattr(Q, k).offset) for k, _ in Q._fields_] == [
        ("kind", 0), ("reset_every", 4), ("first_period", 8), ("reserved", 12), ("local_floor", 16), ("local_cap", 24),
        ("global_floor", 32), ("global_cap", 40), ("q", 48)]
    assert [(k, getattr(R, k).offset) for k, _ in R._fields_] == [
        ("price", 0), ("std_err", 8), ("ci_lo", 16), ("ci_hi", 24), ("sum", 32), ("sumsq", 40), ("n", 48), ("n_floored", 56),
        ("n_capped", 64), ("work_steps", 72), ("kernel_ms", 80), ("total_ms", 84), ("grid", 88), ("block", 92)]
    text = header()
    for struct, cls in (("mcamd_cliquet", Q), ("mcamd_cliquet_result", R)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\}", text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in re.findall(r"\w+\s+([\w\s,]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
        assert names == [k for k, _ in cls._fields_], struct   # the same fields in the same order
    c = capi.make_cliquet(capi.CLIQUET_COMPOUND, 4, 2, -0.03, 0.05, 0.0, 0.25, 0.03)
    assert (c.kind, c.reset_every, c.first_period, c.reserved) == (1, 4, 2, 0)
    assert (c.local_floor, c.local_cap, c.global_floor, c.global_cap, c.q) == (-0.03, 0.05, 0.0, 0.25, 0.03)
    d = capi.make_cliquet()
    assert (d.kind, d.reset_every, d.first_period, d.local_floor, d.local_cap, d.global_floor, d.global_cap, d.q) == \
        (0, 1, 1, -INF, INF, -INF, INF, 0.0)


def test_the_six_kernels_use_no_scratch():
    """the cross-compile alone: cliquet_kernel<T, KIND> for two precisions and three kinds, no private segment, no
    spilled register, and static LDS that leaves the dynamic table 16-byte aligned (tools/isa_diff.py reads the figures)"""
    from importlib import util as ilu
    spec = ilu.spec_from_file_location("isa_diff_for_cliquet", os.path.join(ROOT, "tools", "isa_diff.py"))
    isa = ilu.module_from_spec(spec)
    spec.loader.exec_module(isa)
    kernels = isa.kernels_of(ROOT, "cliquet.hip")
    names = sorted(k for k in kernels if "cliquet_kernel" in k)
    assert len(names) == 6 == len(kernels), sorted(kernels)
    assert {re.search(r"cliquet_kernelI([fd])Li(\d)E", k).groups() for k in names} == \
        {(t, str(kind)) for t in "fd" for kind in cr.KINDS}
    for k in names:
        ops, fig = kernels[k]
        print(k, fig)
        assert fig["scratch"] == 0 and fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0 and fig["agpr"] == 0, (k, fig)
        assert fig["lds"] % 16 == 0, (k, fig)
        # the exponential's instruction is in the fp32 SUM and COMPOUND kernels only, and only SUM has it in the loop
        if "If" in k:
            assert (ops["v_exp_f32_e32"] + ops["v_exp_f32_e64"] > 0) == ("Li2E" not in k), (k, ops["v_exp_f32_e32"])


# ---- refusals ------------------------------------------------------------------------------------------------------

def price(lib, opt, sim, cq, res=True, enqueue=False):
    out = capi.CliquetResult()
    ref = lambda x: None if x is None else C.byref(x)
    if enqueue:
        rc = lib.mcamd_price_cliquet_enqueue(None, ref(opt), ref(sim), ref(cq), None, None, None)
    else:
        rc = lib.mcamd_price_cliquet(None, ref(opt), ref(sim), ref(cq), None, None, C.byref(out) if res else None)
    return rc, lib.mcamd_last_error().decode()


BASE = dict(S0=100.0, v=NAN, K=NAN, B=NAN, r=0.1, T=1.0)   # opt->v, K and B are ignored


def cliquet(kind=capi.CLIQUET_SUM, reset_every=4, first_period=1, **kw):
    if kind != capi.CLIQUET_VARIANCE:
        kw = dict(dict(local_floor=-0.03, local_cap=0.05, global_floor=0.0, global_cap=0.25), **kw)
    return capi.make_cliquet(kind, reset_every, first_period, **dict(dict(q=0.03), **kw))


def refusals():
    O, S = capi.make_option, capi.make_sim
    opt, sim, cq = O(**BASE), S(1000, 12), cliquet()
    yield "no opt", (None, sim, cq), {}, "non-NULL"
    yield "no sim", (opt, None, cq), {}, "non-NULL"
    yield "no cliquet", (opt, sim, None), {}, "non-NULL"
    yield "no res", (opt, sim, cq), dict(res=False), "non-NULL"
    for kind in (-1, 3):
        yield f"kind {kind}", (opt, sim, cliquet(kind)), {}, "kind"
    bad = cliquet()
    bad.reserved = 1
    yield "reserved", (opt, sim, bad), {}, "reserved"
    yield "reset_every 0", (opt, sim, cliquet(reset_every=0)), {}, "reset_every"
    yield "reset_every 5 of 12", (opt, sim, cliquet(reset_every=5)), {}, "reset_every"
    yield "reset_every 24 of 12", (opt, sim, cliquet(reset_every=24)), {}, "reset_every"
    yield "first_period 0", (opt, sim, cliquet(first_period=0)), {}, "first_period"
    yield "first_period 4 of 3", (opt, sim, cliquet(first_period=4)), {}, "first_period"
    for field in ("local_floor", "local_cap", "global_floor", "global_cap"):
        yield f"{field} NaN", (opt, sim, cliquet(**{field: NAN})), {}, "NaN"
    yield "local_floor = local_cap", (opt, sim, cliquet(local_floor=0.05)), {}, "local_floor"
    yield "local_floor > local_cap", (opt, sim, cliquet(local_floor=0.06)), {}, "local_floor"
    yield "local bounds both +inf", (opt, sim, cliquet(local_floor=INF, local_cap=INF)), {}, "local_floor"
    yield "global_floor = global_cap", (opt, sim, cliquet(global_floor=0.25)), {}, "global_floor"
    yield "global_floor > global_cap", (opt, sim, cliquet(global_floor=0.3)), {}, "global_floor"
    yield "global bounds both -inf", (opt, sim, cliquet(global_floor=-INF, global_cap=-INF)), {}, "global_floor"
    yield "compound local_floor < -1", (opt, sim, cliquet(capi.CLIQUET_COMPOUND, local_floor=-1.5)), {}, "compounding"
    yield "compound local_floor -inf", (opt, sim, cliquet(capi.CLIQUET_COMPOUND, local_floor=-INF)), {}, "compounding"
    yield "compound local_cap = -1", (opt, sim, cliquet(capi.CLIQUET_COMPOUND, local_floor=-INF, local_cap=-1.0)), {}, \
        "compounding"
    yield "variance local_floor", (opt, sim, cliquet(capi.CLIQUET_VARIANCE, local_floor=-0.5)), {}, "no local bounds"
    yield "variance local_cap", (opt, sim, cliquet(capi.CLIQUET_VARIANCE, local_cap=0.5)), {}, "no local bounds"
    for value in (NAN, INF, -INF):
        yield f"q = {value}", (opt, sim, cliquet(q=value)), {}, "dividend yield"
    # the other opt fields must be 0
    yield "use_window", (O(**BASE, use_window=1), sim, cq), {}, "window"
    yield "P1", (O(**BASE, P1=1), sim, cq), {}, "window"
    yield "P2", (O(**BASE, P2=3), sim, cq), {}, "window"
    yield "Ik", (O(**BASE, Ik=2), sim, cq), {}, "window"
    yield "Sk", (O(**BASE, Sk=95.0), sim, cq), {}, "Sk"
    yield "Tk", (O(**BASE, Tk=5), sim, cq), {}, "Tk"
    yield "dt", (O(**BASE, dt=0.01), sim, cq), {}, "dt"
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE, capi.FLAG_PRODUCT_FORM,
                  capi.FLAG_LOG_SPACE | capi.FLAG_ANTITHETIC, capi.FLAG_LOG_SPACE | capi.FLAG_PRODUCT_FORM, 32):
        yield f"flags {flags}", (opt, S(1000, 12, flags=flags), cq), {}, "flags"
    # what mcamd_price_localvol refuses of sim
    yield "precision", (opt, S(1000, 12, precision=16), cq), {}, "precision"
    yield "n_steps 0", (opt, S(1000, 0), cliquet(reset_every=1)), {}, "n_steps"
    yield "shard overflow", (opt, S(1 << 63, 12, path_offset=(1 << 64) - 10, n_paths_local=100), cq), {}, "overflows"
    yield "exponent range", (O(**dict(BASE, T=100.0)), sim, cliquet(q=-1e4)), {}, "exponent range"
    yield "T = 0", (O(**dict(BASE, T=0.0)), sim, cq), {}, "T > 0"
    yield "r = nan", (O(**dict(BASE, r=NAN)), sim, cq), {}, "finite"
    # then the surface
    yield "no surface", (opt, sim, cq), {}, "surface must be non-NULL"


@pytest.mark.parametrize("case", list(refusals()), ids=lambda c: c[0])
def test_refusals_before_the_surface_and_the_context_are_looked_at(lib, case):
    """Every case but the last is wrong in one way only and is given no surface and no context: the message names the
    request's fault, so the refusal came before the surface and the context."""
    _, args, kw, words = case
    rc, msg = price(lib, *args, **kw)
    assert rc == capi.ERR_INVALID and words in msg, msg
    if kw.get("res", True):   # the enqueue form shares the checks
        rc, msg = price(lib, *args, enqueue=True, **kw)
        assert rc == capi.ERR_INVALID and words in msg, msg


@pytest.mark.parametrize("kind", cr.KINDS)
@pytest.mark.parametrize("flags,prec", [(0, capi.F64), (capi.FLAG_LOG_SPACE, capi.F32)])
def test_accepted_requests_reach_the_surface(lib, kind, flags, prec):
    sim = capi.make_sim(1000, 12, prec, flags=flags, path_offset=3, n_paths_local=0)
    shapes = [dict(), dict(reset_every=1, first_period=12), dict(reset_every=12), dict(reset_every=3, first_period=4)]
    if kind != capi.CLIQUET_VARIANCE:
        shapes += [dict(local_floor=-1.0, local_cap=INF, global_cap=INF), dict(local_floor=0.0, local_cap=0.04,
                                                                              global_floor=-INF, global_cap=INF)]
    if kind == capi.CLIQUET_SUM:
        shapes += [dict(local_floor=-INF, local_cap=-1.5)]   # a sum of returns takes any ordered pair
    else:
        shapes += [dict(global_floor=0.0), dict(global_cap=0.06)]
    for kw in shapes:
        rc, msg = price(lib, capi.make_option(**BASE), sim, cliquet(kind, **kw))
        assert rc == capi.ERR_INVALID and "surface must be non-NULL" in msg, (kw, msg)
    # opt->v, K and B are ignored, and S0 is read by nothing
    for S0, v, K, B in ((NAN, NAN, NAN, NAN), (-1.0, -1.0, -1.0, -1.0), (0.0, 0.0, INF, INF)):
        rc, msg = price(lib, capi.make_option(**dict(BASE, S0=S0, v=v, K=K, B=B)), sim, cliquet(kind))
        assert rc == capi.ERR_INVALID and "surface must be non-NULL" in msg, msg


def test_closed_form_refusals(lib):
    ok = dict(kind=capi.CLIQUET_SUM, T=1.0, r=0.1, q=0.03, period_vol=[0.2, 0.3], first_period=1, local_floor=-0.03,
              local_cap=0.05)
    assert capi.cliquet_price(**ok) > 0
    for name, kw, words in (("kind", dict(kind=3), "kind"), ("T = 0", dict(T=0.0), "T > 0"), ("T inf", dict(T=INF), "T > 0"),
                            ("r", dict(r=NAN), "finite"), ("q", dict(q=INF), "finite"),
                            ("no periods", dict(period_vol=[]), "n_periods"), ("first 0", dict(first_period=0), "first_period"),
                            ("first 3 of 2", dict(first_period=3), "first_period"),
                            ("vol 0", dict(period_vol=[0.2, 0.0]), "period_vol[1]"),
                            ("vol nan", dict(period_vol=[NAN, 0.2]), "period_vol[0]"),
                            ("floor nan", dict(local_floor=NAN), "NaN"), ("ordered", dict(local_floor=0.05), "local_floor"),
                            ("compound", dict(kind=capi.CLIQUET_COMPOUND, local_floor=-2.0), "compounding"),
                            ("variance", dict(kind=capi.CLIQUET_VARIANCE), "no local bounds")):
        with pytest.raises(capi.McamdError) as e:
            capi.cliquet_price(**dict(ok, **kw))
        assert e.value.code == capi.ERR_INVALID and words in str(e.value), (name, str(e.value))
    out = C.c_double(7.0)
    vols = (C.c_double * 2)(0.2, 0.3)
    assert lib.mcamd_cliquet_price_f64(0, 1.0, 0.1, 0.0, 2, 1, None, -INF, INF, C.byref(out)) == capi.ERR_INVALID
    assert lib.mcamd_cliquet_price_f64(0, 1.0, 0.1, 0.0, 2, 1, vols, -INF, INF, None) == capi.ERR_INVALID


# ---- the closed form -----------------------------------------------------------------------------------------------

R, Q_DIV, T_ = 0.1, 0.03, 1.0
BOUNDS = ((-0.03, 0.05), (0.0, 0.04), (-1.0, INF), (-INF, INF))


def time_only(vols):
    """a surface whose volatility depends on the slice alone"""
    return (len(vols), 2, -1.0, 1.0), [[v, v] for v in vols]


_walk = {}


def numpy_normals(n_steps):
    if n_steps not in _walk:
        _walk[n_steps] = np.random.default_rng(2022 + n_steps).standard_normal((n_steps, 1 << 20))
    return _walk[n_steps]


def mean_and_se(y):
    y = np.asarray(y, dtype=np.float64)
    return math.exp(-R * T_) * y.mean(), math.exp(-R * T_) * y.std(ddof=1) / math.sqrt(y.size)


@pytest.mark.parametrize("n_steps,reset_every,vols,period_vol", [
    (12, 4, (0.15, 0.30, 0.20), (0.15, 0.30, 0.20)),
    (4, 4, (0.15, 0.30), (math.sqrt((0.15 ** 2 + 0.30 ** 2) / 2),))])   # one period over two slices: the rms volatility
def test_closed_form_against_the_restatement_on_numpy_normals(lib, n_steps, reset_every, vols, period_vol):
    """2^20 float64 paths on a time-only surface: within 4 SE for every kind, first_period 1 and the last period"""
    grid, sigma = time_only(vols)
    z = numpy_normals(n_steps)
    M = n_steps // reset_every
    for first in sorted({1, M}):
        for kind, bounds in [(cr.SUM, b) for b in BOUNDS[:3]] + [(cr.COMPOUND, b) for b in BOUNDS[:3]] + \
                            [(cr.VARIANCE, BOUNDS[3])]:
            got = cr.samples(z, T_, R, Q_DIV, grid, sigma, kind, reset_every, first, *bounds)
            price_, se = mean_and_se(got["y"])
            want = capi.cliquet_price(kind, T_, R, Q_DIV, period_vol, first, *bounds)
            print(f"n_steps {n_steps} kind {kind} first {first} bounds {bounds}: closed {want:.7f} restated {price_:.7f} "
                  f"SE {se:.2e} ({(price_ - want) / se:+.2f} SE)")
            assert se > 0 and abs(price_ - want) <= 4.0 * se, (kind, first, bounds, price_, want, se)
            assert np.array_equal(got["y"], got["A"]) and not got["floored"].any() and not got["capped"].any()


def quadrature(payoff, mean, s, kinks):
    """E[payoff(D)], D ~ N(mean, s^2): 64-point Gauss-Legendre on panels whose edges lie on the kinks"""
    x, w = np.polynomial.legendre.leggauss(64)
    lo, hi = mean - 12.0 * s, mean + 12.0 * s
    inner = sorted(k for k in kinks if lo < k < hi)
    edges = [lo] + inner + [hi]
    # split the panels further so that none is wider than 2 s
    fine = []
    for a, b in zip(edges[:-1], edges[1:]):
        m = max(1, int(math.ceil((b - a) / (2.0 * s))))
        fine += [a + (b - a) * j / m for j in range(m)]
    fine.append(hi)
    total = 0.0
    for a, b in zip(fine[:-1], fine[1:]):
        d = 0.5 * (b - a) * x + 0.5 * (a + b)
        dens = np.exp(-0.5 * ((d - mean) / s) ** 2) / (s * math.sqrt(2.0 * math.pi))
        total += 0.5 * (b - a) * float(np.sum(w * payoff(d) * dens))
    return total


@pytest.mark.parametrize("floor,cap", BOUNDS + ((-0.5, 0.5), (0.02, 0.03), (-INF, 0.01), (-2.0, -1.5)))
@pytest.mark.parametrize("v,tau", [(0.2, 1.0), (0.35, 0.25), (0.1, 1.0 / 12)])
def test_closed_form_against_quadrature_of_one_period(lib, floor, cap, v, tau):
    mean, s = (R - Q_DIV - 0.5 * v * v) * tau, v * math.sqrt(tau)
    kinks = [math.log1p(b) for b in (floor, cap) if -1.0 < b < INF]
    E = quadrature(lambda d: np.minimum(np.maximum(np.expm1(d), floor), cap), mean, s, kinks)
    want = math.exp(-R * tau) * E
    got = capi.cliquet_price(cr.SUM, tau, R, Q_DIV, [v], 1, floor, cap)
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (got, want)
    if floor >= -1.0:
        assert abs(capi.cliquet_price(cr.COMPOUND, tau, R, Q_DIV, [v], 1, floor, cap) - want) <= 1e-12
    var = quadrature(lambda d: d * d, mean, s, []) / tau
    got = capi.cliquet_price(cr.VARIANCE, tau, R, Q_DIV, [v], 1)
    assert abs(got - math.exp(-R * tau) * var) <= 1e-12, (got, var)


def test_closed_form_over_several_periods_is_the_sum_and_the_product_of_single_periods(lib):
    vols, T, first = (0.15, 0.30, 0.20, 0.25), 2.0, 2
    tau, disc = T / 4, math.exp(-R * T)
    for floor, cap in BOUNDS[:3]:
        E = [math.exp(R * tau) * capi.cliquet_price(cr.SUM, tau, R, Q_DIV, [v], 1, floor, cap) + 1.0 for v in vols]
        assert abs(capi.cliquet_price(cr.SUM, T, R, Q_DIV, vols, first, floor, cap) - disc * sum(e - 1 for e in E[1:])) < 1e-13
        assert abs(capi.cliquet_price(cr.COMPOUND, T, R, Q_DIV, vols, first, floor, cap) - disc * (math.prod(E[1:]) - 1)) < 1e-13
    one = [math.exp(R * tau) * capi.cliquet_price(cr.VARIANCE, tau, R, Q_DIV, [v]) for v in vols]
    assert abs(capi.cliquet_price(cr.VARIANCE, T, R, Q_DIV, vols, first) - disc * sum(one[1:]) / 3) < 1e-13


@pytest.mark.parametrize("k", [0.9, 1.0, 1.1])
def test_single_period_with_one_bound_is_black_scholes(lib, k):
    """a floor at k - 1 alone: (k - 1) + (S_T / S_0 - k)+; a cap at k - 1 alone: S_T / S_0 - 1 - (S_T / S_0 - k)+"""
    v, T = 0.22, 0.75
    call = capi.bs_price_f64(1.0, k, T, R, Q_DIV, v)
    disc, fwd = math.exp(-R * T), math.exp((R - Q_DIV) * T)
    assert abs(capi.cliquet_price(cr.SUM, T, R, Q_DIV, [v], 1, k - 1.0, INF) - (disc * (k - 1.0) + call)) <= 1e-14
    assert abs(capi.cliquet_price(cr.SUM, T, R, Q_DIV, [v], 1, -INF, k - 1.0) - (disc * (fwd - 1.0) - call)) <= 1e-14
