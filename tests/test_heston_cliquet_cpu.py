"""CPU-only checks of the Heston cliquet call (include/mcamd.h, mcamd_price_heston_cliquet).  No kernels run here.

  1. declarations and struct layout; every refusal through both entry points, given no context, unequal dividend yields
     and the COMPOUND bounds among them, and their order; the cross-compile's resource figures for the six kernels;
  2. the host closed form mcamd_heston_cliquet_price_f64: one period against mcamd_heston_price_f64 (1e-10); every
     period of a four-period cliquet, floors and a cap, against an independent scipy.integrate.quad of the textbook
     forward characteristic function (1e-8), forward windows starting at 0, T/4, T/2 and 3T/4; VARIANCE against
     -phi''(0) from mpmath at 30 digits (1e-8 relative; measured 3e-12 .. 4e-10); the discrete-to-continuous gap; the
     step across MCAMD_HESTON_XI_MIN and the deterministic limit; kappa = 0 and rho = +-1; COMPOUND; the refusals;
  3. the restatement (tests/heston_cliquet_restate.py): at xi = 0, kappa = 0 bit-equal to cliquet_restate on a flat
     surface, every kind; one period of SUM without bounds against heston_restate's S_T / S0;
  4. against the closed form by Richardson extrapolation on input N: 2 p(128 steps) - p(64 steps) within
     4 sqrt(4 SE_128^2 + SE_64^2) of it, for the forward-start call (two periods, the second counts, floor 0) and the
     variance swap (four periods), 120k Philox paths per step count;
  5. the precision spread of the restatement on every shape, job and input of the GPU tests, which fixes their
     tolerance, and the share of paths within that tolerance of a global bound (at most 2 % of any case)."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import cliquet_restate as cr
import heston_cases as hc
import heston_cliquet_cases as cases
import heston_cliquet_restate as hq
import heston_restate as hr
from deep_inputs import SHALLOW

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcamd_price_heston_cliquet", "mcamd_price_heston_cliquet_enqueue", "mcamd_heston_cliquet_price_f64")
NAN, INF = float("nan"), float("inf")
S0, T_, R, Q = hr.S0, hr.T_, hr.R, hr.Q_DIV
SUM, COMPOUND, VARIANCE = hq.SUM, hq.COMPOUND, hq.VARIANCE


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


def header():
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        return f.read()


def closed(name, kind, n_periods, first=1, local_floor=-INF, local_cap=INF, **changes):
    q, v0, kappa, theta, xi, rho = hr.params(name, **changes)
    return capi.heston_cliquet_price(kind, T_, R, q, v0, kappa, theta, xi, rho, n_periods, first, local_floor, local_cap)


# ---- 1. declarations, layout, refusals, resources ----------------------------------------------------------------------

def test_header_declares_the_calls_and_the_struct(lib):
    text = header()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert re.search(r"\}\s*mcamd_heston_cliquet_result\s*;", text)
    assert re.search(r"#define\s+MCAMD_ABI_VERSION\s+5\b", text) and lib.mcamd_abi_version() == 5
    assert "first carried by the build that ships csrc/heston_cliquet.hip" in text
    assert not re.search(r"mcamd_group_\w*heston", text)
    build = importlib.import_module("monte-carlo-project-cuda_amd.build")
    assert "heston_cliquet.hip" in build.SOURCES
    assert "heston_cliquet.hpp" in build.HEADERS and "cliquet_device.hpp" in build.HEADERS


def test_result_struct_matches_the_header():
    # static_assert(sizeof(mcamd_heston_cliquet_result) == 112) in csrc/capi_heston.cpp
    Rs = capi.HestonCliquetResult
    assert C.sizeof(Rs) == 112 and C.sizeof(capi.Heston) == 64 and C.sizeof(capi.Cliquet) == 56
    assert [(k, getattr(Rs, k).offset) for k, _ in Rs._fields_] == [
        ("price", 0), ("std_err", 8), ("ci_lo", 16), ("ci_hi", 24), ("sum", 32), ("sumsq", 40), ("n", 48),
        ("n_floored", 56), ("n_capped", 64), ("work_steps", 72), ("kernel_ms", 80), ("total_ms", 84), ("grid", 88),
        ("block", 92), ("truncated_steps", 96), ("mean_variance", 104)]
    text = header()
    assert re.search(r"typedef struct mcamd_heston_cliquet_result \{\s*/\* 112 bytes \*/", text)
    body = re.search(r"typedef struct mcamd_heston_cliquet_result \{(.*?)\}", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"\w+\s+([\w\s,]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [k for k, _ in Rs._fields_]
    assert names[:14] == [k for k, _ in capi.CliquetResult._fields_]   # mcamd_cliquet_result's fields come first


def test_the_six_kernels_use_no_scratch():
    """the cross-compile alone: heston_cliquet_kernel<T, KIND> for two precisions and three kinds, no private segment,
    no spilled register, and no LDS beyond what MathCtx<T> and the sums need (tools/isa_diff.py reads the figures)"""
    from importlib import util as ilu
    spec = ilu.spec_from_file_location("isa_diff_for_heston_cliquet", os.path.join(ROOT, "tools", "isa_diff.py"))
    isa = ilu.module_from_spec(spec)
    spec.loader.exec_module(isa)
    kernels = isa.kernels_of(ROOT, "heston_cliquet.hip")
    found = sorted(re.search(r"heston_cliquet_kernelI([fd])Li([012])E", k).groups() for k in kernels)
    assert found == [(t, k) for t in "df" for k in "012"], sorted(kernels)
    for k, (ops, fig) in kernels.items():
        print(k, fig)
        assert fig["scratch"] == 0 and fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0 and fig["agpr"] == 0, (k, fig)
        assert fig["lds"] < (1024 if "If" in k else 21 * 1024), (k, fig)
        assert fig["vgpr"] <= (96 if "If" in k else 168), (k, fig)   # five / three wavefronts per SIMD at least


def price(lib, opt, sim, hs, cq, res=True, enqueue=False):
    out = capi.HestonCliquetResult()
    ref = lambda x: None if x is None else C.byref(x)
    if enqueue:
        rc = lib.mcamd_price_heston_cliquet_enqueue(None, ref(opt), ref(sim), ref(hs), ref(cq), None, None)
    else:
        rc = lib.mcamd_price_heston_cliquet(None, ref(opt), ref(sim), ref(hs), ref(cq), None,
                                            C.byref(out) if res else None)
    return rc, lib.mcamd_last_error().decode()


BASE = dict(S0=NAN, K=NAN, v=NAN, B=NAN, r=R, T=T_)   # opt->v, opt->K and opt->B are ignored and nothing reads S0


def heston(payoff=capi.PAYOFF_CALL, **kw):
    q, v0, kappa, theta, xi, rho = hr.params("F")
    return capi.make_heston(payoff, **dict(dict(q=q, v0=v0, kappa=kappa, theta=theta, xi=xi, rho=rho), **kw))


def cliquet(kind=SUM, reset_every=4, first_period=1, **kw):
    return capi.make_cliquet(kind, reset_every, first_period, **dict(dict(q=Q), **kw))


def refusals():
    O, S = capi.make_option, capi.make_sim
    opt, sim, hs, cq = O(**BASE), S(1000, 12), heston(), cliquet()
    yield "no opt", (None, sim, hs, cq), {}, "non-NULL"
    yield "no sim", (opt, None, hs, cq), {}, "non-NULL"
    yield "no heston", (opt, sim, None, cq), {}, "non-NULL"
    yield "no cliquet", (opt, sim, hs, None), {}, "non-NULL"
    yield "no res", (opt, sim, hs, cq), dict(res=False), "non-NULL"
    # what mcamd_price_cliquet refuses before its surface
    for kind in (-1, 3):
        yield f"kind {kind}", (opt, sim, hs, cliquet(kind)), {}, "kind"
    bad = cliquet()
    bad.reserved = 1
    yield "cliquet reserved", (opt, sim, hs, bad), {}, "cliquet->reserved"
    for every in (0, 5, 24):
        yield f"reset_every {every}", (opt, sim, hs, cliquet(reset_every=every)), {}, "reset_every"
    for first in (0, 4):
        yield f"first_period {first}", (opt, sim, hs, cliquet(first_period=first)), {}, "first_period"
    for field in ("local_floor", "local_cap", "global_floor", "global_cap"):
        yield f"{field} nan", (opt, sim, hs, cliquet(**{field: NAN})), {}, "NaN"
    yield "local order", (opt, sim, hs, cliquet(local_floor=0.05, local_cap=0.05)), {}, "local_floor must lie below"
    yield "global order", (opt, sim, hs, cliquet(global_floor=0.3, global_cap=0.1)), {}, "global_floor must lie below"
    yield "compound floor", (opt, sim, hs, cliquet(COMPOUND, local_floor=-1.5)), {}, "compounding"
    yield "compound cap", (opt, sim, hs, cliquet(COMPOUND, local_floor=-INF, local_cap=-1.0)), {}, "compounding"
    yield "variance floor", (opt, sim, hs, cliquet(VARIANCE, local_floor=0.0)), {}, "realized variance"
    yield "variance cap", (opt, sim, hs, cliquet(VARIANCE, local_cap=0.1)), {}, "realized variance"
    for value in (NAN, INF):
        yield f"cliquet q {value}", (opt, sim, hs, cliquet(q=value)), {}, "dividend yield q must be finite"
    yield "r = nan", (O(**dict(BASE, r=NAN)), sim, hs, cq), {}, "finite"
    yield "use_window", (O(**BASE, use_window=1), sim, hs, cq), {}, "window"
    yield "P1", (O(**BASE, P1=1), sim, hs, cq), {}, "window"
    yield "Sk", (O(**BASE, Sk=95.0), sim, hs, cq), {}, "Sk"
    yield "Tk", (O(**BASE, Tk=5), sim, hs, cq), {}, "Tk"
    yield "dt", (O(**BASE, dt=0.01), sim, hs, cq), {}, "dt"
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE, capi.FLAG_PRODUCT_FORM, 32):
        yield f"flags {flags}", (opt, S(1000, 12, flags=flags), hs, cq), {}, "flags"
    yield "precision", (opt, S(1000, 12, precision=16), hs, cq), {}, "precision"
    yield "n_steps 0", (opt, S(1000, 0), hs, cliquet(reset_every=1)), {}, "n_steps"
    yield "shard overflow", (opt, S(1 << 63, 12, path_offset=(1 << 64) - 10, n_paths_local=100), hs, cq), {}, "overflows"
    yield "exponent range", (O(**dict(BASE, T=100.0)), sim, heston(q=-1e4), cliquet(q=-1e4)), {}, "exponent range"
    yield "T = 0", (O(**dict(BASE, T=0.0)), sim, hs, cq), {}, "T > 0"
    yield "T = inf", (O(**dict(BASE, T=INF)), sim, hs, cq), {}, "finite"
    # what mcamd_price_heston refuses of the job and the model
    for payoff in (-1, 2):
        yield f"payoff {payoff}", (opt, sim, heston(payoff), cq), {}, "payoff"
    for scheme in (-1, 1):
        yield f"scheme {scheme}", (opt, sim, heston(scheme=scheme), cq), {}, "scheme"
    for value in (1.0, NAN, 5e-324):
        bad = heston()
        bad.reserved = value
        yield f"heston reserved {value}", (opt, sim, bad, cq), {}, "heston->reserved"
    for field in ("q", "v0", "kappa", "theta", "xi", "rho"):
        for value in (NAN, INF, -INF):
            yield f"{field} = {value}", (opt, sim, heston(**{field: value}), cq), {}, "must be finite"
    for field in ("v0", "kappa", "theta", "xi"):
        yield f"{field} < 0", (opt, sim, heston(**{field: -1e-300}), cq), {}, ">= 0"
    for rho in (1.0000000000000002, -1.5):
        yield f"rho = {rho}", (opt, sim, heston(rho=rho), cq), {}, "rho"
    # one dividend yield, stated twice
    yield "q differs", (opt, sim, heston(q=0.01), cliquet(q=0.02)), {}, "same dividend yield"
    yield "q differs by an ulp", (opt, sim, heston(q=0.01), cliquet(q=math.nextafter(0.01, 1.0))), {}, "same dividend yield"
    yield "q differs in sign of zero", (opt, sim, heston(q=0.0), cliquet(q=-0.0)), {}, "same dividend yield"
    # the order: the cliquet's job, then the model, then the yields, then the context
    yield "kind before payoff", (opt, sim, heston(2), cliquet(3)), {}, "kind"
    yield "sim before the model", (opt, S(1000, 12, precision=16), heston(xi=-1.0), cq), {}, "precision"
    yield "the model before the yields", (opt, sim, heston(q=0.5, rho=2.0), cq), {}, "rho"
    yield "no context", (opt, sim, hs, cq), {}, "ctx is NULL"


@pytest.mark.parametrize("case", list(refusals()), ids=lambda c: c[0])
def test_refusals_before_the_context_is_looked_at(lib, case):
    """Every case but the order cases and the last is wrong in one way only and is given no context: the message names
    the request's fault, so the refusal came before the context."""
    _, args, kw, words = case
    rc, msg = price(lib, *args, **kw)
    assert rc == capi.ERR_INVALID and words in msg, msg
    if kw.get("res", True):   # the enqueue form shares the checks
        rc, msg = price(lib, *args, enqueue=True, **kw)
        assert rc == capi.ERR_INVALID and words in msg, msg


@pytest.mark.parametrize("flags,prec", [(0, capi.F64), (capi.FLAG_LOG_SPACE, capi.F32)])
def test_accepted_requests_reach_the_context(lib, flags, prec):
    sim = capi.make_sim(1000, 12, prec, flags=flags, path_offset=3, n_paths_local=0)
    opt = capi.make_option(**BASE)
    for kw in (dict(), dict(xi=0.0), dict(kappa=0.0), dict(rho=1.0), dict(rho=-1.0), dict(v0=0.0, theta=0.0)):
        for payoff in (capi.PAYOFF_CALL, capi.PAYOFF_PUT):   # in range, not read
            for job in cases.JOBS:
                cq = capi.make_cliquet(job[0], 3, 2, *job[1:], Q)
                rc, msg = price(lib, opt, sim, heston(payoff, **kw), cq)
                assert rc == capi.ERR_INVALID and "ctx is NULL" in msg, (kw, job, msg)
    for S, K in ((0.0, 0.0), (-1.0, INF)):   # S0 and K are not looked at
        rc, msg = price(lib, capi.make_option(**dict(BASE, S0=S, K=K)), sim, heston(), cliquet())
        assert rc == capi.ERR_INVALID and "ctx is NULL" in msg, msg
    rc, msg = price(lib, opt, sim, heston(q=-0.02), cliquet(COMPOUND, local_floor=-1.0, q=-0.02))
    assert rc == capi.ERR_INVALID and "ctx is NULL" in msg, msg


# ---- 2. the closed form --------------------------------------------------------------------------------------------------

def forward_phi(u, t, tau, v0, kappa, theta, xi, rho):
    """E[e^{iu x}] of x = ln(S_{t+tau} / S_t) - (r - q) tau from the textbook form of the Heston coefficients
    (Albrecher et al.) and the moment generating function of v_t: shares no code and no rearrangement with the library"""
    iu = 1j * u
    b = kappa - rho * xi * iu
    d = np.sqrt(b * b + xi * xi * (iu + u * u))
    g = (b - d) / (b + d)
    e = np.exp(-d * tau)
    Cc = kappa * theta / xi ** 2 * ((b - d) * tau - 2.0 * np.log((1.0 - g * e) / (1.0 - g)))
    Dd = (b - d) / xi ** 2 * (1.0 - e) / (1.0 - g * e)
    if t == 0.0:
        return np.exp(Cc + Dd * v0)
    c = xi * xi * (t if kappa == 0.0 else (1.0 - math.exp(-kappa * t)) / kappa) / 4.0
    one = 1.0 - 2.0 * c * Dd
    return np.exp(Cc + Dd * v0 * math.exp(-kappa * t) / one) * one ** (-2.0 * kappa * theta / xi ** 2)


def absorbed_mass(t, model):
    """kappa theta = 0: zero absorbs the variance, P(v_t = 0) = exp(-2 v0 e^{-kappa t} kappa / (xi^2 (1 - e^{-kappa t})))
    (the central chi-square's mass at 0), and from there the return is the forward's: a mass at x = 0 whose call is
    (F - k)+ and without which the characteristic function decays.  0 otherwise."""
    v0, kappa, theta, xi, _ = model
    if kappa * theta != 0.0 or t == 0.0:
        return 0.0
    if kappa == 0.0:
        return math.exp(-2.0 * v0 / (xi * xi * t))
    return math.exp(-2.0 * v0 * math.exp(-kappa * t) * kappa / (xi * xi * (1.0 - math.exp(-kappa * t))))


def quad_forward_call(k, t, tau, q, model):
    """(E[(S_{t+tau} / S_t - k)+], undiscounted, by adaptive quadrature of the Lewis integral; the most that the
    library's rule may drop of it).  The rule stops at U = 4096 at the latest (include/mcamd.h), and what lies beyond is
    at most sqrt(F k) / pi |phi(U - i/2)| / U, |phi(u - i/2)| falling in u: negligible unless rho = +-1 or kappa theta = 0,
    where the characteristic function decays like a power.  The quadrature itself runs three times as far there."""
    from scipy.integrate import quad
    F = math.exp((R - q) * tau)
    if k <= 0.0:
        return F - k, 0.0
    if k == INF:
        return 0.0, 0.0
    lk = math.log(F / k)
    atom = absorbed_mass(t, model)
    slow = atom != 0.0 or abs(model[4]) == 1.0
    f = lambda u: (np.exp(1j * u * lk) * (forward_phi(u - 0.5j, t, tau, *model) - atom)).real / (u * u + 0.25)
    total = sum(quad(f, a, a + 10.0, epsabs=1e-13, epsrel=1e-13, limit=200)[0]
                for a in np.arange(0.0, 12000.0 if slow else 600.0, 10.0))
    dropped = math.sqrt(F * k) / math.pi * abs(forward_phi(4096.0 - 0.5j, t, tau, *model) - atom) / 4096.0
    return F - atom * min(F, k) - math.sqrt(F * k) / math.pi * total, dropped


def quad_period(t, tau, q, model, local_floor, local_cap, with_dropped=False):
    """e^{-rT} (E_p - 1) of one period (and the most the library's rule may drop of it)"""
    lo = max(local_floor, -1.0)
    (c_lo, d_lo), (c_hi, d_hi) = quad_forward_call(1.0 + lo, t, tau, q, model), quad_forward_call(1.0 + local_cap, t, tau, q, model)
    value = math.exp(-R * T_) * ((1.0 + lo) + c_lo - c_hi - 1.0)
    return (value, math.exp(-R * T_) * (d_lo + d_hi)) if with_dropped else value


@pytest.mark.parametrize("name", ["F", "N"])
def test_one_period_sum_is_the_european_call(lib, name):
    q, *model = hr.params(name)
    for k in (0.8, 1.0, 1.2):
        got = closed(name, SUM, 1, 1, k - 1.0)
        want = capi.heston_price(1.0, k, T_, R, q, *model) + math.exp(-R * T_) * (k - 1.0)
        print(f"{name} k {k}: cliquet form {got:.12f}, European form {want:.12f}, difference {got - want:+.2e}")
        assert abs(got - want) <= 1e-10
        assert abs(closed(name, COMPOUND, 1, 1, k - 1.0) - got) == 0.0   # one period: the same thing


@pytest.mark.parametrize("name", ["F", "N"])
def test_sum_against_scipy_quad_of_the_forward_characteristic_function(lib, name):
    pytest.importorskip("scipy")
    q, *model = hr.params(name)
    # forward windows [0, T], [T/2, T], [3T/4, T]: the call struck at k times the spot of the window's start
    for M, first in ((1, 1), (2, 2), (4, 4)):
        tau = T_ / M
        for k in (0.8, 1.0, 1.2):
            got, want = closed(name, SUM, M, first, k - 1.0), quad_period((first - 1) * tau, tau, q, model, k - 1.0, INF)
            print(f"{name} window [{(first - 1) * tau}, {T_}] k {k}: closed {got:.12f} quad {want:.12f} ({got - want:+.2e})")
            assert abs(got - want) <= 1e-8
    # every period of a four-period cliquet with a floor and a cap, one by one and together
    floor, cap = -0.03, 0.08
    per_period = [quad_period(p * 0.25, 0.25, q, model, floor, cap) for p in range(4)]
    for first in (1, 2, 3, 4):
        got, want = closed(name, SUM, 4, first, floor, cap), sum(per_period[first - 1:])
        print(f"{name} four periods from {first}, [{floor}, {cap}]: closed {got:.12f} quad {want:.12f} ({got - want:+.2e})")
        assert abs(got - want) <= 1e-8
    assert per_period[0] != per_period[1]   # the forward smile is not the spot smile
    # a floor at or below -1 never binds and a cap alone is a covered call on the return
    assert closed(name, SUM, 2, 1, -5.0, 0.05) == closed(name, SUM, 2, 1, -1.0, 0.05) == closed(name, SUM, 2, 1, -INF, 0.05)
    fwd = math.exp((R - q) * 0.5)
    assert abs(closed(name, SUM, 2, 1) - math.exp(-R * T_) * 2.0 * (fwd - 1.0)) <= 1e-14   # no bounds: the forward


def mp_second_moment(t, tau, q, model):
    """-phi''(0) of the period's log-return at 30 digits, from the textbook forward characteristic function"""
    import mpmath as mp
    v0, kappa, theta, xi, rho = (mp.mpf(x) for x in model)
    t, tau, mu = mp.mpf(t), mp.mpf(tau), mp.mpf(R) - mp.mpf(q)

    def phi(u):
        iu = mp.mpc(0, 1) * u
        b = kappa - rho * xi * iu
        d = mp.sqrt(b * b + xi * xi * (iu + u * u))
        g = (b - d) / (b + d)
        e = mp.exp(-d * tau)
        Cc = kappa * theta / xi ** 2 * ((b - d) * tau - 2 * mp.log((1 - g * e) / (1 - g)))
        Dd = (b - d) / xi ** 2 * (1 - e) / (1 - g * e)
        one = 1 - 2 * (xi * xi * (1 - mp.exp(-kappa * t)) / (4 * kappa)) * Dd
        return mp.exp(iu * mu * tau + Cc - 2 * kappa * theta / xi ** 2 * mp.log(one) + Dd * v0 * mp.exp(-kappa * t) / one)

    return -mp.diff(phi, 0, 2).real


@pytest.mark.parametrize("name", ["F", "N"])
def test_variance_against_mpmath(lib, name):
    mp = pytest.importorskip("mpmath")
    q, *model = hr.params(name)
    with mp.workdps(30):
        for M, first in ((4, 1), (12, 1), (4, 3), (52, 40)):
            tau = mp.mpf(T_) / M
            total = sum(mp_second_moment((p - 1) * tau, tau, q, model) for p in range(first, M + 1))
            want = float(mp.exp(-mp.mpf(R) * T_) * total / ((M - first + 1) * tau))
            got = closed(name, VARIANCE, M, first)
            print(f"{name} variance, {M} periods from {first}: closed {got:.12f} mpmath {want:.12f}, relative difference "
                  f"{(got - want) / want:+.2e}")
            assert abs(got - want) <= 1e-8 * want


@pytest.mark.parametrize("name,changes", [("F", {}), ("N", {}), ("N", dict(v0=0.09)), ("F", dict(kappa=0.0, v0=0.05))])
def test_discrete_variance_approaches_the_continuous_limit(lib, name, changes):
    q, v0, kappa, theta, xi, rho = hr.params(name, **changes)
    for first_share in (0.0, 0.5):
        gaps = []
        for M in (4, 12, 52, 252):
            first = int(first_share * M) + 1
            t1 = (first - 1) * T_ / M
            mean_v = v0 if kappa == 0.0 else theta + (v0 - theta) * (math.exp(-kappa * t1) - math.exp(-kappa * T_)) / (kappa * (T_ - t1))
            gaps.append(closed(name, VARIANCE, M, first, **changes) - math.exp(-R * T_) * mean_v)
        print(f"{name} {changes} from {first_share} T: discrete minus continuous at 4, 12, 52, 252 periods "
              + ", ".join(f"{g:+.3e}" for g in gaps))
        assert all(abs(b) < abs(a) for a, b in zip(gaps, gaps[1:])) and abs(gaps[-1]) <= 1e-4


def period_vols(v0, kappa, theta, M):
    tau = T_ / M
    gain = tau if kappa == 0.0 else -math.expm1(-kappa * tau) / kappa
    return [math.sqrt(theta + (v0 - theta) * math.exp(-kappa * p * tau) * gain / tau) for p in range(M)]


@pytest.mark.parametrize("kappa,v0,theta", [(2.0, 0.04, 0.04), (1.5, 0.09, 0.04), (0.0, 0.05, 0.3), (3.0, 0.01, 0.06)])
def test_deterministic_limit_and_the_step_across_the_threshold(lib, kappa, v0, theta):
    xi_min = capi.HESTON_XI_MIN
    for kind, M, first, floor, cap in ((SUM, 4, 1, -0.03, 0.08), (SUM, 2, 2, 0.0, INF), (VARIANCE, 4, 1, -INF, INF),
                                       (VARIANCE, 12, 7, -INF, INF), (COMPOUND, 4, 2, -0.03, 0.08)):
        at = lambda xi: capi.heston_cliquet_price(kind, T_, R, Q, v0, kappa, theta, xi, -0.7, M, first, floor, cap)
        limit = capi.cliquet_price(kind, T_, R, Q, period_vols(v0, kappa, theta, M), first, floor, cap)
        for xi in (0.0, 0.5 * xi_min, xi_min * (1 - 1e-12)):
            assert at(xi) == limit                     # below the threshold: the deterministic-variance form itself
        if kind == COMPOUND:
            continue                                   # above it several compounded periods are refused
        step = at(xi_min) - limit
        print(f"kind {kind} {M} periods from {first}, kappa {kappa} v0 {v0} theta {theta}: limit {limit:.10f}, step across "
              f"the threshold {step:+.2e}")
        assert abs(step) <= 1e-9 and abs(at(2.0 * xi_min) - limit) <= 2e-9


def test_no_mean_reversion_and_extreme_correlation_agree_with_quad(lib):
    pytest.importorskip("scipy")
    for name in ("F", "N"):
        forward_start, two_periods = (2, 2, 0.0, INF), (4, 3, -0.03, 0.08)
        for changes, jobs in ((dict(kappa=0.0), (forward_start, two_periods)), (dict(rho=-1.0), (two_periods,)),
                              (dict(rho=1.0), (two_periods,)), (dict(kappa=0.0, rho=-1.0), (forward_start,))):
            q, *model = hr.params(name, **changes)
            for M, first, floor, cap in jobs:
                got = closed(name, SUM, M, first, floor, cap, **changes)
                tau = T_ / M
                periods = [quad_period(p * tau, tau, q, model, floor, cap, True) for p in range(first - 1, M)]
                want, dropped = sum(p[0] for p in periods), sum(p[1] for p in periods)
                print(f"{name} {changes} {M} periods from {first}: closed {got:.12f} quad {want:.12f} ({got - want:+.2e}; "
                      f"the rule may drop {dropped:.1e})")
                assert math.isfinite(got) and abs(got - want) <= 1e-8 + dropped
            assert math.isfinite(closed(name, VARIANCE, 4, 2, **changes)) and closed(name, VARIANCE, 4, 2, **changes) > 0


def test_compound_is_refused_over_dependent_periods_and_served_otherwise(lib):
    with pytest.raises(capi.McamdError) as e:
        closed("F", COMPOUND, 4, 1, -0.03, 0.08)
    assert e.value.code == capi.ERR_INVALID and "depend on each other" in str(e.value)
    with pytest.raises(capi.McamdError):
        closed("F", COMPOUND, 4, 3, -0.03, 0.08)
    # one counted period: the SUM form
    assert closed("F", COMPOUND, 4, 4, -0.03, 0.08) == closed("F", SUM, 4, 4, -0.03, 0.08)
    # below the threshold the periods are independent: the product form
    vols = period_vols(0.09, 1.5, 0.04, 4)
    got = closed("N", COMPOUND, 4, 1, -0.03, 0.08, xi=0.0, v0=0.09)
    assert got == capi.cliquet_price(COMPOUND, T_, R, Q, vols, 1, -0.03, 0.08) and got != 0.0


def test_closed_form_refusals(lib):
    good = dict(kind=SUM, T=T_, r=R, q=Q, v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7, n_periods=4, first_period=1,
                local_floor=-0.03, local_cap=0.08)
    cases_ = [("kind", 3, "kind"), ("kind", -1, "kind"), ("T", 0.0, "T > 0"), ("T", -1.0, "T > 0"), ("rho", 1.5, "rho"),
              ("n_periods", 0, "n_periods"), ("first_period", 0, "first_period"), ("first_period", 5, "first_period"),
              ("local_floor", NAN, "NaN"), ("local_cap", -0.03, "local_floor must lie below")]
    cases_ += [(f, v, "finite") for f in ("T", "r") for v in (NAN, INF)]
    cases_ += [(f, v, "must be finite") for f in ("q", "v0", "kappa", "theta", "xi", "rho") for v in (NAN, INF, -INF)]
    cases_ += [(f, -0.01, ">= 0") for f in ("v0", "kappa", "theta", "xi")]
    for field, value, words in cases_:
        with pytest.raises(capi.McamdError) as e:
            capi.heston_cliquet_price(**dict(good, **{field: value}))
        assert e.value.code == capi.ERR_INVALID and words in str(e.value), (field, value, str(e.value))
    for kind, floor, cap, words in ((COMPOUND, -1.5, 0.1, "compounding"), (VARIANCE, 0.0, INF, "realized variance")):
        with pytest.raises(capi.McamdError) as e:
            capi.heston_cliquet_price(**dict(good, kind=kind, local_floor=floor, local_cap=cap))
        assert words in str(e.value)
    assert lib.mcamd_heston_cliquet_price_f64(0, T_, R, Q, 0.04, 2.0, 0.04, 0.3, -0.7, 4, 1, -0.03, 0.08, None) == capi.ERR_INVALID
    assert capi.heston_cliquet_price(**good) != 0.0


# ---- 3. the restatement against the two it is made of ------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(48, 4, 1), (50, 10, 5), (6, 3, 1), (1, 1, 1)], ids=str)
def test_constant_variance_is_the_cliquet_restatement_on_a_flat_surface(shape):
    """v0 = 0.2 * 0.2 as float64 rounds it, so that sqrt(v0) is 0.2 and s s is v0 again, bit for bit: then every
    operation of the two restatements has the same operands"""
    n_steps, reset_every, first = shape
    sigma = np.float64(0.2)
    v0 = float(sigma * sigma)
    assert np.sqrt(np.float64(v0)) == sigma
    z, zv = hr.draws(64, SHALLOW[0], SHALLOW[1], 256, n_steps)
    grid, flat = (1, 2, -1.0, 1.0), [[float(sigma), float(sigma)]]
    p = hr.params("F", v0=v0, xi=0.0, kappa=0.0, theta=0.3)
    for job in cases.JOBS:
        got = hq.samples(z, zv, T_, R, p, job[0], reset_every, first, *job[1:])
        lv = cr.samples(z, T_, R, Q, grid, flat, job[0], reset_every, first, *job[1:])
        for k in ("y", "A", "D", "floored", "capped"):
            assert np.array_equal(got[k], lv[k]), (job, k)
        assert not got["trunc"].any() and (got["v_n"] == v0).all()


@pytest.mark.parametrize("name", ["F", "N", "H"])
@pytest.mark.parametrize("n_steps", [50, 3, 1])
def test_one_unbounded_period_is_the_european_path(name, n_steps):
    z, zv = hr.draws(64, SHALLOW[0], SHALLOW[1], 256, n_steps)
    p = hr.params(name)
    got = hq.samples(z, zv, T_, R, p, SUM, n_steps)
    eu = hr.samples(z, zv, S0, 100.0, T_, R, p, hr.CALL)
    ratio = eu["S_T"] / S0
    assert np.abs((got["y"] + 1.0) - ratio).max() <= 4.0 * np.finfo(np.float64).eps * ratio.max()
    assert np.array_equal(got["trunc"], eu["trunc"]) and np.array_equal(got["rv"], eu["rv"])
    assert np.array_equal(got["v_n"], eu["v_n"])


# ---- 4. Richardson extrapolation against the closed form --------------------------------------------------------------------

@pytest.mark.parametrize("tag,kind,M,first,floor", [("forward-start call", SUM, 2, 2, 0.0), ("variance swap", VARIANCE, 4, 1, -INF)])
def test_richardson_pair_against_the_closed_form_on_N(lib, tag, kind, M, first, floor):
    n, p = 120_000, hr.params("N")
    p128, se128 = hq.price_f64(128_064 + kind, n, 128, T_, R, p, kind, 128 // M, first, floor)
    p64, se64 = hq.price_f64(64_128 + kind, n, 64, T_, R, p, kind, 64 // M, first, floor)
    want = closed("N", kind, M, first, floor)
    extrapolated, margin = 2.0 * p128 - p64, 4.0 * math.sqrt(4.0 * se128 ** 2 + se64 ** 2)
    print(f"{tag}: closed {want:.6f}; 128 steps {p128 - want:+.6f} (SE {se128:.6f}), 64 steps {p64 - want:+.6f} "
          f"(SE {se64:.6f}), extrapolated {extrapolated - want:+.6f}, margin {margin:.6f}")
    assert abs(extrapolated - want) <= margin


# ---- 5. the precision spread, which fixes the GPU tolerance ------------------------------------------------------------------

def test_precision_spread_and_near_bound_share_of_the_restatement():
    """no kernel runs.  On every case of the GPU tests the restatement is finite and at most 2 % of the paths lie within
    the tolerance of a global bound; on the first shape the local bounds bind on a fair share of the periods and the
    doubly bounded job has paths on both global bounds and between them"""
    for name, precs in cases.MODELS:
        for prec in precs:
            tol = cases.tolerance(prec, name)
            print(f"{name} fp{prec}: restatement spread on the (48, 4, 1) shape {cases.measured_spread(prec, name):.3e}, "
                  f"tolerance {tol:.3e}")
            assert math.isfinite(tol)
            if name != "H":
                assert tol == cases.FLOOR[prec], (name, prec, tol)   # on F and N the floors decide
            for shape in cases.SHAPES:
                worst, near_share = 0.0, 0.0
                for job in cases.JOBS:
                    want, own, spread = cases.compare(prec, name, job, shape)
                    worst = max(worst, spread)
                    assert np.isfinite(np.asarray(want["y"], dtype=np.float64)).all()
                    if prec == cases.F32:   # the paths whose truncation count an fp32 kernel may get differently
                        assert (want["min_abs_v"] < hc.NEAR_ZERO).mean() <= hc.NEAR_CAP, (name, shape)
                    for flags in cases.near(want, job, tol):
                        near_share = max(near_share, flags.mean())
                        assert flags.mean() <= cases.NEAR_CAP, (name, prec, shape, job, flags.mean())
                print(f"  {cases.shape_name(shape)}: largest restatement difference {worst:.3e}, largest near-bound share "
                      f"{near_share:.4f}")
            want, _, _ = cases.compare(prec, name, cases.JOBS[0], cases.FIRST_SHAPE)
            D = np.asarray(want["D"], dtype=np.float64)
            clipped = ((np.exp(D) - 1.0 <= -0.03) | (np.exp(D) - 1.0 >= 0.05)).mean()
            print(f"  periods on a local bound {clipped:.3f}, paths floored {want['floored'].mean():.3f}, capped "
                  f"{want['capped'].mean():.3f}")
            if name != "H":   # H's variance is a quarter of the others' and mostly truncated: its periods move less
                assert 0.2 <= clipped <= 0.9 and want["floored"].mean() >= 0.05 and want["capped"].mean() >= 0.05
                assert (~(want["floored"] | want["capped"])).mean() >= 0.05
