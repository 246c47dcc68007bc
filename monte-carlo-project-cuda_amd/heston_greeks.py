"""ctypes binding of include/mcamd_heston_greeks.h: the Greeks of a European option under Heston stochastic volatility
from one simulation (mcamd_price_heston_greeks).  A module of its own beside capi.py, as the header is one beside
mcamd.h: capi.EXPORTS and capi.PROTOTYPES stay the functions of mcamd.h, and this module binds its four onto the
library capi.load() returns.  tests/test_heston_greeks_header_cpu.py compares the two structs and PROTOTYPES with the
header, field by field and parameter by parameter.

    from importlib import import_module
    hg = import_module("monte-carlo-project-cuda_amd.heston_greeks")
    job = hg.make_job(gamma_eta=0.01, v0=0.005, xi=0.05)
    out = ctx.price_heston_greeks(opt, sim, heston, job)          # capi.Context delegates here
    out.as_dict()["delta"]                                        # (value, std_err)
"""
from __future__ import annotations

import ctypes as C

from . import capi

GREEK_PRICE, GREEK_DELTA, GREEK_GAMMA, GREEK_RHO, GREEK_RHO_Q = 0, 1, 2, 3, 4
GREEK_V0, GREEK_KAPPA, GREEK_THETA, GREEK_XI, GREEK_CORR = 5, 6, 7, 8, 9
GREEKS = 10
GREEK_NAMES = ("price", "delta", "gamma", "rho", "rho_q", "v0", "kappa", "theta", "xi", "corr")
PARAMS = ("v0", "kappa", "theta", "xi", "rho")   # the order of mcamd_heston_greeks_job.bump
STATS = 32                                        # doubles of the statistics record an enqueue leaves


class HestonGreeksJob(C.Structure):
    """mcamd_heston_greeks_job: gamma's half-width in ln(S) (0: no gamma) and the absolute half-widths of the central
    differences in v0, kappa, theta, xi and rho (0: not requested)."""
    _fields_ = [("gamma_eta", C.c_double), ("bump", C.c_double * 5), ("reserved", C.c_double)]

    @property
    def n_params(self) -> int:
        """P: the requested parameters"""
        return sum(1 for b in self.bump if b > 0.0)

    @property
    def n_rows(self) -> int:
        """rows of d_samples: h, d, g, then (h+, h-) per requested parameter"""
        return 3 + 2 * self.n_params


class HestonGreeks(C.Structure):
    """mcamd_heston_greeks: value / std_err indexed GREEK_*, then mcamd_heston_result's diagnostics and timings"""
    _fields_ = [("value", C.c_double * 10), ("std_err", C.c_double * 10), ("n", C.c_uint64),
                ("truncated_steps", C.c_double), ("mean_variance", C.c_double), ("work_steps", C.c_double),
                ("kernel_ms", C.c_float), ("total_ms", C.c_float), ("grid", C.c_uint32), ("block", C.c_uint32)]

    def as_dict(self):
        """{name: (value, std_err)} of the ten quantities"""
        return {name: (self.value[i], self.std_err[i]) for i, name in enumerate(GREEK_NAMES)}


def _prototypes():
    """{name: (restype, argtypes)} of every function include/mcamd_heston_greeks.h declares, typed as capi.PROTOTYPES
    types mcamd.h's"""
    P, vp, i32, f64 = C.POINTER, C.c_void_p, C.c_int, C.c_double
    pf64 = P(f64)
    job = (vp, P(capi.Option), P(capi.Sim), P(capi.Heston), P(HestonGreeksJob), vp)
    return {
        "mcamd_price_heston_greeks": (i32, [*job, P(HestonGreeks)]),
        "mcamd_price_heston_greeks_enqueue": (i32, [*job, vp]),
        "mcamd_finalize_heston_greeks_stats": (i32, [pf64, P(capi.Option), P(HestonGreeksJob), P(HestonGreeks)]),
        "mcamd_heston_greeks_f64": (i32, [*[f64] * 10, i32, f64, pf64, pf64]),
    }


PROTOTYPES = _prototypes()
EXPORTS = list(PROTOTYPES)   # every symbol include/mcamd_heston_greeks.h declares

_bound = None


def load() -> C.CDLL:
    """capi.load()'s library with this header's functions typed; raises if the library lacks one (there is no
    fallback)."""
    global _bound
    L = capi.load()
    if _bound is not L:
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _bound = L
    return L


def make_job(gamma_eta=0.0, v0=0.0, kappa=0.0, theta=0.0, xi=0.0, rho=0.0) -> HestonGreeksJob:
    """gamma_eta: gamma's half-width in ln(S), 0 for none; the others: the absolute half-width of the central difference
    in that parameter, 0 for not requested"""
    return HestonGreeksJob(float(gamma_eta), (C.c_double * 5)(float(v0), float(kappa), float(theta), float(xi), float(rho)),
                           0.0)


def _filled(fn, result, *args):
    out = result()
    capi._check(getattr(load(), fn)(*args, out))
    return out


def price(ctx: "capi.Context", opt, sim, heston, job: HestonGreeksJob, samples=None) -> HestonGreeks:
    """mcamd_price_heston_greeks on a capi.Context.  samples: optional device tensor of job.n_rows x n_paths_local
    values of the path precision, row-major: h, d, g, then (h+, h-) per requested parameter."""
    load()
    return ctx._sync("mcamd_price_heston_greeks", HestonGreeks, opt, sim, heston, job, capi._ptr(samples))


def enqueue(ctx: "capi.Context", opt, sim, heston, job: HestonGreeksJob, stats, samples=None) -> None:
    """mcamd_price_heston_greeks_enqueue: leaves the 32-double record in the device tensor stats, in stream order"""
    load()
    ctx._enqueue("mcamd_price_heston_greeks_enqueue", opt, sim, heston, job, capi._ptr(samples), capi._ptr(stats))


def finalize_stats(stats32, opt, job: HestonGreeksJob) -> HestonGreeks:
    """Greeks of a (possibly all-reduced) 32-double record left by enqueue; S0, T and r come from opt"""
    return _filled("mcamd_finalize_heston_greeks_stats", HestonGreeks, capi._doubles(stats32, STATS), opt, job)


def greeks_closed_form(S0, K, T, r, q, v0, kappa, theta, xi, rho, payoff=capi.PAYOFF_CALL, gamma_eta=0.0,
                       bump=(0.0, 0.0, 0.0, 0.0, 0.0)):
    """The model's ten values, indexed GREEK_* (mcamd_heston_greeks_f64): the price and the analytic delta of the Lewis
    integral, gamma as the finite difference of that delta over gamma_eta that the kernel estimates, rho and rho_q from
    homogeneity, and the parameter entries as central differences of heston_price at bump (0 where the bump is 0)."""
    return list(_filled("mcamd_heston_greeks_f64", C.c_double * 10, S0, K, T, r, q, v0, kappa, theta, xi, rho, payoff,
                        gamma_eta, capi._doubles(bump, 5)))
