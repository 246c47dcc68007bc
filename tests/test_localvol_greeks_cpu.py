"""CPU-only checks of the local-volatility Greeks (include/mcamd.h, mcamd_price_localvol_greeks): declarations and struct
layouts; every refusal that needs neither surface nor context; the finalize call on hand-made records; and the numpy
restatement (tests/localvol_greeks_restate.py) itself — its price sample against tests/localvol_restate.py bit for bit,
the sum of the buckets against vega, every tangent estimator against a central common-random-number finite difference
of the restated price, a time-only surface and displaced diffusion against closed forms — and, on every input of the
GPU test, that the restatement's own rounding uses up at most half the tolerance and leaves out at most 1 % of a case.
No kernels run here."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import localvol_greeks_cases as cases
import localvol_greeks_restate as gr
import localvol_restate as lv

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcamd_price_localvol_greeks", "mcamd_price_localvol_greeks_enqueue", "mcamd_finalize_localvol_greeks_stats")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


# ---- declarations ----------------------------------------------------------------------------------------------------

def test_header_declares_the_calls_and_the_structs(lib):
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS and hasattr(lib, name)
    for struct in ("mcamd_localvol_greeks_job", "mcamd_localvol_greeks"):
        assert re.search(r"\}\s*" + struct + r"\s*;", header), struct
    assert re.search(r"#define\s+MCAMD_LOCALVOL_GREEKS_MAX_BUCKETS\s+8\b", header) and capi.LOCALVOL_GREEKS_MAX_BUCKETS == 8
    for i, name in enumerate(("PRICE", "DELTA", "GAMMA", "VEGA", "RHO", "RHO_Q")):
        assert re.search(r"#define\s+MCAMD_LOCALVOL_GREEK_" + name + r"\s+" + str(i) + r"\b", header)
        assert getattr(capi, "LOCALVOL_GREEK_" + name) == i == getattr(gr, name)
    assert re.search(r"#define\s+MCAMD_ABI_VERSION\s+5\b", header) and lib.mcamd_abi_version() == 5
    assert not re.search(r"mcamd_group_\w*localvol", header)
    # the header says why gamma is a difference and what delta is on a node
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    assert "a second pathwise derivative does not exist" in flat and "one-sided derivative" in flat


def test_structs_match_the_header():
    # static_assert(sizeof(mcamd_localvol_greeks_job) == 24 && sizeof(mcamd_localvol_greeks) == 472) in csrc/capi_localvol.cpp
    J, G = capi.LocalVolGreeksJob, capi.LocalVolGreeks
    assert C.sizeof(J) == 24
    assert (J.payoff.offset, J.n_vega_buckets.offset, J.q.offset, J.gamma_bump.offset) == (0, 4, 8, 16)
    assert C.sizeof(G) == 472
    assert (G.value.offset, G.std_err.offset, G.bucket_value.offset, G.bucket_std_err.offset, G.sum.offset,
            G.sumsq.offset, G.bucket_sum.offset, G.bucket_sumsq.offset) == (0, 48, 96, 160, 224, 272, 320, 384)
    assert (G.n.offset, G.kernel_ms.offset, G.total_ms.offset, G.grid.offset, G.block.offset) == (448, 456, 460, 464, 468)
    j = capi.make_localvol_greeks_job(capi.PAYOFF_PUT, 5, 0.03, 0.01)
    assert (j.payoff, j.n_vega_buckets, j.q, j.gamma_bump) == (1, 5, 0.03, 0.01)
    d = capi.make_localvol_greeks_job()
    assert (d.payoff, d.n_vega_buckets, d.q, d.gamma_bump) == (0, 0, 0.0, 0.0)
    assert capi.LOCALVOL_GREEKS_STATS == 32 and capi.LOCALVOL_GREEK_NAMES == gr.NAMES


# ---- refusals --------------------------------------------------------------------------------------------------------

OPT = dict(S0=100.0, K=100.0, r=0.1, v=0.0, T=1.0)   # v is ignored


def price(lib, opt, sim, job, out=True):
    res = capi.LocalVolGreeks()
    ref = lambda x: None if x is None else C.byref(x)
    rc = lib.mcamd_price_localvol_greeks(None, ref(opt), ref(sim), ref(job), None, None, C.byref(res) if out else None)
    return rc, lib.mcamd_last_error().decode()


def job_refusals():
    O, S, J = capi.make_option, capi.make_sim, capi.make_localvol_greeks_job
    opt, sim, job = O(**OPT), S(1000, 50), J()
    inf, nan = float("inf"), float("nan")
    yield "no opt", (None, sim, job), {}, "non-NULL"
    yield "no sim", (opt, None, job), {}, "non-NULL"
    yield "no job", (opt, sim, None), {}, "non-NULL"
    yield "no out", (opt, sim, job), dict(out=False), "non-NULL"
    for p in (-1, 2):
        yield f"payoff {p}", (opt, sim, J(payoff=p)), {}, "payoff"
    for B in (9, 64, 2 ** 32 - 1):
        yield f"buckets {B}", (opt, sim, J(n_vega_buckets=B)), {}, "n_vega_buckets"
    for eta in (nan, inf, -inf, -0.01, 0.1000001, 1.0):
        yield f"gamma_bump {eta}", (opt, sim, J(gamma_bump=eta)), {}, "gamma_bump"
    for q in (nan, inf, -inf):
        yield f"q = {q}", (opt, sim, J(q=q)), {}, "dividend yield"
    yield "use_window", (O(**OPT, use_window=1), sim, job), {}, "window"
    yield "P1", (O(**OPT, P1=1), sim, job), {}, "window"
    yield "P2", (O(**OPT, P2=3), sim, job), {}, "window"
    yield "Ik", (O(**OPT, Ik=2), sim, job), {}, "window"
    yield "Sk", (O(**OPT, Sk=95.0), sim, job), {}, "Sk"
    yield "Tk", (O(**OPT, Tk=5), sim, job), {}, "Tk"
    yield "dt", (O(**OPT, dt=0.01), sim, job), {}, "dt"
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE, capi.FLAG_PRODUCT_FORM,
                  capi.FLAG_LOG_SPACE | capi.FLAG_ANTITHETIC, 32):
        yield f"flags {flags}", (opt, S(1000, 50, flags=flags), job), {}, "flags"
    yield "precision", (opt, S(1000, 50, precision=16), job), {}, "precision"
    yield "n_steps 0", (opt, S(1000, 0), job), {}, "n_steps"
    yield "shard overflow", (opt, S(1 << 63, 50, path_offset=(1 << 64) - 10, n_paths_local=100), job), {}, "overflows"
    yield "exponent range", (O(**dict(OPT, r=1000.0, T=100.0)), S(1000, 50), job), {}, "exponent range"
    yield "r nan", (O(**dict(OPT, r=nan)), sim, job), {}, "finite"
    yield "T 0", (O(**dict(OPT, T=0.0)), sim, job), {}, "T > 0"
    for S0 in (0.0, -100.0):
        yield f"S0 {S0}", (O(**dict(OPT, S0=S0)), sim, job), {}, "S0"


@pytest.mark.parametrize("case", list(job_refusals()), ids=lambda c: c[0])
def test_refusals_before_the_surface_and_the_context_are_looked_at(lib, case):
    _, args, kw, words = case
    rc, msg = price(lib, *args, **kw)
    assert rc == capi.ERR_INVALID and words in msg, msg
    if kw.get("out", True):   # the enqueue form shares the checks
        ref = lambda x: None if x is None else C.byref(x)
        rc = lib.mcamd_price_localvol_greeks_enqueue(None, ref(args[0]), ref(args[1]), ref(args[2]), None, None, None)
        assert rc == capi.ERR_INVALID and words in lib.mcamd_last_error().decode()


@pytest.mark.parametrize("payoff", [capi.PAYOFF_CALL, capi.PAYOFF_PUT])
@pytest.mark.parametrize("B,eta", [(0, 0.0), (8, 0.1), (3, 0.01)])
@pytest.mark.parametrize("flags,prec", [(0, capi.F64), (capi.FLAG_LOG_SPACE, capi.F32)])
def test_accepted_requests_reach_the_missing_surface(lib, payoff, B, eta, flags, prec):
    """opt->v is ignored: 0, a negative number and NaN all pass"""
    for v in (0.0, -1.0, float("nan"), 0.2):
        sim = capi.make_sim(1000, 50, prec, flags=flags, path_offset=3, n_paths_local=0)
        rc, msg = price(lib, capi.make_option(**dict(OPT, v=v)), sim, capi.make_localvol_greeks_job(payoff, B, 0.03, eta))
        assert rc == capi.ERR_INVALID and "surface" in msg and "non-NULL" in msg, msg


# ---- finalize --------------------------------------------------------------------------------------------------------

def test_finalize_on_hand_made_records(lib):
    r, T, n = 0.1, 2.0, 4
    disc = math.exp(-r * T)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((14, n))
    stats = np.zeros(32)
    stats[0:28:2], stats[1:28:2], stats[28] = x.sum(axis=1), (x * x).sum(axis=1), n
    g = capi.finalize_localvol_greeks_stats(stats, r, T, 8, True)
    assert g.n == n and (g.kernel_ms, g.total_ms, g.grid, g.block) == (0.0, 0.0, 0, 0)
    for e in range(14):
        fin = capi.finalize(stats[2 * e], stats[2 * e + 1], n, r, T)
        got = (g.value[e], g.std_err[e], g.sum[e], g.sumsq[e]) if e < 6 else \
              (g.bucket_value[e - 6], g.bucket_std_err[e - 6], g.bucket_sum[e - 6], g.bucket_sumsq[e - 6])
        assert got == (fin.price, fin.std_err, stats[2 * e], stats[2 * e + 1])
        assert got[0] == pytest.approx(disc * x[e].mean(), rel=1e-14, abs=1e-15)
        assert got[1] == pytest.approx(disc * x[e].std(ddof=1) / 2.0, rel=1e-12)
    # gamma undefined: NaN with zero sums; buckets from n_vega_buckets on stay 0
    h = capi.finalize_localvol_greeks_stats(stats, r, T, 3, False)
    assert math.isnan(h.value[2]) and math.isnan(h.std_err[2]) and h.sum[2] == h.sumsq[2] == 0.0
    assert [h.value[e] for e in (0, 1, 3, 4, 5)] == [g.value[e] for e in (0, 1, 3, 4, 5)]
    assert list(h.bucket_value)[:3] == list(g.bucket_value)[:3] and not any(list(h.bucket_value)[3:])
    assert not any(list(h.bucket_std_err)[3:] + list(h.bucket_sum)[3:] + list(h.bucket_sumsq)[3:])
    # an empty record, one path, and the refusals
    z = capi.finalize_localvol_greeks_stats(np.zeros(32), r, T, 8, True)
    assert z.n == 0 and not any(list(z.value) + list(z.std_err) + list(z.bucket_value))
    one = np.zeros(32)
    one[0], one[1], one[28] = 3.0, 9.0, 1
    assert capi.finalize_localvol_greeks_stats(one, r, T).value[0] == disc * 3.0
    assert capi.finalize_localvol_greeks_stats(one, r, T).std_err[0] == 0.0
    out = capi.LocalVolGreeks()
    arr = (C.c_double * 32)()
    assert lib.mcamd_finalize_localvol_greeks_stats(None, r, T, 0, 1, C.byref(out)) == capi.ERR_INVALID
    assert lib.mcamd_finalize_localvol_greeks_stats(arr, r, T, 0, 1, None) == capi.ERR_INVALID
    assert lib.mcamd_finalize_localvol_greeks_stats(arr, r, T, 9, 1, C.byref(out)) == capi.ERR_INVALID
    assert "n_vega_buckets" in lib.mcamd_last_error().decode()


# ---- the restatement: price, buckets, finite differences ---------------------------------------------------------------

N_FD, S0, K, T, R_, Q_ = 1 << 17, 100.0, 100.0, 1.0, 0.1, 0.03
FD_SURFACES = {   # n_t = B, so that a row bump is a bucket bump
    "skew": (cases.skew(4, 65, -1.47, 1.53), 50),
    "skew8": (cases.skew(8, 65, -1.47, 1.53, 0.16, 0.02), 48),
    "narrow": (cases.skew(4, 65, -0.047, 0.053), 50),
    "two": (((1, 2, -1.5, 1.5), np.array([[0.30, 0.14]])), 49),
}
_z = {}


def fd_normals(n_steps):
    if n_steps not in _z:
        _z[n_steps] = np.random.default_rng(1000 + n_steps).standard_normal((n_steps, N_FD))
    return _z[n_steps]


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.longdouble])
def test_price_sample_is_that_of_the_pricing_restatement_bit_for_bit(dtype):
    (grid, sigma), n_steps = FD_SURFACES["skew"]
    z = fd_normals(n_steps)[:, :5000].astype(np.float32).astype(np.float64)
    for payoff in (gr.CALL, gr.PUT):
        got = gr.samples(z, S0, K, T, R_, Q_, grid, sigma, payoff, 3, 0.01, dtype)
        want = lv.samples(z, S0, K, 0.0, T, R_, Q_, grid, sigma, lv.NO_BARRIER, payoff, lv.DISCRETE, dtype)
        assert got["q"].dtype == want["y"].dtype == gr.wide_of(dtype)
        assert np.array_equal(got["q"][gr.PRICE], want["y"]) and np.array_equal(got["S_T"], want["S_T"])
        assert (want["y"] != 0).mean() > 0.2
        assert got["J"].dtype == got["U"].dtype == got["R"].dtype == got["Ub"].dtype == np.dtype(dtype)


def within_4_se(tag, diff):
    mean, se = diff.mean(), diff.std(ddof=1) / math.sqrt(diff.size)
    print(f"{tag}: mean difference {mean:+.3e}, SE {se:.3e} ({mean / se:+.2f} SE)")
    assert se > 0 and abs(mean) <= 4.0 * se, (tag, mean, se)


@pytest.mark.parametrize("name", list(FD_SURFACES))
@pytest.mark.parametrize("payoff", [gr.CALL, gr.PUT])
def test_tangents_against_finite_differences_of_the_restated_price(name, payoff):
    """central differences on the same normals: 1e-3 in X_0, 1e-4 in sigma (everywhere, and row by row), 1e-5 in r and
    q; the bound is 4 SE of the per-path difference (the prototype of the estimators saw 1.4 SE at most)"""
    (grid, sigma), n_steps = FD_SURFACES[name]
    B = grid[0]
    z = fd_normals(n_steps)
    got = gr.samples(z, S0, K, T, R_, Q_, grid, sigma, payoff, B, 0.0)
    q = got["q"]
    # the buckets add up to the parallel vega
    total = q[gr.N_EST:].sum(axis=0)
    worst = np.abs(total - q[gr.VEGA]).max() / np.abs(q[gr.VEGA]).mean()
    print(f"{name}: sum of the buckets against vega {worst:.2e} of mean |vega|")
    assert worst <= 1e-11
    price = lambda x0=0.0, sig=sigma, r=R_, qd=Q_: gr.price_samples(z, S0, K, T, r, qd, grid, sig, payoff, x0)
    h = 1e-3
    fd = (price(x0=h) - price(x0=-h)) / (S0 * math.exp(h) - S0 * math.exp(-h))
    within_4_se(f"{name} payoff {payoff} delta", q[gr.DELTA] - fd)
    h = 1e-4
    within_4_se(f"{name} payoff {payoff} vega", q[gr.VEGA] - (price(sig=sigma + h) - price(sig=sigma - h)) / (2 * h))
    for b in range(B):
        bump = np.zeros_like(sigma)
        bump[b] = h
        within_4_se(f"{name} payoff {payoff} bucket {b}",
                    q[gr.N_EST + b] - (price(sig=sigma + bump) - price(sig=sigma - bump)) / (2 * h))
    # rho and rho_q differentiate e^{-rT} E[y]: the samples carry the -T y of the discount, the finite difference does too
    h = 1e-5
    disc = lambda r: math.exp(-(r - R_) * T)
    within_4_se(f"{name} payoff {payoff} rho", q[gr.RHO] - (disc(R_ + h) * price(r=R_ + h) - disc(R_ - h) * price(r=R_ - h)) / (2 * h))
    within_4_se(f"{name} payoff {payoff} rho_q", q[gr.RHO_Q] - (price(qd=Q_ + h) - price(qd=Q_ - h)) / (2 * h))
    assert (np.abs(q[gr.DELTA]) > 0).mean() > 0.2 and np.isfinite(np.asarray(q, dtype=np.float64)).all()
    if name == "narrow":   # what makes it worth running: most paths end clamped, so most steps have s' = 0
        x = np.log(got["S_T"] / S0)
        assert ((x < -0.047) | (x > 0.053)).mean() > 0.4


# ---- closed forms ----------------------------------------------------------------------------------------------------

def ncdf(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def bs_d1(S, K_, T_, r, q, v):
    return (math.log(S / K_) + (r - q + 0.5 * v * v) * T_) / (v * math.sqrt(T_))


@pytest.mark.parametrize("payoff", [gr.CALL, gr.PUT])
def test_time_only_surface_against_black_scholes_at_the_rms_volatility(payoff):
    """sigma depends on the slice alone: the price is Black-Scholes at the rms volatility vbar, and a shift theta of the
    steps in a set A moves vbar by theta sum_{i in A} s_i / (n vbar): vega = BSvega(vbar) mean(s) / vbar, and bucket b
    = BSvega(vbar) (sum_{i in b} s_i / n) / vbar"""
    vols, n_steps, B, n = (0.15, 0.30, 0.20, 0.25), 12, 3, 1 << 18
    grid, sigma = (4, 2, -1.0, 1.0), np.array([[v, v] for v in vols])
    z = np.random.default_rng(77).standard_normal((n_steps, n))
    q = gr.samples(z, S0, K, T, R_, Q_, grid, sigma, payoff, B, 0.0)["q"]
    s = np.array([vols[lv.row_of(i, 4, n_steps)] for i in range(n_steps)])
    vbar = math.sqrt((s * s).mean())
    d1 = bs_d1(S0, K, T, R_, Q_, vbar)
    bs_vega = S0 * math.exp(-Q_ * T) * math.exp(-0.5 * d1 * d1) / math.sqrt(2 * math.pi) * math.sqrt(T)
    disc = math.exp(-R_ * T)
    omega = -1.0 if payoff == gr.PUT else 1.0
    within_4_se(f"time-only payoff {payoff} price", disc * q[gr.PRICE] - capi.bs_price_f64(S0, K, T, R_, Q_, vbar, payoff))
    within_4_se(f"time-only payoff {payoff} delta", disc * q[gr.DELTA] - omega * math.exp(-Q_ * T) * ncdf(omega * d1))
    within_4_se(f"time-only payoff {payoff} vega", disc * q[gr.VEGA] - bs_vega * s.mean() / vbar)
    for b in range(B):
        in_b = np.array([gr.bucket_of(i, B, n_steps) == b for i in range(n_steps)])
        within_4_se(f"time-only payoff {payoff} bucket {b}", disc * q[gr.N_EST + b] - bs_vega * (s[in_b].sum() / n_steps) / vbar)
    # the surface has no slope: J stays 1 exactly
    assert (gr.samples(z[:, :100], S0, K, T, R_, Q_, grid, sigma, payoff)["J"] == 1.0).all()


def test_displaced_diffusion_delta_and_gamma_against_the_closed_form():
    """r = q = 0, sigma(x) = sigma_d (1 + a / (S0 e^x)) on the 65 nodes of tests/test_localvol_cpu.py: call(K) =
    BS(S0 + a, K + a, sigma_d), so delta = N(d1) at (S0 + a, K + a); gamma against the difference of that delta at
    S+- (the prototype saw 0.7 SE at most)"""
    a, n_steps, n, eta = 50.0, 64, 1 << 19, 0.01
    sigma_d = 0.2 * S0 / (S0 + a)
    grid = (1, 65, -1.5, 1.5)
    sigma = (sigma_d * (1.0 + a / (S0 * np.exp(np.linspace(-1.5, 1.5, 65)))))[None, :]
    z = np.random.default_rng(20240611).standard_normal((n_steps, n))
    main, up, down = gr.walks(z, 1.0, 0.0, 0.0, grid, sigma, 0, eta)
    S_up, S_dn = S0 * math.exp(eta), S0 * math.exp(-eta)
    for K_ in (80.0, 100.0, 125.0):
        q = gr.form(main, S0, K_, 1.0, gr.CALL, np.float64, up, down, eta)["q"]
        delta = lambda S: ncdf(bs_d1(S + a, K_ + a, 1.0, 0.0, 0.0, sigma_d))
        within_4_se(f"displaced K {K_} delta", q[gr.DELTA] - delta(S0))
        within_4_se(f"displaced K {K_} gamma", q[gr.GAMMA] - (delta(S_up) - delta(S_dn)) / (S_up - S_dn))


# ---- the GPU test's inputs: the restatement stays under half the tolerance and under the cap ------------------------------

def test_restatement_stays_under_the_spread_and_the_cap():
    """no kernel runs: on every input of tests/test_gpu_localvol_greeks.py the restatement alone leaves out at most 1 %
    of a case, and its two precisions differ by no more than half the tolerance on every kept path and estimator, i.e.
    the restatement's own rounding uses up at most half of what the kernels are held to"""
    for prec in (cases.F64, cases.F32):
        print(f"prec {prec}: relative restatement spread on the 50-step inputs (price, delta, gamma, vega, rho, rho_q, "
              f"buckets) " + " ".join(f"{v:.2e}" for v in cases.measured_spread(prec)))
    left_out = 0.0
    for case in cases.ALL_CASES:
        own, other, keep, keep3 = cases.compare(case)
        eta, B = case[5], case[6]
        excluded = 1.0 - (keep3 if eta > 0.0 else keep).mean()
        left_out = max(left_out, excluded)
        assert excluded <= cases.CAP, (cases.case_id(case), excluded)
        want = cases.want_of(case)[:gr.N_EST + B]
        tol = cases.tolerance(case, want)
        assert (want[gr.PRICE] != 0).mean() > 0.02
        for e in cases.rows_of(eta, B):
            if case[0] == "node" and e in (gr.DELTA, gr.GAMMA):
                continue   # compared with the restatement of the kernel's own precision only
            k = keep3 if e == gr.GAMMA else keep
            d = np.abs(np.asarray(own["q"][e] - other["q"][e], dtype=np.float64))
            assert (2.0 * d[k] <= tol[e][k]).all(), (cases.case_id(case), e, (d[k] / np.maximum(tol[e][k], 1e-300)).max())
    print(f"largest excluded fraction {left_out:.4f} over {len(cases.ALL_CASES)} cases")
