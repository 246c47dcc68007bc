"""CPU-only checks of the Heston Greeks (include/mcamd_heston_greeks.h).  No kernels run here.

  1. every refusal through both entry points, given no context, in the header's order, each with its own words; the
     cross-compile's resource figures for the twelve kernels;
  2. the host closed form mcamd_heston_greeks_f64 on inputs F, N, H x hr.STRIKES:
       delta against a Richardson central difference R(h) = (4 D(h / 2) - D(h)) / 3 of mcamd_heston_price_f64 in S0.
         The bound: the price is good to EPS = 3e-13 S0 (mcamd.h), so D(h) carries at most EPS / h and R(h) at most
         (4 EPS / (h / 2) + EPS / h) / 3 = 3 EPS / h of rounding; R(h)'s truncation error is 1 / 15 of R(2h) - R(h) (both
         are h^4 rules), and the whole of |R(2h) - R(h)| is allowed for it: fifteen times the estimate.  h = 1 / 8.
       delta_call - delta_put = e^{-qT} to 1e-12;
       below MCAMD_HESTON_XI_MIN with kappa = 0: the Black-Scholes delta with dividend yield at sqrt(v0);
       rho and rho_q against the same Richardson difference in r and in q (h = 1 / 1024);
       gamma as the stated finite difference of the delta, 0 at gamma_eta = 0; rho and rho_q as the stated
         combinations; the parameter entries EQUAL to the stated differences of mcamd_heston_price_f64; its refusals;
  3. the restatement (tests/heston_greeks_cases.py): rows of hr.samples at base and bumped models on shared normals; the
     finalize formulas restated in numpy against mcamd_finalize_heston_greeks_stats on a hand-made record and on the
     restated rows' record to 1e-15 relative; shards add; a subset's record is the full record's slots;
  4. the scheme bias b_k the GPU statistical test allows for (gc.BIAS, measured once at 2^22 paths): a short run of the
     same restatement, 2^16 paths on another generator seed, lies within b_k + 4 of its own SE of the closed form."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import heston_greeks_cases as gc
import heston_restate as hr

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
hg = importlib.import_module("monte-carlo-project-cuda_amd.heston_greeks")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
S0, T_, R, Q = hr.S0, hr.T_, hr.R, hr.Q_DIV
EPS = 3e-13 * S0   # the accuracy include/mcamd.h states for mcamd_heston_price_f64
BUMP5 = gc.bump_list(gc.BUMPS)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return hg.load()


# ---- 1. refusals, resources --------------------------------------------------------------------------------------------

def job(gamma_eta=gc.ETA, reserved=0.0, **bumps):
    j = hg.make_job(gamma_eta, **dict(gc.BUMPS, **bumps))
    j.reserved = reserved
    return j


def refusals():
    """(name, (opt, sim, heston, job), kw, words): what mcamd_price_heston refuses, in its order, then the job's own"""
    from test_heston_cpu import BASE, heston, refusals as heston_refusals
    for name, (opt, sim, hs), kw, words in heston_refusals():
        if name != "no context":
            yield name, (opt, sim, hs, job()), kw, words
    opt, sim, hs = capi.make_option(**BASE), capi.make_sim(1000, 12), heston()
    yield "no job", (opt, sim, hs, None), {}, "job is NULL"
    for value in (1.0, -1.0, NAN, 5e-324):
        yield f"job reserved {value}", (opt, sim, hs, job(reserved=value)), {}, "job->reserved"
    for value in (-1e-300, NAN, INF, -INF):
        yield f"gamma_eta {value}", (opt, sim, hs, job(gamma_eta=value)), {}, "gamma_eta"
    for k, p in enumerate(gc.PARAMS):
        for value in (-1e-300, NAN, INF, -INF):
            yield f"bump {p} {value}", (opt, sim, hs, job(**{p: value})), {}, f"bump[{k}] (of {p})"
    # a bumped model that is no model: F has v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7
    for k, (p, value) in enumerate(zip(gc.PARAMS, (0.0400001, 2.5, 0.05, 0.31, 0.3000001))):
        yield f"{p} - {value} leaves the model", (opt, sim, hs, job(**{p: value})), {}, f"{p} - bump[{k}]"
    yield "rho + bump > 1", (opt, sim, heston(rho=0.96), job()), {}, "rho + bump[4]"
    yield "no context", (opt, sim, hs, job()), {}, "ctx is NULL"


def price(lib, opt, sim, hs, gj, res=True, enqueue=False):
    out = hg.HestonGreeks()
    ref = lambda x: None if x is None else C.byref(x)
    if enqueue:
        rc = lib.mcamd_price_heston_greeks_enqueue(None, ref(opt), ref(sim), ref(hs), ref(gj), None, None)
    else:
        rc = lib.mcamd_price_heston_greeks(None, ref(opt), ref(sim), ref(hs), ref(gj), None, C.byref(out) if res else None)
    return rc, lib.mcamd_last_error().decode()


@pytest.mark.parametrize("case", list(refusals()), ids=lambda c: c[0])
def test_refusals_before_the_context_is_looked_at(lib, case):
    """Every case but the last is wrong in one way only and is given no context: the message names the request's fault,
    so the refusal came before the context."""
    _, args, kw, words = case
    rc, msg = price(lib, *args, **kw)
    assert rc == capi.ERR_INVALID and words in msg, msg
    if kw.get("res", True):   # the enqueue form shares the checks
        rc, msg = price(lib, *args, enqueue=True, **kw)
        assert rc == capi.ERR_INVALID and words in msg, msg


def test_the_refusals_keep_their_order(lib):
    """two faults at once: the earlier stage speaks"""
    from test_heston_cpu import BASE, heston
    opt, sim = capi.make_option(**BASE), capi.make_sim(1000, 12)
    for args, words in (((opt, sim, heston(v0=-1.0), None), ">= 0"),                              # the model before the job
                        ((capi.make_option(**dict(BASE, K=0.0)), sim, heston(), None), "K > 0"),   # opt before the job
                        ((opt, sim, heston(), job(reserved=1.0, gamma_eta=-1.0)), "job->reserved"),
                        ((opt, sim, heston(), job(gamma_eta=-1.0, v0=NAN)), "gamma_eta"),
                        ((opt, sim, heston(), job(v0=NAN, kappa=9.0)), "bump[0] (of v0)"),          # every bump before a model
                        ((opt, sim, heston(), job(v0=1.0, rho=1.0)), "v0 - bump[0]")):             # the models in index order
        rc, msg = price(lib, *args)
        assert rc == capi.ERR_INVALID and words in msg, msg


def test_accepted_requests_reach_the_context(lib):
    from test_heston_cpu import BASE, heston
    sim = capi.make_sim(1000, 12, capi.F32, path_offset=3, n_paths_local=0)
    for gj in (job(), hg.make_job(), hg.make_job(0.5), hg.make_job(0.0, xi=0.3), hg.make_job(0.0, v0=0.04, theta=0.04),
               hg.make_job(0.0, rho=0.3)):   # a bump may take a parameter onto the edge of its range
        rc, msg = price(lib, capi.make_option(**BASE), sim, heston(), gj)
        assert rc == capi.ERR_INVALID and "ctx is NULL" in msg, msg


def test_the_twelve_kernels_use_no_scratch():
    """the cross-compile alone: heston_greeks_kernel<T, P> for two precisions and P = 0 .. 5: no private segment and
    no vector register spilled (tools/isa_diff.py reads the figures; DESIGN records them)"""
    from importlib import util as ilu
    spec = ilu.spec_from_file_location("isa_diff_for_heston_greeks", os.path.join(ROOT, "tools", "isa_diff.py"))
    isa = ilu.module_from_spec(spec)
    spec.loader.exec_module(isa)
    kernels = isa.kernels_of(ROOT, "heston_greeks.hip")
    found = sorted(re.search(r"heston_greeks_kernelI([fd])Li(\d)E", k).groups() for k in kernels)
    assert found == sorted((t, str(p)) for t in "df" for p in range(6)), sorted(kernels)
    for k, (ops, fig) in sorted(kernels.items()):
        print(k, fig)
        assert fig["scratch"] == 0 and fig["vgpr_spill"] == 0 and fig["agpr"] == 0, (k, fig)
        assert fig["vgpr"] <= 256, (k, fig)


# ---- 2. the closed form ------------------------------------------------------------------------------------------------

def closed(name, K, payoff, eta=gc.ETA, bump=BUMP5, S=S0, r=R, **changes):
    q, v0, kappa, theta, xi, rho = hr.params(name, **changes)
    return hg.greeks_closed_form(S, K, T_, r, q, v0, kappa, theta, xi, rho, payoff, eta, bump)


def price_at(name, K, payoff, S=S0, r=R, **changes):
    q, v0, kappa, theta, xi, rho = hr.params(name, **changes)
    return capi.heston_price(S, K, T_, r, q, v0, kappa, theta, xi, rho, payoff)


def richardson(f, x, h):
    """(R(h), the bound on its error): see the module docstring"""
    D = lambda s: (f(x + s) - f(x - s)) / (2.0 * s)
    R_h = (4.0 * D(h / 2) - D(h)) / 3.0
    R_2h = (4.0 * D(h) - D(2 * h)) / 3.0
    return R_h, 3.0 * EPS / h + abs(R_2h - R_h)


CASES = [pytest.param(name, K, payoff, id=f"{name}-{K:g}") for name in "FNH" for K, payoff in hr.STRIKES]


@pytest.mark.parametrize("name,K,payoff", CASES)
def test_delta_rho_and_rho_q_against_richardson_differences_of_the_price(lib, name, K, payoff):
    got = closed(name, K, payoff)
    want, bound = richardson(lambda s: price_at(name, K, payoff, S=s), S0, 0.125)
    print(f"{name} K {K}: delta {got[1]:+.12f} Richardson {want:+.12f} differ {got[1] - want:+.2e} bound {bound:.2e}")
    assert abs(got[1] - want) <= bound and bound < 2e-7
    want, bound = richardson(lambda r: price_at(name, K, payoff, r=r), R, 1.0 / 1024)
    print(f"{name} K {K}: rho {got[3]:+.10f} Richardson {want:+.10f} differ {got[3] - want:+.2e} bound {bound:.2e}")
    assert abs(got[3] - want) <= bound and bound < 1e-5
    want, bound = richardson(lambda q: price_at(name, K, payoff, q=q), Q, 1.0 / 1024)
    print(f"{name} K {K}: rho_q {got[4]:+.10f} Richardson {want:+.10f} differ {got[4] - want:+.2e} bound {bound:.2e}")
    assert abs(got[4] - want) <= bound and bound < 1e-5
    assert got[0] == price_at(name, K, payoff)
    assert got[3] == T_ * (S0 * got[1] - got[0]) and got[4] == -T_ * S0 * got[1]


@pytest.mark.parametrize("name,K,payoff", CASES)
def test_delta_parity_gamma_and_the_parameter_differences(lib, name, K, payoff):
    got, other = closed(name, K, payoff), closed(name, K, 1 - payoff)
    call, put = (got, other) if payoff == hr.CALL else (other, got)
    assert abs(call[1] - put[1] - math.exp(-Q * T_)) <= 1e-12
    up, dn = math.exp(gc.ETA), math.exp(-gc.ETA)
    d_up, d_dn = closed(name, K, payoff, S=S0 * up)[1], closed(name, K, payoff, S=S0 * dn)[1]
    assert got[2] == (d_up - d_dn) / (S0 * (up - dn)) and got[2] > 0
    assert abs(call[2] - put[2]) <= 1e-12            # parity: the same gamma
    base = dict(zip(gc.PARAMS, hr.MODELS[name]))
    for k, p in enumerate(gc.PARAMS):
        b = gc.BUMPS[p]
        want = (price_at(name, K, payoff, **{p: base[p] + b}) - price_at(name, K, payoff, **{p: base[p] - b})) / (2.0 * b)
        assert got[5 + k] == want and want != 0.0, p
    none = closed(name, K, payoff, eta=0.0, bump=[0.0] * 5)
    assert none[:2] == got[:2] and none[3:5] == got[3:5] and none[2] == 0.0 and none[5:] == [0.0] * 5
    only = closed(name, K, payoff, eta=0.0, bump=[0.0, 0.0, 0.0, gc.BUMPS["xi"], 0.0])
    assert only[8] == got[8] and only[5:8] == [0.0] * 3 and only[9] == 0.0


def test_deterministic_variance_gives_the_black_scholes_delta(lib):
    none = [0.0] * 5   # xi - bump would leave the model
    for xi in (0.0, 0.5 * capi.HESTON_XI_MIN):
        for K, payoff in hr.STRIKES:
            got = closed("F", K, payoff, bump=none, kappa=0.0, xi=xi, theta=0.3)
            v = math.sqrt(hr.MODELS["F"][0])
            d1 = (math.log(S0 / K) + (R - Q + 0.5 * v * v) * T_) / (v * math.sqrt(T_))
            N = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))
            want = math.exp(-Q * T_) * (N(d1) if payoff == hr.CALL else -N(-d1))
            assert abs(got[1] - want) <= 1e-15 and abs(got[0] - capi.bs_price_f64(S0, K, T_, R, Q, v, payoff)) <= 1e-13
    # continuity across the threshold: the integral just above it
    for K, payoff in hr.STRIKES:
        below = closed("F", K, payoff, bump=none, xi=0.5 * capi.HESTON_XI_MIN)[1]
        above = closed("F", K, payoff, bump=none, xi=2.0 * capi.HESTON_XI_MIN)[1]
        assert abs(below - above) <= 1e-8
    # no variance at all: the step function of the forward
    assert closed("F", 90.0, hr.CALL, v0=0.0, theta=0.0, xi=0.0, bump=none)[1] == math.exp(-Q * T_)
    assert closed("F", 120.0, hr.CALL, v0=0.0, theta=0.0, xi=0.0, bump=none)[1] == 0.0


def test_closed_form_refusals(lib):
    q, v0, kappa, theta, xi, rho = hr.params("F")
    out, bump = (C.c_double * 10)(*[7.0] * 10), (C.c_double * 5)(*BUMP5)

    def call(S=S0, K=100.0, T=T_, xi_=xi, payoff=0, eta=gc.ETA, bump_=bump, out_=out):
        rc = lib.mcamd_heston_greeks_f64(S, K, T, R, q, v0, kappa, theta, xi_, rho, payoff, eta, bump_, out_)
        return rc, lib.mcamd_last_error().decode()

    assert call()[0] == capi.OK and out[0] > 0
    for kw, words in ((dict(out_=None), "non-NULL"), (dict(bump_=None), "non-NULL"), (dict(payoff=2), "payoff"),
                      (dict(S=0.0), "S0"), (dict(K=-1.0), "K"), (dict(T=0.0), "T > 0"), (dict(xi_=-0.1), ">= 0"),
                      (dict(eta=-1.0), "gamma_eta"), (dict(eta=NAN), "gamma_eta"),
                      (dict(bump_=(C.c_double * 5)(0, 0, -1.0, 0, 0)), "bump[2]"),
                      (dict(bump_=(C.c_double * 5)(0, 0, 0, INF, 0)), "bump[3]"),
                      (dict(bump_=(C.c_double * 5)(0.05, 0, 0, 0, 0)), ">= 0"),       # v0 - bump < 0
                      (dict(bump_=(C.c_double * 5)(0, 0, 0, 0, 0.4)), "rho")):        # rho - bump < -1
        rc, msg = call(**kw)
        assert rc == capi.ERR_INVALID and words in msg, (kw, msg)
        if kw.get("out_", out) is not None:
            assert list(out) == [0.0] * 10
            call()


# ---- 3. the restatement ------------------------------------------------------------------------------------------------

def normals(n_steps, n, seed=11):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_steps, n)), rng.standard_normal((n_steps, n))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restated_rows_are_the_samples_of_the_bumped_models(dtype):
    z, zv = normals(24, 500)
    n_band = 0
    for name in "FNH":
        for K, payoff in hr.STRIKES:
            rows, base = gc.restated_rows(z, zv, name, K, payoff, gc.ETA, gc.BUMPS, dtype)
            assert rows.shape == (13, 500) and rows.dtype == np.dtype(dtype)
            assert np.array_equal(rows[0].astype(np.float64), base["y"])
            for j, (label, params) in enumerate(gc.walks(name, gc.BUMPS)[1:]):
                want = hr.samples(z, zv, S0, K, T_, R, params, payoff, dtype)
                assert np.array_equal(rows[3 + j].astype(np.float64), want["y"]), label
                # another path, whatever the payoff shows of it (on H a path whose v+ stays 0 reads no parameter)
                assert (want["S_T"] != base["S_T"]).mean() > 0.5, label
            S_T, sgn = base["S_T"], (-1 if payoff == hr.PUT else 1)
            itm = rows[0] > 0
            assert np.array_equal(rows[1], np.where(itm, sgn * S_T, 0)) and (sgn * rows[1] >= 0).all()
            band = rows[2] != 0
            assert (rows[2][band] == S_T[band]).all() and not np.signbit(rows[2]).any()
            # the band is where S_T lies within a factor e^{+-eta} of the strike
            n_band += int(band.sum())
            assert (np.abs(np.log(S_T[band].astype(np.float64) / K)) <= gc.ETA * 1.0001).all()
            assert (np.abs(np.log(S_T[~band].astype(np.float64) / K)) >= gc.ETA * 0.9999).all()
            none = gc.rows_from_state(S_T, [], K, payoff, 0.0)
            assert not none[2].any()
    assert n_band > 50


def hand_made_record(P):
    """a record no simulation made: sums whose variances are positive, in the layout of P requested parameters"""
    n = 1000.0
    rec = [5.0e3, 9.1e4, 4.2e4, 6.3e6, 5.9e6, 3.7e3, 5.5e5]
    for j in range(P):
        rec += [(-1.0) ** j * 37.5 * (j + 1), 9.75 * (j + 2)]
    rec += [1234.0, 41.5, n]
    return rec + [0.0] * (gc.STATS - len(rec))


@pytest.mark.parametrize("subset", [(), ("xi",), ("v0", "rho"), ("kappa", "theta", "xi"), gc.PARAMS],
                         ids=lambda s: str(len(s)))
def test_finalize_is_the_headers_formulas(lib, subset):
    bumps = {p: gc.BUMPS[p] for p in subset}
    for eta in (gc.ETA, 0.0):
        gj = hg.make_job(eta, **bumps)
        opt = capi.make_option(S0=S0, K=100.0, r=R, T=T_)
        rec = hand_made_record(len(subset))
        got = hg.finalize_stats(rec, opt, gj)
        value, se, trunc, rv = gc.finalize(rec, S0, R, T_, eta, gc.bump_list(bumps))
        assert (got.n, got.truncated_steps, got.mean_variance) == (1000, trunc, rv) == (1000, 1234.0, 41.5 / 1000)
        assert (got.work_steps, got.kernel_ms, got.total_ms, got.grid, got.block) == (0, 0, 0, 0, 0)
        for k, what in enumerate(gc.NAMES):
            wanted = k < 5 and (k != 2 or eta > 0) or (k >= 5 and gc.PARAMS[k - 5] in subset)
            if not wanted:
                assert (got.value[k], got.std_err[k]) == (0.0, 0.0) == (value[k], se[k]), what
                continue
            assert se[k] > 0 and value[k] != 0
            assert abs(got.value[k] - value[k]) <= 1e-15 * abs(value[k]), what
            assert abs(got.std_err[k] - se[k]) <= 1e-15 * se[k], what
        assert got.as_dict()["delta"] == (got.value[1], got.std_err[1])
    # n = 0: zeros; its refusals
    zero = hg.finalize_stats([0.0] * 32, opt, gj)
    assert not any(zero.value) and not any(zero.std_err) and zero.n == 0 and zero.mean_variance == 0
    out, stats = hg.HestonGreeks(), (C.c_double * 32)()
    for args, words in (((None, opt, gj, out), "non-NULL"), ((stats, None, gj, out), "non-NULL"),
                        ((stats, opt, None, out), "non-NULL"), ((stats, opt, gj, None), "non-NULL"),
                        ((stats, opt, job(reserved=2.0), out), "job->reserved"),
                        ((stats, opt, job(gamma_eta=-1.0), out), "gamma_eta"), ((stats, opt, job(xi=NAN), out), "bump[3]"),
                        ((stats, capi.make_option(S0=0.0), gj, out), "S0 > 0"),
                        ((stats, capi.make_option(r=INF), gj, out), "finite")):
        ref = lambda x: None if x is None else C.byref(x)
        rc = lib.mcamd_finalize_heston_greeks_stats(args[0], ref(args[1]), ref(args[2]), ref(args[3]))
        assert rc == capi.ERR_INVALID and words in lib.mcamd_last_error().decode(), words


def test_records_of_shards_add_and_a_subset_is_the_full_records_slots(lib):
    z, zv = normals(12, 900, seed=5)
    K, payoff = hr.STRIKES[1]
    rows, base = gc.restated_rows(z, zv, "N", K, payoff, gc.ETA, gc.BUMPS)
    whole = gc.record(rows, base["trunc"].sum(), base["rv"].sum())
    assert whole[19] == 900 and not whole[20:].any() and whole[17] == base["trunc"].sum() > 0
    parts = np.zeros(gc.STATS)
    for lo, hi in ((0, 100), (100, 101), (101, 900)):
        parts += gc.record(rows[:, lo:hi], base["trunc"][lo:hi].sum(), base["rv"][lo:hi].sum())
    assert parts[19] == 900 and parts[17] == whole[17]
    opt = capi.make_option(S0=S0, K=K, r=R, T=T_)
    a, b = hg.finalize_stats(parts, opt, job()), hg.finalize_stats(whole, opt, job())
    for k in range(hg.GREEKS):
        assert abs(a.value[k] - b.value[k]) <= 1e-12 * (abs(b.value[k]) + 30 * b.std_err[k])
        assert abs(a.std_err[k] - b.std_err[k]) <= 1e-11 * b.std_err[k]
    # the restated values against the C finalize of the restated record
    value, se, _, _ = gc.finalize(whole, S0, R, T_, gc.ETA, BUMP5)
    assert all(abs(b.value[k] - value[k]) <= 1e-15 * abs(value[k]) and abs(b.std_err[k] - se[k]) <= 1e-15 * se[k]
               for k in range(hg.GREEKS))
    # a subset's rows are the full request's, so its record is the full one's slots, moved up
    sub_rows, _ = gc.restated_rows(z, zv, "N", K, payoff, gc.ETA, dict(kappa=gc.BUMPS["kappa"], rho=gc.BUMPS["rho"]))
    assert np.array_equal(sub_rows, rows[[0, 1, 2, 5, 6, 11, 12]])
    sub = gc.record(sub_rows, base["trunc"].sum(), base["rv"].sum())
    assert list(sub[:14]) == list(whole[[0, 1, 2, 3, 4, 5, 6, 9, 10, 15, 16, 17, 18, 19]]) and not sub[14:].any()


# ---- 4. the scheme bias --------------------------------------------------------------------------------------------------

def test_a_short_run_of_the_restatement_lies_within_the_recorded_bias(lib):
    assert set(gc.BIAS) == set(gc.STAT_STRIKES) and all(len(b) == 10 and min(b) > 0 for b in gc.BIAS.values())
    est = gc.restated_estimate(2 ** 16, 2 ** 15, np.random.default_rng(7))
    for (K, payoff), (value, se) in est.items():
        want = closed("F", K, payoff)
        for k, what in enumerate(gc.NAMES):
            print(f"K {K} {what:6s}: closed {want[k]:+.6f} restated {value[k]:+.6f} SE {se[k]:.6f} b {gc.BIAS[(K, payoff)][k]:.2e}")
            assert abs(value[k] - want[k]) <= gc.BIAS[(K, payoff)][k] + 4.0 * se[k], what
