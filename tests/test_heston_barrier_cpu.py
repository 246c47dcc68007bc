"""CPU-only checks of the Heston barrier call (include/mcamd.h, mcamd_price_heston_barrier).  No kernels run here.

  1. declarations, struct layout and exported symbols; the cross-compile's resource figures for the 16 kernels;
  2. every refusal through both entry points, given no context, and the order of the four groups of refusals;
  3. a barrier nobody reaches (B = 1e-30 down, 1e30 up): the knock-out's y, S_T, v_n and trunc are
     heston_restate.samples' bit for bit, the knock-in's y is 0, w is 1;
  4. xi = 0, kappa = 0, q = 0, v0 = fl(0.2 * 0.2) against barrier_restate.samples in all 16 kind x monitoring x payoff
     cases: S_T bit-equal in float64, y within 1e-12 of the payoff scale (the rule DESIGN.md section 18 used for the
     flat surface);
  5. per path y_out + y_in = h(S_T) to rounding, and w_continuous <= w_discrete;
  6. the exact check: with rho = 0 and r = q the continuous sample's expectation given the variance path is
     mcamd_barrier_price_f64 at r = 0 and v = sqrt(sum_i v+_i dt / T), at EVERY n_steps.  F and N, 1, 4 and 16 steps, all
     eight kind x payoff cases, 200k Philox paths: |mean(y_j - c_j)| <= 4 SE(y_j - c_j) on the same paths;
  7. the left-out rule: on every elementwise case of the GPU test the restatement leaves out at most 3 % of the paths;
  8. the precision spread of the restatement, which fixes the GPU tolerances (tests/heston_barrier_cases.py)."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import barrier_restate as br
import heston_barrier_cases as hbc
import heston_barrier_restate as hbr
import heston_cases as hc
import heston_restate as hr
from deep_inputs import SHALLOW

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcamd_price_heston_barrier", "mcamd_price_heston_barrier_enqueue")
NAN, INF = float("nan"), float("inf")
S0, T_, R, Q = hr.S0, hr.T_, hr.R, hr.Q_DIV


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


def header():
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        return f.read()


# ---- 1. declarations, layout, resources ----------------------------------------------------------------------------------

def test_header_declares_the_calls_and_the_struct(lib):
    text = header()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert re.search(r"\}\s*mcamd_heston_barrier_result\s*;", text)
    assert re.search(r"#define\s+MCAMD_ABI_VERSION\s+5\b", text) and lib.mcamd_abi_version() == 5
    assert "first carried by the build that ships csrc/heston_barrier.hip" in text
    assert not re.search(r"mcamd_group_\w*heston", text)
    assert hasattr(capi.Context, "price_heston_barrier") and hasattr(capi.Context, "price_heston_barrier_enqueue")
    build = importlib.import_module("monte-carlo-project-cuda_amd.build")
    assert "heston_barrier.hip" in build.SOURCES and "heston_barrier.hpp" in build.HEADERS


def test_result_struct_matches_the_header():
    # static_assert(sizeof(mcamd_heston_barrier_result) == 104) in csrc/capi_heston.cpp
    Rs = capi.HestonBarrierResult
    assert C.sizeof(Rs) == 104 and C.sizeof(capi.Heston) == 64 and C.sizeof(capi.Barrier) == 16
    assert [(k, getattr(Rs, k).offset) for k, _ in Rs._fields_] == [
        ("price", 0), ("std_err", 8), ("ci_lo", 16), ("ci_hi", 24), ("sum", 32), ("sumsq", 40), ("n", 48),
        ("live_steps", 56), ("work_steps", 64), ("truncated_steps", 72), ("mean_variance", 80), ("kernel_ms", 88),
        ("total_ms", 92), ("grid", 96), ("block", 100)]
    body = re.search(r"typedef struct mcamd_heston_barrier_result \{(.*?)\}", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"\w+\s+([\w\s,]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [k for k, _ in Rs._fields_]   # the same fields in the same order


def test_the_sixteen_kernels_use_no_scratch():
    """the cross-compile alone: heston_barrier_kernel<T, UP, CONT, OUT> for two precisions, no private segment, no
    spilled vector register, and no LDS beyond what MathCtx<T> and the sums need (tools/isa_diff.py reads the
    figures).  Scalar registers parked in vector lanes are recorded, not refused: the fp64 continuous kernels of
    localvol.hip park some too, and none of it is memory."""
    from importlib import util as ilu
    spec = ilu.spec_from_file_location("isa_diff_for_heston_barrier", os.path.join(ROOT, "tools", "isa_diff.py"))
    isa = ilu.module_from_spec(spec)
    spec.loader.exec_module(isa)
    kernels = isa.kernels_of(ROOT, "heston_barrier.hip")
    found = sorted(re.search(r"heston_barrier_kernelI([fd])Lb([01])ELb([01])ELb([01])E", k).groups() for k in kernels)
    assert found == sorted((t, u, c, o) for t in "df" for u in "01" for c in "01" for o in "01"), sorted(kernels)
    for k, (ops, fig) in sorted(kernels.items()):
        print(k, fig)
        assert fig["scratch"] == 0 and fig["vgpr_spill"] == 0 and fig["agpr"] == 0, (k, fig)
        assert fig["lds"] < (1024 if "kernelIf" in k else 21 * 1024), (k, fig)


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------

BASE = dict(S0=S0, K=100.0, v=NAN, B=90.0, r=R, T=T_)   # opt->v is ignored


def heston(payoff=capi.PAYOFF_CALL, **kw):
    q, v0, kappa, theta, xi, rho = hr.params("F")
    return capi.make_heston(payoff, **dict(dict(q=q, v0=v0, kappa=kappa, theta=theta, xi=xi, rho=rho), **kw))


def barrier(kind=capi.BARRIER_DOWN_OUT, payoff=capi.PAYOFF_CALL, monitoring=capi.MONITOR_CONTINUOUS, reserved=0):
    b = capi.make_barrier(kind, payoff, monitoring)
    b.reserved = reserved
    return b


def price(lib, opt, sim, hs, bar, res=True, enqueue=False, ctx=None, stats=None):
    out = capi.HestonBarrierResult()
    ref = lambda x: None if x is None else C.byref(x)
    if enqueue:
        rc = lib.mcamd_price_heston_barrier_enqueue(ctx, ref(opt), ref(sim), ref(hs), ref(bar), None, None, stats)
    else:
        rc = lib.mcamd_price_heston_barrier(ctx, ref(opt), ref(sim), ref(hs), ref(bar), None, None,
                                            C.byref(out) if res else None)
    assert all(v == 0 for v in out.as_dict().values())
    return rc, lib.mcamd_last_error().decode()


def refusals():
    """(name, (opt, sim, heston, barrier), kw, words of the message), in the order the header states"""
    O, S = capi.make_option, capi.make_sim
    opt, sim, hs, bar = O(**BASE), S(1000, 12), heston(), barrier()
    yield "no opt", (None, sim, hs, bar), {}, "non-NULL"
    yield "no sim", (opt, None, hs, bar), {}, "non-NULL"
    yield "no heston", (opt, sim, None, bar), {}, "non-NULL"
    yield "no barrier", (opt, sim, hs, None), {}, "non-NULL"
    yield "no res", (opt, sim, hs, bar), dict(res=False), "non-NULL"
    # what mcamd_price_barrier refuses of the barrier
    for monitoring in (-1, 2):
        yield f"monitoring {monitoring}", (opt, sim, hs, barrier(monitoring=monitoring)), {}, "monitoring"
    for reserved in (1, -1):
        yield f"barrier reserved {reserved}", (opt, sim, hs, barrier(reserved=reserved)), {}, "barrier->reserved"
    for kind in (-1, 4):
        yield f"kind {kind}", (opt, sim, hs, barrier(kind=kind)), {}, "barrier kind"
    for payoff in (-1, 2):
        yield f"barrier payoff {payoff}", (opt, sim, hs, barrier(payoff=payoff)), {}, "payoff"
    for B in (0.0, -1.0, NAN, INF):
        yield f"B = {B}", (O(**dict(BASE, B=B)), sim, hs, bar), {}, "barrier level"
    for kind, B in ((capi.BARRIER_DOWN_OUT, 100.0), (capi.BARRIER_DOWN_IN, 110.0), (capi.BARRIER_UP_OUT, 100.0),
                    (capi.BARRIER_UP_IN, 90.0)):
        yield f"kind {kind} at B = {B}", (O(**dict(BASE, B=B)), sim, hs, barrier(kind=kind)), {}, "live side"
    for value in (NAN, 0.0, -1.0, INF):
        yield f"S0 = {value}", (O(**dict(BASE, S0=value)), sim, hs, bar), {}, "live side"
    # what mcamd_price_heston refuses
    for payoff in (-1, 2):
        yield f"heston payoff {payoff}", (opt, sim, heston(payoff), bar), {}, "payoff"
    for scheme in (-1, 1):
        yield f"scheme {scheme}", (opt, sim, heston(scheme=scheme), bar), {}, "scheme"
    for value in (1.0, -1.0, NAN, 5e-324):
        bad = heston()
        bad.reserved = value
        yield f"heston reserved {value}", (opt, sim, bad, bar), {}, "heston->reserved"
    for field in ("q", "v0", "kappa", "theta", "xi", "rho"):
        for value in (NAN, INF, -INF):
            yield f"{field} = {value}", (opt, sim, heston(**{field: value}), bar), {}, "must be finite"
    for field in ("v0", "kappa", "theta", "xi"):
        yield f"{field} < 0", (opt, sim, heston(**{field: -1e-300}), bar), {}, ">= 0"
    for rho in (1.0000000000000002, -1.5):
        yield f"rho = {rho}", (opt, sim, heston(rho=rho), bar), {}, "rho"
    yield "r = nan", (O(**dict(BASE, r=NAN)), sim, hs, bar), {}, "finite"
    yield "use_window", (O(**BASE, use_window=1), sim, hs, bar), {}, "window"
    yield "P1", (O(**BASE, P1=1), sim, hs, bar), {}, "window"
    yield "P2", (O(**BASE, P2=3), sim, hs, bar), {}, "window"
    yield "Ik", (O(**BASE, Ik=2), sim, hs, bar), {}, "window"
    yield "Sk", (O(**BASE, Sk=95.0), sim, hs, bar), {}, "Sk"
    yield "Tk", (O(**BASE, Tk=5), sim, hs, bar), {}, "Tk"
    yield "dt", (O(**BASE, dt=0.01), sim, hs, bar), {}, "dt"
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE, capi.FLAG_PRODUCT_FORM,
                  capi.FLAG_LOG_SPACE | capi.FLAG_ANTITHETIC, capi.FLAG_LOG_SPACE | capi.FLAG_PRODUCT_FORM, 32):
        yield f"flags {flags}", (opt, S(1000, 12, flags=flags), hs, bar), {}, "flags"
    yield "precision", (opt, S(1000, 12, precision=16), hs, bar), {}, "precision"
    yield "n_steps 0", (opt, S(1000, 0), hs, bar), {}, "n_steps"
    yield "shard overflow", (opt, S(1 << 63, 12, path_offset=(1 << 64) - 10, n_paths_local=100), hs, bar), {}, "overflows"
    yield "exponent range", (O(**dict(BASE, T=100.0)), sim, heston(q=-1e4), bar), {}, "exponent range"
    yield "T = 0", (O(**dict(BASE, T=0.0)), sim, hs, bar), {}, "T > 0"
    yield "T = inf", (O(**dict(BASE, T=INF)), sim, hs, bar), {}, "finite"
    yield "K = nan", (O(**dict(BASE, K=NAN)), sim, hs, bar), {}, "finite"
    for value in (0.0, -1.0):
        yield f"K = {value}", (O(**dict(BASE, K=value)), sim, hs, bar), {}, "S0 > 0 and K > 0"
    # the payoff stated twice
    yield "call and put", (opt, sim, heston(capi.PAYOFF_CALL), barrier(payoff=capi.PAYOFF_PUT)), {}, "the same payoff"
    yield "put and call", (opt, sim, heston(capi.PAYOFF_PUT), barrier(payoff=capi.PAYOFF_CALL)), {}, "the same payoff"
    # then the context
    yield "no context", (opt, sim, hs, bar), {}, "ctx is NULL"


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


def test_refusals_come_in_the_stated_order(lib):
    """a request wrong in two ways is refused for the earlier one: the barrier, then the Heston job, the model, r, opt's
    other fields and sim, S0 and K, then the two payoffs, then the context"""
    O, S = capi.make_option, capi.make_sim
    opt, sim = O(**BASE), S(1000, 12)
    mismatch = (heston(capi.PAYOFF_CALL), barrier(payoff=capi.PAYOFF_PUT))
    twice = [
        ((opt, sim, heston(scheme=1), barrier(monitoring=2)), "monitoring"),
        ((opt, sim, heston(scheme=1), barrier(reserved=1)), "barrier->reserved"),
        ((opt, sim, heston(2), barrier(kind=4)), "barrier kind"),
        ((O(**dict(BASE, B=-1.0)), sim, heston(v0=-1.0), barrier()), "barrier level"),
        ((O(**dict(BASE, B=100.0)), S(1000, 0), heston(), barrier()), "live side"),
        ((opt, S(1000, 0), heston(scheme=1), barrier()), "scheme"),
        ((O(**dict(BASE, K=0.0)), S(1000, 0), heston(), barrier()), "n_steps"),
        ((O(**dict(BASE, K=0.0)), sim, *mismatch), "S0 > 0 and K > 0"),
        ((opt, S(1000, 12, flags=32), *mismatch), "flags"),
        ((opt, sim, *mismatch), "the same payoff"),
    ]
    for args, words in twice:
        for enqueue in (False, True):
            rc, msg = price(lib, *args, enqueue=enqueue)
            assert rc == capi.ERR_INVALID and words in msg, (words, msg)


@pytest.mark.parametrize("flags,prec", [(0, capi.F64), (capi.FLAG_LOG_SPACE, capi.F32)])
def test_accepted_requests_reach_the_context(lib, flags, prec):
    sim = capi.make_sim(1000, 12, prec, flags=flags, path_offset=3, n_paths_local=0)
    for kind in br.KINDS:
        opt = capi.make_option(**dict(BASE, B=hbc.LEVEL[kind], v=-1.0))
        for mon in (capi.MONITOR_DISCRETE, capi.MONITOR_CONTINUOUS):
            for payoff in (capi.PAYOFF_CALL, capi.PAYOFF_PUT):
                for kw in (dict(), dict(xi=0.0, kappa=0.0), dict(rho=1.0), dict(v0=0.0, theta=0.0)):
                    rc, msg = price(lib, opt, sim, heston(payoff, **kw), barrier(kind, payoff, mon))
                    assert rc == capi.ERR_INVALID and "ctx is NULL" in msg, (kind, mon, payoff, kw, msg)


# ---- 3. a barrier nobody reaches --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n_steps", [50, 5, 1])
def test_unreachable_barrier_is_the_european_heston_path(dtype, n_steps):
    prec = hc.F64 if dtype == np.float64 else hc.F32
    z, zv = hr.draws(prec, SHALLOW[0], SHALLOW[1], 256, n_steps)
    for name in ("F", "N", "H"):
        p = hr.params(name)
        for payoff in (br.CALL, br.PUT):
            want = hr.samples(z, zv, S0, 100.0, T_, R, p, payoff, dtype)
            for kind in br.KINDS:
                B = 1e30 if br.is_up(kind) else 1e-30
                for mon in (br.DISCRETE, br.CONTINUOUS):
                    got = hbr.samples(z, zv, S0, 100.0, B, T_, R, p, kind, payoff, mon, dtype)
                    assert (got["w"] == 1).all() and (got["live"] == n_steps).all()
                    assert np.array_equal(got["S_T"], want["S_T"]) and np.array_equal(got["v_n"], want["v_n"])
                    assert np.array_equal(got["trunc"], want["trunc"])
                    assert np.array_equal(got["vs"].astype(np.float64) * (1.0 / n_steps), want["rv"])
                    if br.is_out(kind):
                        assert np.array_equal(got["y"], want["y"])
                    else:
                        assert not got["y"].any()


# ---- 4. xi = 0, kappa = 0: the constant-volatility barrier ------------------------------------------------------------------

@pytest.mark.parametrize("n_steps", [50, 3, 1])
def test_constant_variance_is_the_barrier_restatement(n_steps):
    """v0 = 0.2 * 0.2 as float64 rounds it, so that sqrt(v0) is 0.2 and s s is v0 again, bit for bit"""
    sigma = np.float64(0.2)
    v0 = float(sigma * sigma)
    assert np.sqrt(np.float64(v0)) == sigma and v0 != 0.04
    z, zv = hr.draws(64, SHALLOW[0], SHALLOW[1], 256, n_steps)
    p = hr.params("F", q=0.0, v0=v0, xi=0.0, kappa=0.0, theta=0.3)
    worst = 0.0
    for kind, mon, payoff in hbc.CASES:
        B = hbc.LEVEL[kind]
        got = hbr.samples(z, zv, S0, 100.0, B, T_, R, p, kind, payoff, mon)
        want = br.samples(z, S0, 100.0, B, T_, R, float(sigma), kind, payoff, mon)
        assert np.array_equal(got["S_T"], want["S_T"]) and np.array_equal(got["live"], want["live"])
        assert (got["v_n"] == v0).all() and not got["trunc"].any()
        worst = max(worst, float(np.abs(got["y"] - want["y"]).max()), float(np.abs(got["w"] - want["w"]).max()) * S0)
        assert np.abs(got["y"] - want["y"]).max() <= 1e-12 * S0, (kind, mon, payoff)
        assert np.abs(got["w"] - want["w"]).max() <= 1e-12
    if n_steps == 50:
        assert 0 < want["live"].sum() < 256 * n_steps   # some paths are hit, some are not
    print(f"{n_steps} steps: worst deviation from the constant-volatility barrier restatement {worst:.2e}")


# ---- 5. in plus out, continuous below discrete -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["F", "N", "H"])
def test_in_plus_out_is_the_european_payoff_and_the_bridge_only_removes_weight(name):
    for n_steps, where in hbc.SHAPES:
        for up_kinds in ((br.DOWN_OUT, br.DOWN_IN), (br.UP_OUT, br.UP_IN)):
            for payoff in (br.CALL, br.PUT):
                w_of = {}
                for mon in (br.DISCRETE, br.CONTINUOUS):
                    out, in_ = (hbc.restate(hc.F64, name, n_steps, where, hbc.N_PATHS, (kind, mon, payoff), np.float64)
                                for kind in up_kinds)
                    assert np.array_equal(out["S_T"], in_["S_T"]) and np.array_equal(out["w"], in_["w"])
                    assert np.abs((out["y"] + in_["y"]) - out["h"]).max() <= 4 * np.finfo(np.float64).eps * S0
                    assert ((out["w"] >= 0) & (out["w"] <= 1)).all()
                    # a knock-in counts every step, a knock-out its live ones
                    assert (in_["counted"] == n_steps).all() and np.array_equal(out["counted"], out["live"])
                    assert (out["trunc"] <= in_["trunc"]).all() and (out["vs"] <= in_["vs"]).all()
                    w_of[mon] = out["w"]
                assert (w_of[br.CONTINUOUS] <= w_of[br.DISCRETE]).all()
                assert set(np.unique(w_of[br.DISCRETE])) <= {0.0, 1.0}
                if n_steps == 50:
                    assert (w_of[br.CONTINUOUS] < w_of[br.DISCRETE]).any()


# ---- 6. the exact check ------------------------------------------------------------------------------------------------------

EXACT_PATHS = 200_000


@pytest.mark.parametrize("n_steps", [1, 4, 16])
@pytest.mark.parametrize("name", ["F", "N"])
def test_continuous_sample_has_the_exact_conditional_expectation(lib, name, n_steps):
    """the 4 is the project's usual statistical margin; nothing is measured to set it"""
    r, p = hbc.exact_inputs(name)
    seed = 6000 + 100 * n_steps + ord(name)
    z = hr.philox_normals_f64(seed, 0, EXACT_PATHS, n_steps)
    zv = hr.philox_normals_f64(seed, 0, EXACT_PATHS, n_steps, hr.VARIANCE_BLOCKS)
    clock = hbr.variance_clock(zv, T_, p)
    assert (clock > 0).all()
    for kind in br.KINDS:
        for payoff in (br.CALL, br.PUT):
            got = hbr.samples(z, zv, S0, hbc.STRIKE, hbc.LEVEL[kind], T_, r, p, kind, payoff, br.CONTINUOUS)
            if not br.is_out(kind):   # a knock-in counts every step: its vs is the clock
                assert np.abs(got["vs"] * (T_ / n_steps) - clock).max() <= 1e-14
            c = hbc.conditional_expectation(capi, clock, kind, payoff)
            mean, se = hbc.mean_in_standard_errors(got["y"], c)
            print(f"{name} {n_steps} steps kind {kind} payoff {payoff}: mean y {got['y'].mean():.5f}, mean c {c.mean():.5f}, "
                  f"mean(y - c) {mean:+.2e} = {mean / se:+.2f} SE (SE {se:.2e}); discrete sample's mean "
                  f"{discrete_mean(z, zv, r, p, kind, payoff):.5f}")
            assert se > 0 and abs(mean) <= 4.0 * se


def discrete_mean(z, zv, r, p, kind, payoff):
    return float(hbr.samples(z, zv, S0, hbc.STRIKE, hbc.LEVEL[kind], T_, r, p, kind, payoff, br.DISCRETE)["y"].mean())


# ---- 7. the left-out rule ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,precs", hbc.ELEMENTWISE, ids=[m for m, _ in hbc.ELEMENTWISE])
def test_restatement_leaves_out_at_most_three_percent_of_any_elementwise_case(name, precs):
    for prec in precs:
        for n_steps, where in hbc.SHAPES:
            for kind in (br.DOWN_OUT, br.UP_OUT):   # the distances depend on the level alone
                keep = hbc.kept(prec, name, n_steps, where, hbc.N_PATHS, (kind, br.DISCRETE, br.CALL))
                share = 1.0 - keep.mean()
                print(f"{name} fp{prec} {n_steps} steps at id {where[1]} level {hbc.LEVEL[kind]}: left out "
                      f"{hbc.N_PATHS - int(keep.sum())} of {hbc.N_PATHS} ({100 * share:.2f} %)")
                assert share <= hbc.LEFT_CAP


# ---- 8. the precision spread, which fixes the GPU tolerances -------------------------------------------------------------------

@pytest.mark.parametrize("name,precs", hbc.ELEMENTWISE, ids=[m for m, _ in hbc.ELEMENTWISE])
def test_precision_spread_of_the_restatement(name, precs):
    for prec in precs:
        s, tol = hbc.spread(prec, name), hbc.tolerance(prec, name)
        print(f"{name} fp{prec}: spread " + ", ".join(f"{k} {s[k]:.2e}" for k in s) + "; tolerance " +
              ", ".join(f"{k} {tol[k]:.2e}" for k in tol) + "; decided by the " +
              ", ".join(f"{k}: {'spread' if 4.0 * s[k] > hbc.FLOOR[prec][k] else 'floor'}" for k in s))
        assert all(math.isfinite(x) for x in s.values())
        assert all(tol[k] >= hbc.FLOOR[prec][k] and tol[k] >= 4.0 * s[k] for k in s)
        # the walk is heston_restate's: its spreads of S_T and v_n are at least those of the 256 paths heston_cases takes
        assert s["S_T"] >= hc.spread(prec, name)["S_T"] and s["v_n"] >= hc.spread(prec, name)["v_n"]
        # a kept path is hit in both precisions or in neither: a flip would move a discrete weight by exactly 1
        assert s["w"] < 1.0
