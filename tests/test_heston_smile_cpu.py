"""CPU-only checks of the Heston smile call (include/mcamd.h, mcamd_price_heston_smile).  No kernels run here.

  1. declarations; every refusal through both entry points, given no context, and their documented order (a request
     wrong at two stages is refused for the earlier one);
  2. the restatement (tests/heston_smile_restate.py): its last expiry at s = n_steps is heston_restate.samples' S_T and
     v_n bit for bit, in three dtypes; an inner expiry is bit for bit the restatement stopped there (and within rounding
     of dt the shorter job of heston_restate.samples); the three restated mistakes change it;
  3. mcamd_finalize_smile reads n_expiries and n_strikes of its mcamd_smile alone;
  4. capi.heston_smile_prices against capi.heston_price, node by node;
  5. the cross-compile's resource figures: the two new kernels and the two local-volatility smile kernels use no scratch
     and spill nothing.  Occupancy is printed, not asserted."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import heston_restate as hr
import heston_smile_restate as hs
from deep_inputs import SHALLOW

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcamd_price_heston_smile", "mcamd_price_heston_smile_enqueue")
NAN, INF = float("nan"), float("inf")
S0, T_, R, Q = hr.S0, hr.T_, hr.R, hr.Q_DIV


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


# ---- 1. declarations and refusals -------------------------------------------------------------------------------------------

def test_header_declares_the_calls(lib):
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        text = f.read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert re.search(r"#define\s+MCAMD_ABI_VERSION\s+5\b", text) and lib.mcamd_abi_version() == 5
    assert "first carried by the build that ships csrc/heston_smile.hip" in text
    assert not re.search(r"mcamd_group_\w*heston", text)
    # the smile is no longer among what the Heston call leaves out, and the finalize says what it reads
    assert "a smile call" not in text
    assert "reads only n_expiries and n_strikes" in text and "truncated_steps and mean_variance are NOT reported" in text
    build = importlib.import_module("monte-carlo-project-cuda_amd.build")
    assert "heston_smile.hip" in build.SOURCES and "smile.hip" in build.SOURCES
    assert "heston_smile.hpp" in build.HEADERS and "smile_device.hpp" in build.HEADERS and "smile.hpp" in build.HEADERS
    assert hasattr(capi.Context, "price_heston_smile") and hasattr(capi.Context, "price_heston_smile_enqueue")


BASE = dict(S0=S0, K=NAN, v=NAN, B=NAN, r=R, T=T_)   # opt->K, opt->v and opt->B are ignored: NaN passes
REF = lambda x: None if x is None else C.byref(x)


def heston(payoff=capi.PAYOFF_CALL, **kw):
    q, v0, kappa, theta, xi, rho = hr.params("F")
    return capi.make_heston(payoff, **dict(dict(q=q, v0=v0, kappa=kappa, theta=theta, xi=xi, rho=rho), **kw))


def arrays(steps, strikes):
    return (None if steps is None else (C.c_uint32 * max(len(steps), 1))(*steps),
            None if strikes is None else (C.c_double * max(len(strikes), 1))(*strikes))


def price(lib, opt, sim, model, steps, strikes, n_e=None, n_K=None, stats=True, res=True, ctx=None, d_stats=None):
    """both forms: ((rc, message) of the synchronous one, then of the enqueue one).  n_e, n_K: the counts passed, where
    they are not the lengths of the arrays.  ctx: a live context's handle; d_stats: a device address for the enqueue
    form (without a context nothing is written: any non-NULL address serves)."""
    e, k = arrays(steps, strikes)
    n_e = len(steps or ()) if n_e is None else n_e
    n_K = len(strikes or ()) if n_K is None else n_K
    h_stats, out = (C.c_double * 8192)(), capi.Result()
    rc = lib.mcamd_price_heston_smile(ctx, REF(opt), REF(sim), REF(model), n_e, n_K, e, k, None,
                                      h_stats if stats else None, C.byref(out) if res else None)
    first = (rc, lib.mcamd_last_error().decode())
    assert all(v == 0 for v in out.as_dict().values()) and not any(h_stats)
    rc = lib.mcamd_price_heston_smile_enqueue(ctx, REF(opt), REF(sim), REF(model), n_e, n_K, e, k, None,
                                              (d_stats or C.c_void_p(64)) if stats and res else None)
    return first, (rc, lib.mcamd_last_error().decode())


def refusals():
    """(stage, name, (opt, sim, heston, steps, strikes), keywords of price(), words of the message), in the documented
    order of the stages: 1 NULL pointers; 2 payoff, scheme, reserved, the model, r; 3 the counts; 4 the expiry steps;
    5 the strikes; 6 sim and the rest of opt; 7 S0; 8 the context"""
    O, S = capi.make_option, capi.make_sim
    opt, sim, model, e1, k1 = O(**BASE), S(1000, 50), heston(), [50], [100.0]
    yield 1, "no opt", (None, sim, model, e1, k1), {}, "non-NULL"
    yield 1, "no sim", (opt, None, model, e1, k1), {}, "non-NULL"
    yield 1, "no heston", (opt, sim, None, e1, k1), {}, "non-NULL"
    yield 1, "no expiry steps", (opt, sim, model, None, k1), dict(n_e=1), "non-NULL"
    yield 1, "no strikes", (opt, sim, model, e1, None), dict(n_K=1), "non-NULL"
    yield 1, "no h_stats", (opt, sim, model, e1, k1), dict(stats=False), "NULL"
    yield 1, "no res", (opt, sim, model, e1, k1), dict(res=False), "NULL"
    for payoff in (-1, 2):
        yield 2, f"payoff {payoff}", (opt, sim, heston(payoff), e1, k1), {}, "payoff"
    for scheme in (-1, 1):
        yield 2, f"scheme {scheme}", (opt, sim, heston(scheme=scheme), e1, k1), {}, "scheme"
    for value in (1.0, NAN, 5e-324):
        bad = heston()
        bad.reserved = value
        yield 2, f"reserved {value}", (opt, sim, bad, e1, k1), {}, "reserved"
    for field in ("q", "v0", "kappa", "theta", "xi", "rho"):
        for value in (NAN, INF, -INF):
            yield 2, f"{field} = {value}", (opt, sim, heston(**{field: value}), e1, k1), {}, "must be finite"
    for field in ("v0", "kappa", "theta", "xi"):
        yield 2, f"{field} < 0", (opt, sim, heston(**{field: -1e-300}), e1, k1), {}, ">= 0"
    for rho in (1.0000000000000002, -1.5):
        yield 2, f"rho = {rho}", (opt, sim, heston(rho=rho), e1, k1), {}, "rho"
    for r in (NAN, INF):
        yield 2, f"r = {r}", (O(**dict(BASE, r=r)), sim, model, e1, k1), {}, "finite"
    yield 3, "0 expiries", (opt, sim, model, [], k1), {}, "n_expiries"
    yield 3, "33 expiries", (opt, sim, model, list(range(1, 34)), k1), {}, "n_expiries"
    yield 3, "0 strikes", (opt, sim, model, e1, []), {}, "n_strikes"
    yield 3, "65 strikes", (opt, sim, model, e1, [100.0] * 65), {}, "n_strikes"
    yield 4, "expiries descend", (opt, sim, model, [10, 30, 20], k1), {}, "strictly ascending"
    yield 4, "expiry repeated", (opt, sim, model, [10, 20, 20], k1), {}, "strictly ascending"
    yield 4, "expiry 0", (opt, sim, model, [0, 20], k1), {}, "strictly ascending"
    yield 4, "expiry beyond n_steps", (opt, sim, model, [20, 51], k1), {}, "strictly ascending"
    yield 4, "first expiry beyond n_steps", (opt, sim, model, [51], k1), {}, "strictly ascending"
    for K in (NAN, INF, -100.0, 0.0):
        yield 5, f"strike {K}", (opt, sim, model, e1, [90.0, 100.0, K]), {}, "strike"
    yield 6, "use_window", (O(**BASE, use_window=1), sim, model, e1, k1), {}, "window"
    yield 6, "P1", (O(**BASE, P1=1), sim, model, e1, k1), {}, "window"
    yield 6, "P2", (O(**BASE, P2=3), sim, model, e1, k1), {}, "window"
    yield 6, "Ik", (O(**BASE, Ik=2), sim, model, e1, k1), {}, "window"
    yield 6, "Sk", (O(**BASE, Sk=95.0), sim, model, e1, k1), {}, "Sk"
    yield 6, "Tk", (O(**BASE, Tk=5), sim, model, e1, k1), {}, "Tk"
    yield 6, "dt", (O(**BASE, dt=0.01), sim, model, e1, k1), {}, "dt"
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE, capi.FLAG_PRODUCT_FORM,
                  capi.FLAG_LOG_SPACE | capi.FLAG_ANTITHETIC, 32):
        yield 6, f"flags {flags}", (opt, S(1000, 50, flags=flags), model, e1, k1), {}, "flags"
    yield 6, "precision", (opt, S(1000, 50, precision=16), model, e1, k1), {}, "precision"
    yield 6, "shard overflow", (opt, S(1 << 63, 50, path_offset=(1 << 64) - 10, n_paths_local=100), model, e1, k1), {}, \
        "overflows"
    yield 6, "exponent range", (O(**dict(BASE, T=100.0)), sim, heston(q=-1e4), e1, k1), {}, "exponent range"
    yield 6, "T = 0", (O(**dict(BASE, T=0.0)), sim, model, e1, k1), {}, "T > 0"
    yield 6, "T = inf", (O(**dict(BASE, T=INF)), sim, model, e1, k1), {}, "finite"
    yield 6, "S0 = nan", (O(**dict(BASE, S0=NAN)), sim, model, e1, k1), {}, "finite"
    for value in (0.0, -1.0):
        yield 7, f"S0 = {value}", (O(**dict(BASE, S0=value)), sim, model, e1, k1), {}, "S0 > 0"
    yield 8, "no context", (opt, sim, model, e1, k1), {}, "ctx is NULL"


@pytest.mark.parametrize("case", list(refusals()), ids=lambda c: c[1])
def test_refusals_before_the_context_is_looked_at(lib, case):
    """Every case but the last is wrong in one way only and is given no context: the message names the request's fault,
    so the refusal came before the context."""
    _, _, args, kw, words = case
    for rc, msg in price(lib, *args, **kw):
        assert rc == capi.ERR_INVALID and words in msg, msg


def test_n_steps_zero_is_refused_with_the_expiry_steps(lib):
    """no expiry step lies in 1 .. 0, so stage 4 speaks before sim's own n_steps refusal can"""
    for rc, msg in price(lib, capi.make_option(**BASE), capi.make_sim(1000, 0), heston(), [1], [100.0]):
        assert rc == capi.ERR_INVALID and "strictly ascending" in msg, msg


def test_refusals_come_in_the_documented_order(lib):
    """a request wrong at two stages is refused for the earlier one: one fault per stage 2 .. 7, every pair of them"""
    O, S = capi.make_option, capi.make_sim
    faults = {2: dict(model=heston(xi=-1.0)), 3: dict(strikes=[100.0] * 65), 4: dict(steps=[7, 7]),
              5: dict(strikes=[100.0, -1.0]), 6: dict(sim=S(1000, 50, flags=capi.FLAG_ANTITHETIC)), 7: dict(S0=0.0)}
    words = {2: ">= 0", 3: "n_strikes", 4: "strictly ascending", 5: "strike", 6: "flags", 7: "S0 > 0"}
    n_pairs = 0
    for a in faults:
        for b in faults:
            if b <= a or (a, b) == (3, 5):   # 3 and 5 both speak through the strikes array
                continue
            req = dict(model=heston(), steps=[50], strikes=[100.0], sim=S(1000, 50), S0=S0)
            req.update(faults[a])
            req.update({k: v for k, v in faults[b].items() if k not in faults[a]})
            assert all(k in req and (req[k] is faults[b][k]) for k in faults[b]), (a, b)
            opt = O(**dict(BASE, S0=req["S0"]))
            for rc, msg in price(lib, opt, req["sim"], req["model"], req["steps"], req["strikes"]):
                assert rc == capi.ERR_INVALID and words[a] in msg, (a, b, msg)
            n_pairs += 1
    assert n_pairs == 14
    # a NULL pointer goes before everything, the context after everything
    for rc, msg in price(lib, None, S(1000, 50), heston(xi=-1.0), [7, 7], [-1.0]):
        assert "non-NULL" in msg
    for rc, msg in price(lib, O(**dict(BASE, S0=0.0)), S(1000, 50), heston(), [50], [100.0]):
        assert "S0 > 0" in msg and "ctx" not in msg


@pytest.mark.parametrize("payoff", [capi.PAYOFF_CALL, capi.PAYOFF_PUT])
@pytest.mark.parametrize("flags,prec", [(0, capi.F64), (capi.FLAG_LOG_SPACE, capi.F32)])
@pytest.mark.parametrize("steps,strikes", [([50], [100.0]), ([1, 2, 49], [1e-3, 100.0, 1e6]),
                                           (list(range(1, 33)), [50.0 + k for k in range(64)])])
def test_accepted_requests_reach_the_context(lib, payoff, flags, prec, steps, strikes):
    """everything the request alone decides has passed when the missing context is named; opt->K, opt->v and opt->B are
    ignored"""
    for K, v, B in ((0.0, 0.0, 0.0), (-5.0, -1.0, INF), (NAN, NAN, NAN)):
        opt = capi.make_option(**dict(BASE, K=K, v=v, B=B))
        sim = capi.make_sim(1000, 50, prec, flags=flags, path_offset=3, n_paths_local=0)
        for kw in (dict(), dict(xi=0.0, kappa=0.0), dict(rho=1.0), dict(v0=0.0, theta=0.0)):
            for rc, msg in price(lib, opt, sim, heston(payoff, **kw), steps, strikes):
                assert rc == capi.ERR_INVALID and "ctx is NULL" in msg, msg


# ---- 2. the restatement -----------------------------------------------------------------------------------------------------

DTYPES = [np.float32, np.float64, np.longdouble]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", ["F", "N", "H"])
@pytest.mark.parametrize("n_steps", [50, 7, 1])
def test_last_expiry_at_n_steps_is_the_heston_restatement(name, n_steps, dtype):
    prec = 32 if dtype == np.float32 else 64
    z, zv = hr.draws(prec, SHALLOW[0], SHALLOW[1], 96, n_steps)
    p = hr.params(name)
    steps = sorted({1, (n_steps + 1) // 2, n_steps})
    S, v = hs.states(z, zv, S0, T_, R, p, n_steps, steps, dtype)
    want = hr.samples(z, zv, S0, 100.0, T_, R, p, hr.CALL, dtype)
    assert S.dtype == v.dtype == np.dtype(dtype) and S.shape == v.shape == (len(steps), 96)
    assert np.array_equal(S[-1], want["S_T"]) and np.array_equal(v[-1], want["v_n"])
    if name == "H" and n_steps == 50:
        assert (v < 0).any()   # the raw variance is recorded, not v+


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_inner_expiries_are_the_restatement_stopped_there(dtype):
    prec = 32 if dtype == np.float32 else 64
    n_steps, steps = 12, (1, 5, 6, 11)
    z, zv = hr.draws(prec, SHALLOW[0], SHALLOW[1], 96, n_steps)
    p = hr.params("N")
    S, v = hs.states(z, zv, S0, T_, R, p, n_steps, steps, dtype)
    for m, s in enumerate(steps):
        # stopped there: the same job (dt from the whole n_steps) with that expiry alone, fed no later normal
        S_m, v_m = hs.states(z[:s], zv[:s], S0, T_, R, p, n_steps, (s,), dtype)
        assert np.array_equal(S_m[0], S[m]) and np.array_equal(v_m[0], v[m])
        # the shorter job of the Heston restatement takes dt = (T s / n) / s with T s / n rounded to a double, which may
        # differ from T / n in the last bit of a double
        short = hr.samples(z[:s], zv[:s], S0, 100.0, T_ * s / n_steps, R, p, hr.CALL, dtype)
        eps = max(float(np.finfo(dtype).eps), float(np.finfo(np.float64).eps))
        assert np.abs(short["S_T"] - S[m]).max() <= 64 * s * eps * S0
        assert np.abs(short["v_n"] - v[m]).max() <= 64 * s * eps
    assert not np.array_equal(S[1], S[2])


def test_restated_mistakes_change_the_restatement():
    n_steps, steps = 12, (3, 12)
    z, zv = hr.draws(64, SHALLOW[0], SHALLOW[1], 96, n_steps)
    S, v = hs.states(z, zv, S0, T_, R, hr.params("H"), n_steps, steps)
    late = hs.states(z, zv, S0, T_, R, hr.params("H"), n_steps, steps, mutate=hs.LATE_EXPIRY)
    assert (late[0][0] != S[0]).all() and np.array_equal(late[0][1], S[1])   # the last expiry has no later step
    same = hs.states(z, zv, S0, T_, R, hr.params("H"), n_steps, steps, mutate=hs.SAME_BLOCKS)
    assert (same[1] != v).all() and (same[0][1] != S[1]).mean() > 0.5   # H: often both variances are below zero
    plus = hs.states(z, zv, S0, T_, R, hr.params("H"), n_steps, steps, mutate=hs.V_PLUS)
    assert np.array_equal(plus[0], S) and np.array_equal(plus[1], np.maximum(v, 0.0)) and (v < 0).any()


# ---- 3. mcamd_finalize_smile ------------------------------------------------------------------------------------------------

def test_finalize_reads_the_counts_of_its_smile_alone(lib):
    import localvol_smile_restate as sm
    n_e, n_K, n, n_steps, steps = 3, 5, 77_777, 128, [32, 64, 128]
    rng = np.random.default_rng(11)
    mean, std = rng.uniform(0.0, 30.0, n_e * n_K), rng.uniform(0.5, 20.0, n_e * n_K)
    stats = np.concatenate([n * mean, n * (mean * mean) + (n - 1) * std * std])
    opt = capi.make_option(**BASE)
    plain = capi.finalize_smile(stats, n, opt, n_steps, capi.make_smile(n_e, n_K), steps)
    odd = capi.Smile(-7, n_e, n_K, 99, NAN)   # payoff, reserved and q of no meaning: from n_e and n_K alone
    other = capi.finalize_smile(stats, n, opt, n_steps, odd, steps)
    assert np.array_equal(plain[0], other[0]) and np.array_equal(plain[1], other[1])
    want_price, want_se = sm.finalize(stats, n, R, T_, n_steps, steps, n_K)
    assert np.allclose(other[0], want_price, rtol=1e-14, atol=0) and np.allclose(other[1], want_se, rtol=1e-9, atol=0)


# ---- 4. the closed-form grid ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("payoff", [capi.PAYOFF_CALL, capi.PAYOFF_PUT])
@pytest.mark.parametrize("name", ["F", "N", "H"])
def test_closed_form_grid_is_the_closed_form_at_every_node(lib, name, payoff):
    q, v0, kappa, theta, xi, rho = hr.params(name)
    strikes, times = [80.0, 90.0, 100.0, 110.0, 120.0], [0.25, 0.5, 0.75, 1.0]
    grid = capi.heston_smile_prices(S0, strikes, times, R, q, v0, kappa, theta, xi, rho, payoff)
    assert grid.shape == (4, 5) and grid.dtype == np.float64
    for m, t in enumerate(times):
        for k, K in enumerate(strikes):
            assert grid[m, k] == capi.heston_price(S0, K, t, R, q, v0, kappa, theta, xi, rho, payoff)
    # calls fall and puts rise with the strike; both grow with the expiry at the money
    d = np.diff(grid, axis=1)
    assert (d < 0).all() if payoff == capi.PAYOFF_CALL else (d > 0).all()
    assert (np.diff(grid[:, 2]) > 0).all()
    assert capi.heston_smile_prices(S0, strikes, times, R, q, v0, kappa, theta, xi, rho)[1, 1] == \
        capi.heston_price(S0, 90.0, 0.5, R, q, v0, kappa, theta, xi, rho, capi.PAYOFF_CALL)
    with pytest.raises(capi.McamdError):
        capi.heston_smile_prices(S0, strikes, [0.5, 0.0], R, q, v0, kappa, theta, xi, rho, payoff)


# ---- 5. resources -------------------------------------------------------------------------------------------------------------

def isa_tool():
    from importlib import util as ilu
    spec = ilu.spec_from_file_location("isa_diff_for_heston_smile", os.path.join(ROOT, "tools", "isa_diff.py"))
    isa = ilu.module_from_spec(spec)
    spec.loader.exec_module(isa)
    return isa


def waves_per_simd(fig):
    """gfx950: 512 VGPRs per SIMD lane in units of 8, at most 8 wavefronts; 160 KiB of LDS per CU, 4 SIMDs, workgroups of
    4 wavefronts"""
    by_vgpr = 512 // (-(-max(fig["vgpr"], 1) // 8) * 8)
    by_lds = (160 * 1024) // fig["lds"] if fig["lds"] else 8   # workgroups per CU = wavefronts per SIMD at 4 per group
    return min(8, by_vgpr, by_lds)


def test_the_two_kernels_use_no_scratch():
    """the cross-compile alone: heston_smile_kernel<T> for two precisions, no private segment, no spilled register"""
    kernels = isa_tool().kernels_of(ROOT, "heston_smile.hip")
    assert sorted(re.search(r"heston_smile_kernelI([fd])E", k).group(1) for k in kernels) == ["d", "f"], sorted(kernels)
    for k, (ops, fig) in kernels.items():
        print(k, fig, "waves/SIMD", waves_per_simd(fig))
        assert fig["scratch"] == 0 and fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0 and fig["agpr"] == 0, (k, fig)
        # the strike phase reads its spots by v_readlane and the record through global memory
        assert ops["v_readlane_b32"] >= 1 and any(op.startswith("global_store") for op in ops), (k, dict(ops))


def test_the_localvol_smile_kernels_still_use_no_scratch():
    isa = isa_tool()
    kernels = isa.kernels_of(ROOT, "localvol_smile.hip")
    walks = [k for k in kernels if "smile_kernelI" in k]
    assert len(walks) == 2 and len(kernels) == 2, sorted(kernels)
    finish = isa.kernels_of(ROOT, "smile.hip")
    assert len(finish) == 1 and all("smile_finish_kernel" in k for k in finish), sorted(finish)
    kernels.update(finish)
    for k, (ops, fig) in kernels.items():
        print(k, fig, "waves/SIMD", waves_per_simd(fig))
        assert fig["scratch"] == 0 and fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0, (k, fig)
