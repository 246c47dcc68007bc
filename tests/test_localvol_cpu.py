"""CPU-only checks of the local-volatility entry points (include/mcamd.h, mcamd_price_localvol): declarations and
struct layout; every refusal that needs no device — the grid's through the host lookup and through
mcamd_localvol_surface_create with ctx = NULL (the grid is checked first), the pricing calls' with ctx = NULL and
surface = NULL (everything that does not need the surface is refused before the surface is looked at, the surface
before the context); the two host helpers against closed forms and the numpy restatement
(tests/localvol_restate.py); the restatement against the barrier restatement on a flat surface and against the exact
displaced-diffusion price.  No kernels run here."""
import ctypes as C
import importlib
import itertools
import math
import os
import re

import numpy as np
import pytest

import barrier_restate as br
import localvol_restate as lv

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


NAMES = ("mcamd_localvol_surface_create", "mcamd_localvol_surface_destroy", "mcamd_price_localvol",
         "mcamd_price_localvol_enqueue", "mcamd_localvol_sigma_f64", "mcamd_bs_price_f64")


# ---- declarations ----------------------------------------------------------------------------------------------------

def test_header_declares_the_calls_and_the_structs(lib):
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS and hasattr(lib, name)
    for struct in ("mcamd_localvol_grid", "mcamd_localvol"):
        assert re.search(r"\}\s*" + struct + r"\s*;", header), struct
    assert re.search(r"typedef\s+struct\s+mcamd_localvol_surface\s+mcamd_localvol_surface\s*;", header)
    assert re.search(r"#define\s+MCAMD_LOCALVOL_NO_BARRIER\s+\(-1\)", header) and capi.LOCALVOL_NO_BARRIER == -1 == lv.NO_BARRIER
    assert re.search(r"#define\s+MCAMD_LOCALVOL_MAX_NODES\s+2048\b", header) and capi.LOCALVOL_MAX_NODES == 2048
    assert re.search(r"#define\s+MCAMD_ABI_VERSION\s+5\b", header) and lib.mcamd_abi_version() == 5
    assert not re.search(r"mcamd_group_\w*localvol", header)
    # the bias of the frozen-volatility bridge is stated where the weight is defined
    assert "O(dt) bias" in header and "varies in time only" in header


def test_structs_match_the_header():
    # static_assert(sizeof(mcamd_localvol_grid) == 24 && sizeof(mcamd_localvol) == 24) in csrc/capi_localvol.cpp
    G, J = capi.LocalVolGrid, capi.LocalVol
    assert C.sizeof(G) == 24 and (G.n_t.offset, G.n_x.offset, G.x_min.offset, G.x_max.offset) == (0, 4, 8, 16)
    assert C.sizeof(J) == 24
    assert (J.payoff.offset, J.barrier.offset, J.monitoring.offset, J.reserved.offset, J.q.offset) == (0, 4, 8, 12, 16)
    j = capi.make_localvol(capi.PAYOFF_PUT, capi.BARRIER_UP_IN, capi.MONITOR_CONTINUOUS, 0.03)
    assert (j.payoff, j.barrier, j.monitoring, j.reserved, j.q) == (1, 3, 1, 0, 0.03)
    d = capi.make_localvol()
    assert (d.payoff, d.barrier, d.monitoring, d.reserved, d.q) == (0, -1, 0, 0, 0.0)
    g = capi.make_localvol_grid(4, 65, -1.5, 1.5)
    assert (g.n_t, g.n_x, g.x_min, g.x_max) == (4, 65, -1.5, 1.5)


# ---- refusals: the grid and the table ----------------------------------------------------------------------------------

def grid_refusals():
    ok = [0.2] * 6
    inf, nan = float("inf"), float("nan")
    yield "n_t 0", (0, 3, -1.0, 1.0), ok, "n_t >= 1"
    yield "n_x 0", (2, 0, -1.0, 1.0), ok, "n_x >= 2"
    yield "n_x 1", (2, 1, -1.0, 1.0), ok, "n_x >= 2"
    yield "2049 nodes", (1, 2049, -1.0, 1.0), [0.2] * 2049, "nodes"
    yield "3 x 683 nodes", (3, 683, -1.0, 1.0), [0.2] * 2049, "nodes"
    yield "2^16 x 2^16 nodes", (1 << 16, 1 << 16, -1.0, 1.0), ok, "nodes"
    yield "x_min inf", (2, 3, -inf, 1.0), ok, "x_min < x_max"
    yield "x_max inf", (2, 3, -1.0, inf), ok, "x_min < x_max"
    yield "x_min nan", (2, 3, nan, 1.0), ok, "x_min < x_max"
    yield "x_max nan", (2, 3, -1.0, nan), ok, "x_min < x_max"
    yield "x_min = x_max", (2, 3, 1.0, 1.0), ok, "x_min < x_max"
    yield "x_min > x_max", (2, 3, 1.0, -1.0), ok, "x_min < x_max"
    for bad in (0.0, -0.2, inf, nan):
        for where in (0, 5):
            t = list(ok)
            t[where] = bad
            yield f"entry {where} = {bad}", (2, 3, -1.0, 1.0), t, "finite and > 0"


def _table(values):
    return (C.c_double * len(values))(*values)


@pytest.mark.parametrize("case", list(grid_refusals()), ids=lambda c: c[0])
def test_grid_refusals_need_no_device(lib, case):
    _, grid, table, words = case
    g = capi.make_localvol_grid(*grid)
    out = C.c_double(7.0)
    assert lib.mcamd_localvol_sigma_f64(C.byref(g), _table(table), 10, 0, 0.0, C.byref(out)) == capi.ERR_INVALID
    assert words in lib.mcamd_last_error().decode() and out.value == 0.0
    h = C.c_void_p(12345)
    assert lib.mcamd_localvol_surface_create(None, C.byref(g), _table(table), C.byref(h)) == capi.ERR_INVALID
    assert words in lib.mcamd_last_error().decode() and not h.value


def test_null_pointers_and_lookup_arguments(lib):
    g, t = capi.make_localvol_grid(2, 3, -1.0, 1.0), _table([0.2] * 6)
    out, h = C.c_double(0), C.c_void_p()
    fn = lib.mcamd_localvol_sigma_f64
    assert fn(C.byref(g), t, 10, 9, 0.0, C.byref(out)) == capi.OK and out.value == pytest.approx(0.2, rel=1e-15)
    assert fn(None, t, 10, 0, 0.0, C.byref(out)) == capi.ERR_INVALID
    assert fn(C.byref(g), None, 10, 0, 0.0, C.byref(out)) == capi.ERR_INVALID
    assert fn(C.byref(g), t, 10, 0, 0.0, None) == capi.ERR_INVALID
    for n_steps, step in ((0, 0), (10, 10), (10, 11), (1, 1)):
        assert fn(C.byref(g), t, n_steps, step, 0.0, C.byref(out)) == capi.ERR_INVALID
        assert "step" in lib.mcamd_last_error().decode()
    assert fn(C.byref(g), t, 10, 0, float("nan"), C.byref(out)) == capi.ERR_INVALID
    create = lib.mcamd_localvol_surface_create
    assert create(None, None, t, C.byref(h)) == capi.ERR_INVALID
    assert create(None, C.byref(g), None, C.byref(h)) == capi.ERR_INVALID
    assert create(None, C.byref(g), t, None) == capi.ERR_INVALID
    # an acceptable grid reaches the missing context
    assert create(None, C.byref(g), t, C.byref(h)) == capi.ERR_INVALID and "ctx" in lib.mcamd_last_error().decode()
    assert lib.mcamd_localvol_surface_destroy(None) == capi.OK


# ---- refusals: the pricing calls ---------------------------------------------------------------------------------------

def price(lib, opt, sim, job, res=True):
    out = capi.Result()
    ref = lambda x: None if x is None else C.byref(x)
    rc = lib.mcamd_price_localvol(None, ref(opt), ref(sim), ref(job), None, None, C.byref(out) if res else None)
    return rc, lib.mcamd_last_error().decode()


DOWN = dict(S0=100.0, K=100.0, B=90.0, r=0.1, v=0.0, T=1.0)   # v is ignored: 0 would be refused by every other call


def job_refusals():
    O, S, J = capi.make_option, capi.make_sim, capi.make_localvol
    opt, sim, job = O(**DOWN), S(1000, 50), J()
    down = J(barrier=capi.BARRIER_DOWN_OUT)
    yield "no opt", (None, sim, job), {}, "non-NULL"
    yield "no sim", (opt, None, job), {}, "non-NULL"
    yield "no job", (opt, sim, None), {}, "non-NULL"
    yield "no res", (opt, sim, job), dict(res=False), "non-NULL"
    for p in (-1, 2):
        yield f"payoff {p}", (opt, sim, J(payoff=p)), {}, "payoff"
    for b in (-2, 4):
        yield f"barrier {b}", (opt, sim, J(barrier=b)), {}, "barrier"
    for m in (-1, 2):
        yield f"monitoring {m}", (opt, sim, J(monitoring=m)), {}, "monitoring"
        yield f"monitoring {m} with a barrier", (opt, sim, J(barrier=capi.BARRIER_DOWN_IN, monitoring=m)), {}, "monitoring"
    bad = J()
    bad.reserved = 1
    yield "reserved", (opt, sim, bad), {}, "reserved"
    for q in (float("nan"), float("inf"), -float("inf")):
        yield f"q = {q}", (opt, sim, J(q=q)), {}, "dividend yield"
    for B in (0.0, -90.0, float("nan")):
        yield f"B = {B}", (O(**dict(DOWN, B=B)), sim, down), {}, "B must be positive"
    yield "down, S0 below B", (O(**dict(DOWN, B=110.0)), sim, down), {}, "live side"
    yield "down, S0 on B", (O(**dict(DOWN, B=100.0)), sim, J(barrier=capi.BARRIER_DOWN_IN)), {}, "live side"
    yield "up, S0 above B", (opt, sim, J(barrier=capi.BARRIER_UP_OUT)), {}, "live side"
    yield "up, S0 on B", (O(**dict(DOWN, B=100.0)), sim, J(barrier=capi.BARRIER_UP_IN)), {}, "live side"
    yield "use_window", (O(**DOWN, use_window=1), sim, job), {}, "window"
    yield "P1", (O(**DOWN, P1=1), sim, job), {}, "window"
    yield "P2", (O(**DOWN, P2=3), sim, job), {}, "window"
    yield "Ik", (O(**DOWN, Ik=2), sim, job), {}, "window"
    yield "Sk", (O(**DOWN, Sk=95.0), sim, job), {}, "Sk"
    yield "Tk", (O(**DOWN, Tk=5), sim, job), {}, "Tk"
    yield "dt", (O(**DOWN, dt=0.01), sim, job), {}, "dt"
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE, capi.FLAG_PRODUCT_FORM,
                  capi.FLAG_LOG_SPACE | capi.FLAG_ANTITHETIC, 32):
        yield f"flags {flags}", (opt, S(1000, 50, flags=flags), job), {}, "flags"
    # what mcamd_price_paths refuses on sim
    yield "precision", (opt, S(1000, 50, precision=16), job), {}, "precision"
    yield "n_steps 0", (opt, S(1000, 0), job), {}, "n_steps"
    yield "shard overflow", (opt, S(1 << 63, 50, path_offset=(1 << 64) - 10, n_paths_local=100), job), {}, "overflows"
    yield "exponent range", (O(**dict(DOWN, r=1000.0, T=100.0)), S(1000, 50), job), {}, "exponent range"


@pytest.mark.parametrize("case", list(job_refusals()), ids=lambda c: c[0])
def test_refusals_before_the_surface_and_the_context_are_looked_at(lib, case):
    _, args, kw, words = case
    rc, msg = price(lib, *args, **kw)
    assert rc == capi.ERR_INVALID and words in msg, msg
    if kw.get("res", True):   # the enqueue form shares the checks
        ref = lambda x: None if x is None else C.byref(x)
        rc = lib.mcamd_price_localvol_enqueue(None, ref(args[0]), ref(args[1]), ref(args[2]), None, None, None)
        assert rc == capi.ERR_INVALID and words in lib.mcamd_last_error().decode()


@pytest.mark.parametrize("barrier", (capi.LOCALVOL_NO_BARRIER,) + br.KINDS)
@pytest.mark.parametrize("payoff", [capi.PAYOFF_CALL, capi.PAYOFF_PUT])
@pytest.mark.parametrize("monitoring", [capi.MONITOR_DISCRETE, capi.MONITOR_CONTINUOUS])
@pytest.mark.parametrize("flags,prec", [(0, capi.F64), (capi.FLAG_LOG_SPACE, capi.F32)])
def test_accepted_requests_reach_the_missing_surface(lib, barrier, payoff, monitoring, flags, prec):
    """opt->v is ignored: 0, a negative number and NaN all pass"""
    for v in (0.0, -1.0, float("nan"), 0.2):
        opt = capi.make_option(**dict(DOWN, v=v, B=110.0 if barrier in (br.UP_OUT, br.UP_IN) else 90.0))
        sim = capi.make_sim(1000, 50, prec, flags=flags, path_offset=3, n_paths_local=0)
        rc, msg = price(lib, opt, sim, capi.make_localvol(payoff, barrier, monitoring, 0.03))
        assert rc == capi.ERR_INVALID and "surface" in msg and "non-NULL" in msg, msg


def test_python_surface_table_must_match_the_grid():
    with pytest.raises(ValueError):
        capi.localvol_sigma_f64((2, 3, -1.0, 1.0), [[0.2] * 3], 10, 0, 0.0)


# ---- Black-Scholes with a dividend yield -------------------------------------------------------------------------------

BS_GRID = list(itertools.product((80.0, 100.0, 125.0), (0.25, 1.0, 3.0), ((0.1, 0.2), (0.03, 0.35), (0.0, 0.1))))


def test_bs_price_is_bs_call_without_dividends(lib):
    """the same formula: 4 ulp of the larger of the two terms it subtracts"""
    for K, T, (r, v) in BS_GRID:
        got, want = capi.bs_price_f64(100.0, K, T, r, 0.0, v), capi.bs_call_f64(100.0, K, T, r, v)
        assert abs(got - want) <= 4 * 2.2e-16 * 100.0, (K, T, r, v, got, want)


def test_bs_price_put_call_parity_with_dividends(lib):
    """call - put = S0 e^{-qT} - K e^{-rT}: terms of the size of S0 and K, each good to a few ulp of itself"""
    for K, T, (r, v) in BS_GRID:
        for q in (0.03, 0.12, -0.02):
            call = capi.bs_price_f64(100.0, K, T, r, q, v, capi.PAYOFF_CALL)
            put = capi.bs_price_f64(100.0, K, T, r, q, v, capi.PAYOFF_PUT)
            fwd = 100.0 * math.exp(-q * T) - K * math.exp(-r * T)
            assert call > 0 and put > 0 and abs(call - put - fwd) <= 1e-13 * max(100.0, K), (K, T, r, q, v)
    # a dividend yield lowers the call and lifts the put
    assert capi.bs_price_f64(100, 100, 1, 0.1, 0.03, 0.2) < capi.bs_price_f64(100, 100, 1, 0.1, 0.0, 0.2)
    assert capi.bs_price_f64(100, 100, 1, 0.1, 0.03, 0.2, 1) > capi.bs_price_f64(100, 100, 1, 0.1, 0.0, 0.2, 1)


def test_bs_price_refusals(lib):
    p = C.c_double(7.0)
    fn = lib.mcamd_bs_price_f64
    ok = (100.0, 100.0, 1.0, 0.1, 0.03, 0.2, capi.PAYOFF_CALL)
    assert fn(*ok, C.byref(p)) == capi.OK and p.value > 0
    assert fn(*ok, None) == capi.ERR_INVALID
    for i, value in ((0, 0.0), (0, -1.0), (1, 0.0), (2, 0.0), (2, -1.0), (5, 0.0), (5, -0.2), (6, 2), (6, -1),
                     (3, float("nan")), (4, float("inf")), (0, float("inf"))):
        args = list(ok)
        args[i] = value
        assert fn(*args, C.byref(p)) == capi.ERR_INVALID and p.value == 0.0, (i, value)


# ---- the host lookup against the restatement -------------------------------------------------------------------------

def skew(n_t, n_x, x_min, x_max):
    x = np.linspace(x_min, x_max, n_x)
    return np.array([(0.18 + 0.04 * j) * (1.0 + 0.5 * np.exp(-x)) / 1.5 for j in range(n_t)])


def test_lookup_at_nodes_midpoints_and_beyond_the_clamps(lib):
    """fma(f, slope, sigma_k) against the restatement's f * slope + sigma_k: two roundings against one, 2 ulp"""
    grid = (4, 65, -1.5, 1.5)
    sigma = skew(*grid)
    dx = 3.0 / 64
    for step, row in ((0, 0), (12, 0), (13, 1), (49, 3)):
        assert lv.row_of(step, 4, 50) == row
        for k in range(65):
            got = capi.localvol_sigma_f64(grid, sigma, 50, step, -1.5 + k * dx)
            assert abs(got - sigma[row, k]) <= 4.5e-16 * sigma[row, k]
            assert abs(got - lv.sigma_at(grid, sigma, 50, step, -1.5 + k * dx)) <= 4.5e-16 * got
        for k in range(64):
            x = -1.5 + (k + 0.5) * dx
            got, want = capi.localvol_sigma_f64(grid, sigma, 50, step, x), lv.sigma_at(grid, sigma, 50, step, x)
            assert abs(got - want) <= 4.5e-16 * want
            assert abs(got - 0.5 * (sigma[row, k] + sigma[row, k + 1])) <= 1e-13   # x is a mid-point to ~1e-16 only
        for x, k in ((-1.5000001, 0), (-2.0, 0), (-1e300, 0), (-float("inf"), 0), (1.5000001, 64), (7.0, 64), (1e300, 64),
                     (float("inf"), 64)):
            assert capi.localvol_sigma_f64(grid, sigma, 50, step, x) == sigma[row, k]
            assert lv.sigma_at(grid, sigma, 50, step, x) == sigma[row, k]
    # the smallest surface: one slice, two nodes
    two = (1, 2, -0.5, 0.5)
    for x, want in ((-0.5, 0.1), (0.5, 0.3), (0.0, 0.2), (-0.25, 0.15), (3.0, 0.3), (-3.0, 0.1)):
        assert capi.localvol_sigma_f64(two, [[0.1, 0.3]], 7, 6, x) == pytest.approx(want, rel=1e-15)


@pytest.mark.parametrize("n_t,n_steps", [(3, 50), (7, 5), (4, 12)])
def test_lookup_at_slice_boundaries(lib, n_t, n_steps):
    """every step of the job: the row is floor(step n_t / n_steps), also where n_t does not divide n_steps (3, 50) and
    where it exceeds it (7, 5: rows 0, 1, 2, 4, 5 — rows 3 and 6 are never used)"""
    grid = (n_t, 5, -1.0, 1.0)
    sigma = np.array([[0.1 * (j + 1) + 0.01 * k for k in range(5)] for j in range(n_t)])
    rows = [lv.row_of(i, n_t, n_steps) for i in range(n_steps)]
    assert rows == [math.floor(i * n_t / n_steps + 1e-9) for i in range(n_steps)] and rows[0] == 0 and rows[-1] <= n_t - 1
    if (n_t, n_steps) == (7, 5):
        assert rows == [0, 1, 2, 4, 5]
    if (n_t, n_steps) == (4, 12):
        assert rows == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    for i in range(n_steps):
        for x in (-1.0, -0.3, 0.0, 0.25, 1.0):
            got, want = capi.localvol_sigma_f64(grid, sigma, n_steps, i, x), lv.sigma_at(grid, sigma, n_steps, i, x)
            assert abs(got - want) <= 4.5e-16 * want, (i, x)
            assert 0.1 * (rows[i] + 1) - 1e-12 <= got <= 0.1 * (rows[i] + 1) + 0.04 + 1e-12


# ---- the restatement against the barrier restatement -------------------------------------------------------------------

@pytest.mark.parametrize("kind", br.KINDS)
@pytest.mark.parametrize("payoff", [br.CALL, br.PUT])
@pytest.mark.parametrize("monitoring", [br.DISCRETE, br.CONTINUOUS])
def test_a_flat_surface_without_dividends_is_the_barrier_restatement(kind, payoff, monitoring):
    """1e-12 relative, taken relative to the path's payoff h: both w h and (1 - w) h are formed on that scale, and a
    knock-in's 1 - w near 0 carries the rounding of w, not of itself.  The paths are walked with the same operations (a
    flat row interpolates to its value exactly); only q_i is divided out in another order."""
    S0, K, T, r, v, n_steps = 100.0, 100.0, 1.0, 0.1, 0.2, 12
    B = 110.0 if br.is_up(kind) else 92.0
    z = np.random.default_rng(31).standard_normal((n_steps, 20_000))
    want = br.samples(z, S0, K, B, T, r, v, kind, payoff, monitoring)
    for grid, sigma in (((1, 2, -1.0, 1.0), [[v, v]]), ((3, 7, -0.2, 0.1), np.full((3, 7), v))):
        got = lv.samples(z, S0, K, B, T, r, 0.0, grid, sigma, kind, payoff, monitoring)
        assert np.array_equal(got["S_T"], want["S_T"]) and np.array_equal(got["live"], want["live"])
        assert np.array_equal(got["min_abs_d"], want["min_abs_d"])
        assert (np.abs(got["y"] - want["y"]) <= 1e-12 * want["h"]).all()
        assert (got["y"] != 0).mean() > 0.02
    # and without a barrier the sample is the payoff
    eur = lv.samples(z, S0, K, B, T, r, 0.0, (1, 2, -1.0, 1.0), [[v, v]], lv.NO_BARRIER, payoff, monitoring)
    assert np.array_equal(eur["y"], want["h"]) and (eur["live"] == n_steps).all() and np.isinf(eur["min_abs_d"]).all()


def test_restatement_precisions_agree():
    """the three dtypes walk the same paths on a skewed surface"""
    grid = (4, 65, -1.5, 1.5)
    sigma = skew(*grid)
    z = np.random.default_rng(3).standard_normal((50, 5000)).astype(np.float32).astype(np.float64)
    args = (100.0, 100.0, 92.0, 1.0, 0.1, 0.03, grid, sigma)
    y64 = lv.samples(z, *args, lv.NO_BARRIER, lv.CALL, lv.DISCRETE)["y"]
    yld = lv.samples(z, *args, lv.NO_BARRIER, lv.CALL, lv.DISCRETE, np.longdouble)["y"]
    y32 = lv.samples(z, *args, lv.NO_BARRIER, lv.CALL, lv.DISCRETE, np.float32)["y"]
    assert np.abs(y64 - yld.astype(np.float64)).max() <= 1e-11 and np.abs(y64 - y32).max() <= 2e-3
    b64 = lv.samples(z, *args, lv.DOWN_OUT, lv.CALL, lv.CONTINUOUS)
    keep = b64["min_abs_d"] >= 1e-4
    b32 = lv.samples(z, *args, lv.DOWN_OUT, lv.CALL, lv.CONTINUOUS, np.float32)["y"]
    assert keep.mean() > 0.9 and np.abs(b64["y"][keep] - b32[keep]).max() <= 2e-3
    assert (b64["y"] <= y64).all() and (b64["y"] < y64).any()


# ---- displaced diffusion: a surface that varies in x, with an exact price ---------------------------------------------

DD_SEED, DD_PATHS, DD_STEPS = 20240611, 1 << 19, 64


def displaced_surface(S0=100.0, a=50.0, n_x=65, x_min=-1.5, x_max=1.5):
    """sigma(x) = sigma_d (1 + a / (S0 e^x)): S + a is then geometric Brownian motion with volatility sigma_d"""
    sigma_d = 0.2 * S0 / (S0 + a)
    x = np.linspace(x_min, x_max, n_x)
    return (1, n_x, x_min, x_max), (sigma_d * (1.0 + a / (S0 * np.exp(x))))[None, :], sigma_d


def test_restatement_prices_displaced_diffusion(lib):
    """r = q = 0, T = 1: call(K) = BS(S0 + a, K + a, sigma_d) exactly.  The float64 restatement at 64 steps on 2^19 paths
    lies within 4 SE of it for K = 80, 100 and 125 (the piecewise-linear surface on 65 nodes and the Euler step bias the
    price by far less than one SE here; at 8 steps K = 125 is some 3 SE off)."""
    S0, a = 100.0, 50.0
    grid, sigma, sigma_d = displaced_surface(S0, a)
    z = np.random.default_rng(DD_SEED).standard_normal((DD_STEPS, DD_PATHS))
    S_T = lv.samples(z, S0, 100.0, 0.0, 1.0, 0.0, 0.0, grid, sigma, lv.NO_BARRIER, lv.CALL, lv.DISCRETE)["S_T"]
    for K in (80.0, 100.0, 125.0):
        y = np.maximum(S_T - K, 0.0)
        got, se = y.mean(), y.std(ddof=1) / math.sqrt(y.size)
        want = capi.bs_price_f64(S0 + a, K + a, 1.0, 0.0, 0.0, sigma_d)
        print(f"K {K}: exact {want:.5f} restated {got:.5f} SE {se:.5f} ({(got - want) / se:+.2f} SE)")
        assert abs(got - want) <= 4.0 * se, (K, got, want, se)
