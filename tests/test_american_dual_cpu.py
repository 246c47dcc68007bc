"""CPU-only checks of the dual-bound entry points (include/mcamd.h, mcamd_american_upper_bound): declarations and struct
layout, the workspace-size formula, every refusal that depends on the request alone — each happens before the
context is looked at, so ctx = NULL reaches them — and the numpy restatement against itself.  No kernels run here."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import american_dual_restate as adr
import american_restate as ar

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


def test_header_declares_the_calls_and_structs(lib):
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        header = f.read()
    for name in ("mcamd_american_dual_workspace_bytes", "mcamd_american_upper_bound"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS and hasattr(lib, name)
    for name in ("mcamd_american_dual", "mcamd_american_dual_result"):
        assert re.search(r"\}\s*" + name + r"\s*;", header), name
    assert re.search(r"#define\s+MCAMD_ABI_VERSION\s+5\b", header) and lib.mcamd_abi_version() == 5


def test_structs_match_the_header(lib):
    # static_assert(sizeof(mcamd_american_dual) == 16 && sizeof(mcamd_american_dual_result) == 104) in csrc/capi_american.cpp
    D, R = capi.AmericanDual, capi.AmericanDualResult
    assert C.sizeof(D) == 16 and C.sizeof(R) == 104
    assert (D.n_inner.offset, D.reserved.offset, D.inner_seed.offset) == (0, 4, 8)
    assert (R.upper.offset, R.std_err.offset, R.ci_hi.offset, R.sum.offset, R.sumsq.offset, R.n.offset) == \
        (0, 8, 16, 24, 32, 40)
    assert (R.sum_q0.offset, R.work_steps.offset, R.live_steps.offset, R.n_dates.offset,
            R.immediate_exercise.offset) == (48, 56, 64, 72, 76)
    assert (R.outer_ms.offset, R.inner_ms.offset, R.scan_ms.offset, R.total_ms.offset, R.grid.offset,
            R.block.offset) == (80, 84, 88, 92, 96, 100)


@pytest.mark.parametrize("n_local,n_steps,k,prec", [
    (1, 1, 1, capi.F64), (7, 3, 3, capi.F32), (4096, 50, 1, capi.F64), (4096, 50, 1, capi.F32), (100, 250, 5, capi.F64),
    (1_000_001, 252, 252, capi.F32), (3_000_001, 12, 3, capi.F64),
    (1 << 31, 4, 2, capi.F32),   # beyond 2^20 store workgroups and the 8192-workgroup caps
    (0, 50, 1, capi.F64),        # an empty shard still has a size: the table and one record of every kernel
])
def test_workspace_bytes_formula(lib, n_local, n_steps, k, prec):
    am = capi.make_american(exercise_every=k, n_train=0)   # n_train plays no part
    dual = capi.make_american_dual(n_inner=100)
    sim = capi.make_sim(n_local + 17, n_steps, prec, path_offset=5, n_paths_local=n_local)
    got = capi.american_dual_workspace_bytes(am, sim, dual)
    assert got == adr.workspace_formula(n_local, n_steps, k, prec)
    # the size depends on the shard and the dates, not on the inner sample or the basis
    assert got == capi.american_dual_workspace_bytes(capi.make_american(exercise_every=k, n_basis=4, n_train=9), sim,
                                                     capi.make_american_dual(n_inner=7, inner_seed=1))


PUT = dict(S0=36.0, K=40.0, r=0.06, v=0.2, T=1.0)
SHORT_BY_ONE = object()   # resolved inside the test (see tests/test_american_cpu.py)


def rule(M, nb=3, flag=1.0):
    t = np.zeros((M, nb + 1))
    t[:, :nb] = [0.1, -0.5, 1.0, 0.3][:nb]
    t[:, nb] = flag
    t[M - 1, :nb] = np.nan
    t[M - 1, nb] = 0.0
    return t


def bound(lib, opt, sim, am, dual, coeffs, work=C.c_void_p(1 << 20), work_bytes=1 << 60, res=True, ctx=None):
    out = capi.AmericanDualResult()
    ref = lambda x: None if x is None else C.byref(x)
    table = None if coeffs is None else np.ascontiguousarray(coeffs, dtype=np.float64)
    rc = lib.mcamd_american_upper_bound(ctx, ref(opt), ref(sim), ref(am), ref(dual),
                                        None if table is None else table.ctypes.data_as(C.POINTER(C.c_double)), work,
                                        work_bytes, None, C.byref(out) if res else None)
    return rc, lib.mcamd_last_error().decode()


def refusals():
    opt, sim, am = capi.make_option(**PUT), capi.make_sim(1000, 50), capi.make_american(n_train=0)
    dual, tab = capi.make_american_dual(), rule(50)
    A, D = capi.make_american, capi.make_american_dual
    yield "no opt", (None, sim, am, dual, tab), {}, "non-NULL"
    yield "no sim", (opt, None, am, dual, tab), {}, "non-NULL"
    yield "no am", (opt, sim, None, dual, tab), {}, "non-NULL"
    yield "no dual", (opt, sim, am, None, tab), {}, "non-NULL"
    yield "no res", (opt, sim, am, dual, tab), dict(res=False), "non-NULL"
    for p in (2, -1):
        yield f"payoff {p}", (opt, sim, A(payoff=p), dual, tab), {}, "payoff"
    for nb in (1, 5, 7):
        yield f"n_basis {nb}", (opt, sim, A(n_basis=nb), dual, tab), {}, "n_basis"
    yield "k = 0", (opt, sim, A(exercise_every=0), dual, tab), {}, "exercise_every"
    yield "k does not divide", (opt, sim, A(exercise_every=3), dual, tab), {}, "exercise_every"
    bad = A()
    bad.reserved = 1
    yield "am reserved", (opt, sim, bad, dual, tab), {}, "reserved"
    yield "M > 4096", (opt, capi.make_sim(1000, 4097), am, dual, rule(4097)), {}, "4096"
    yield "precision", (opt, capi.make_sim(1000, 50, precision=16), am, dual, tab), {}, "precision"
    yield "window", (capi.make_option(**PUT, B=30.0, P1=0, P2=10, use_window=1), sim, am, dual, tab), {}, "window"
    yield "Tk", (capi.make_option(**PUT, Tk=5), sim, am, dual, tab), {}, "Tk"
    yield "Sk", (capi.make_option(**PUT, Sk=37.0), sim, am, dual, tab), {}, "Sk"
    yield "dt", (capi.make_option(**PUT, dt=0.01), sim, am, dual, tab), {}, "dt"
    yield "v = 0", (capi.make_option(**dict(PUT, v=0.0)), sim, am, dual, tab), {}, "v > 0"
    yield "v < 0", (capi.make_option(**dict(PUT, v=-0.2)), sim, am, dual, tab), {}, "v > 0"
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE,
                  capi.FLAG_LOG_SPACE | capi.FLAG_PRODUCT_FORM, capi.FLAG_LOG_SPACE | capi.FLAG_ANTITHETIC):
        yield f"flags {flags}", (opt, capi.make_sim(1000, 50, flags=flags), am, dual, tab), {}, "flags"
    yield "no d_work", (opt, sim, am, dual, tab), dict(work=None), "d_work"
    yield "work_bytes short by one", (opt, sim, am, dual, tab), dict(work_bytes=SHORT_BY_ONE), "work_bytes"
    # the refusals of this call alone
    yield "n_inner 0", (opt, sim, am, D(n_inner=0), tab), {}, "n_inner"
    bad = D()
    bad.reserved = 7
    yield "dual reserved", (opt, sim, am, bad, tab), {}, "reserved"
    yield "no h_coeffs", (opt, sim, am, dual, None), {}, "h_coeffs"
    for flag in (2.0, 0.5, -1.0, float("nan")):
        t = rule(50)
        t[17, -1] = flag
        yield f"flag {flag}", (opt, sim, am, dual, t), {}, "flag"
    for value in (float("nan"), float("inf")):
        t = rule(50)
        t[3, 1] = value
        yield f"regressed row with {value}", (opt, sim, am, dual, t), {}, "finite"
    # (path_offset + n_paths_local) M n_inner must fit the 64-bit subsequence
    yield "subsequence overflow", (opt, capi.make_sim(1 << 62, 50, path_offset=(1 << 62) - 1000, n_paths_local=1000),
                                   am, D(n_inner=1 << 20), tab), {}, "subsequence"
    yield "subsequence overflow by the dates", (opt, capi.make_sim(1 << 50, 4000, path_offset=1 << 49,
                                                                   n_paths_local=1000),
                                                am, D(n_inner=1 << 6), rule(4000)), {}, "subsequence"


@pytest.mark.parametrize("case", list(refusals()), ids=lambda c: c[0])
def test_refusals_before_any_device_work(lib, case):
    _, args, kw, words = case
    if kw.get("work_bytes") is SHORT_BY_ONE:
        kw = dict(kw, work_bytes=capi.american_dual_workspace_bytes(args[2], args[1], args[3]) - 1)
    rc, msg = bound(lib, *args, **kw)
    assert rc == capi.ERR_INVALID and words in msg, msg


def test_workspace_query_refusals(lib):
    sim, am, dual = capi.make_sim(1000, 50), capi.make_american(), capi.make_american_dual()
    b = C.c_uint64(7)
    fn = lib.mcamd_american_dual_workspace_bytes
    assert fn(None, C.byref(sim), C.byref(dual), C.byref(b)) == capi.ERR_INVALID
    assert fn(C.byref(am), None, C.byref(dual), C.byref(b)) == capi.ERR_INVALID
    assert fn(C.byref(am), C.byref(sim), None, C.byref(b)) == capi.ERR_INVALID
    assert fn(C.byref(am), C.byref(sim), C.byref(dual), None) == capi.ERR_INVALID
    for bad_am, bad_dual, words in ((capi.make_american(payoff=3), dual, "payoff"),
                                    (capi.make_american(exercise_every=7), dual, "exercise_every"),
                                    (am, capi.make_american_dual(n_inner=0), "n_inner")):
        assert fn(C.byref(bad_am), C.byref(sim), C.byref(bad_dual), C.byref(b)) == capi.ERR_INVALID
        assert words in lib.mcamd_last_error().decode() and b.value == 0


@pytest.mark.parametrize("payoff", [capi.PAYOFF_CALL, capi.PAYOFF_PUT])
@pytest.mark.parametrize("flags", [0, capi.FLAG_LOG_SPACE, capi.FLAG_PRODUCT_FORM])
@pytest.mark.parametrize("n_basis,k,n_steps", [(0, 1, 50), (2, 5, 250), (3, 50, 50), (4, 1, 4096), (4, 2, 8192)])
def test_accepted_requests_reach_the_missing_context(lib, payoff, flags, n_basis, k, n_steps):
    opt = capi.make_option(**PUT)
    sim = capi.make_sim(1000, n_steps, capi.F32 if k % 2 else capi.F64, flags=flags, path_offset=3, n_paths_local=0)
    am = capi.make_american(payoff=payoff, exercise_every=k, n_basis=n_basis, n_train=0)
    dual = capi.make_american_dual(n_inner=1)
    need = capi.american_dual_workspace_bytes(am, sim, dual)
    M, nb = n_steps // k, n_basis or 3
    for table in (rule(M, nb), rule(M, nb, flag=0.0)):
        table = table.copy()
        table[table[:, -1] == 0, :-1] = np.nan   # rows without a rule may hold anything
        rc, msg = bound(lib, opt, sim, am, dual, table, work_bytes=need)
        assert rc == capi.ERR_INVALID and "ctx" in msg, msg


# ---- the restatement against itself ----------------------------------------------------------------------------------

def gbm_rows(rng, S0, r, v, T, n_steps, n):
    dt = T / n_steps
    z = rng.standard_normal((n_steps, n))
    return S0 * np.exp(np.cumsum((r - 0.5 * v * v) * dt + v * math.sqrt(dt) * z, axis=0))


def test_scan_with_one_date_returns_q0():
    """One date, never exercise early, exact conditional expectations: pi_1 = Z_1 - Q_0, so u_p = Q_{p,0} exactly"""
    K, r, v, T, n_steps = 40.0, 0.06, 0.2, 1.0, 10
    rows = gbm_rows(np.random.default_rng(1), 40.0, r, v, T, n_steps, 1000)
    M, t, disc = ar.dates(T, r, n_steps, n_steps)
    assert M == 1
    Q = np.full((1, 1000), float(adr.bs_put(40.0, K, r, v, T)))
    u = adr.scan(rows, Q, K, True, n_steps, disc, np.full((1, 3), np.nan), np.array([False]))
    assert np.array_equal(u, Q[0])


def test_scan_with_exact_european_values_of_a_never_exercise_rule():
    """Never exercise early, Q the exact European values: pi_j = Q_j - Q_0 and u_p = Q_0 + max(0, max_j (Z_j - Q_j))"""
    K, r, v, T, n_steps, k = 40.0, 0.06, 0.2, 1.0, 20, 2
    rows = gbm_rows(np.random.default_rng(2), 36.0, r, v, T, n_steps, 2000)
    M, t, disc = ar.dates(T, r, n_steps, k)
    Q = np.empty((M, 2000))
    Q[0] = adr.bs_put(36.0, K, r, v, T)
    for j in range(1, M):
        Q[j] = disc[j - 1] * adr.bs_put(rows[j * k - 1], K, r, v, T - t[j - 1])
    u = adr.scan(rows, Q, K, True, k, disc, np.full((M, 3), np.nan), np.zeros(M, dtype=bool))
    Z = disc[:, None] * ar.payoff(rows[k - 1::k], K, True)
    want = Q[0] + np.maximum(0.0, (Z[:-1] - Q[1:]).max(axis=0))
    assert np.allclose(u, want, rtol=0, atol=1e-12) and (u >= Q[0] - 1e-12).all() and (u > Q[0] + 0.1).any()
    # an upper bound of the Bermudan price: the European rule's bound lies above the tree
    tree = ar.crr_bermudan(36.0, K, r, v, T, M, per_date=50)
    assert u.mean() - 4 * u.std(ddof=1) / math.sqrt(u.size) > tree > Q[0, 0]


def test_follow_applies_the_rule_from_a_mid_date():
    K, k, n_steps = 40.0, 2, 12
    M, t, disc = ar.dates(1.0, 0.06, n_steps, k)
    beta = np.tile([2.0, 0.0, 0.0], (M, 1))          # continuation value 2 at every date: stop where d h(S) > 2
    flags = np.array([True, False, True, True, True, False])
    rows = np.full(((M - 1) * k, 3), 39.0)           # three paths from date 1 on: h = 1 until told otherwise
    rows[1 * k - 1, 0] = 30.0                        # date 2 is not regressed: path 0 walks past
    rows[2 * k - 1:, 0] = 35.0                       # ... and stops at date 3
    rows[4 * k - 1, 1] = 20.0                        # path 1 stops at date 5
    y, stop = adr.follow(rows, 1, K, True, k, disc, beta, flags)
    assert list(stop) == [3, 5, 6]
    assert np.allclose(y, [disc[2] * 5.0, disc[4] * 20.0, disc[5] * 1.0], rtol=1e-15)


def test_close_decisions_go_through_decide():
    beta = [0.3, -0.7, 0.4]
    S = np.linspace(30.0, 39.9, 200)
    disc = 0.97
    c = np.array([ar.continuation(beta, s / 40.0 - 1.0) for s in S])
    # the discount that puts each price exactly on its boundary, then one ulp either side
    for s, cv in zip(S, c):
        d0 = cv / (40.0 - s)
        for d in (np.nextafter(d0, 0.0), d0, np.nextafter(d0, 1.0)):
            assert adr.decide_vec(beta, d, 40.0, True, np.array([s]))[0] == ar.decide(beta, d, 40.0, True, s)[0]
    assert adr.decide_vec(beta, disc, 40.0, True, S).tolist() == [ar.decide(beta, disc, 40.0, True, s)[0] for s in S]
