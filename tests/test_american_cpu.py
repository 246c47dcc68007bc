"""CPU-only checks of the American / Bermudan entry points (include/mcamd.h, mcamd_price_american): struct layout, the
workspace-size formula, and every refusal that depends on the request alone — each happens before the context is
looked at, so ctx = NULL reaches them.  No kernels are launched here."""
import ctypes as C
import importlib
import os

import pytest

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


def test_american_structs_match_the_header(lib):
    # static_assert(sizeof(mcamd_american) == 32 && sizeof(mcamd_american_result) == 152) in csrc/capi_american.cpp
    A, R = capi.American, capi.AmericanResult
    assert C.sizeof(A) == 32 and C.sizeof(R) == 152
    assert (A.exercise_every.offset, A.n_basis.offset, A.reserved.offset, A.n_train.offset, A.train_seed.offset) == \
        (4, 8, 12, 16, 24)
    assert (R.sum.offset, R.n.offset, R.in_sample_price.offset, R.in_sample_sum.offset, R.n_train.offset) == \
        (32, 48, 56, 72, 88)
    assert (R.n_early.offset, R.sum_t_exercise.offset, R.n_dates.offset, R.n_regressed.offset) == (96, 104, 112, 116)
    assert (R.immediate_exercise.offset, R.train_ms.offset, R.total_ms.offset, R.grid.offset, R.train_grid.offset,
            R.reserved.offset) == (120, 124, 132, 136, 144, 148)


def align(x):
    return (x + 255) // 256 * 256


def workspace_formula(n_train, n_steps, k, prec):
    """include/mcamd.h, mcamd_american_workspace_bytes, restated"""
    M = n_steps // k
    elem = 4 if prec == capi.F32 else 8
    per_thread = 4 if prec == capi.F32 else 2
    groups = -(-n_train // per_thread)
    g_store = min(max(-(-groups // 256), 1), 1 << 20)
    g_sweep = min(-(-n_train // 256), 8192)
    return (256 + align(n_steps * n_train * elem) + align(8 * n_train) + align(8 * (8 * (M + 1) + 32))
            + align(8 * max(2 * g_store, 12 * g_sweep)))


@pytest.mark.parametrize("n_train,n_steps,k,prec", [
    (1, 1, 1, capi.F64), (7, 3, 3, capi.F32), (1000, 50, 1, capi.F64), (200_000, 50, 1, capi.F32),
    (1_000_000, 250, 5, capi.F64), (1_000_001, 252, 1, capi.F32), (3_000_001, 252, 252, capi.F64),
    (1 << 31, 4, 2, capi.F32),   # beyond 2^20 store workgroups and 8192 sweep workgroups: both caps
])
def test_workspace_bytes_formula(lib, n_train, n_steps, k, prec):
    am = capi.make_american(exercise_every=k, n_train=n_train)
    got = capi.american_workspace_bytes(am, capi.make_sim(10, n_steps, prec))
    assert got == workspace_formula(n_train, n_steps, k, prec)
    # the size depends on the training set and the dates, not on the pricing shard
    assert got == capi.american_workspace_bytes(am, capi.make_sim(10**9, n_steps, prec, path_offset=5,
                                                                  n_paths_local=0))


def price(lib, opt, sim, am, work=C.c_void_p(1 << 20), work_bytes=1 << 60, coeffs=None, res=True, ctx=None):
    out = capi.AmericanResult()
    rc = lib.mcamd_price_american(ctx, None if opt is None else C.byref(opt), None if sim is None else C.byref(sim),
                                  None if am is None else C.byref(am), work, work_bytes, coeffs,
                                  C.byref(out) if res else None)
    return rc, lib.mcamd_last_error().decode()


PUT = dict(S0=36.0, K=40.0, r=0.06, v=0.2, T=1.0)
# work_bytes one below what the workspace query states, resolved inside the test: the cases are built at collection
# time, and loading the library then (before torch is imported) would put a second HIP runtime into the GPU run's
# process
SHORT_BY_ONE = object()


def refusals():
    opt, sim, am = capi.make_option(**PUT), capi.make_sim(1000, 50), capi.make_american(n_train=1000)
    A = capi.make_american
    yield "no opt", (None, sim, am), {}, "non-NULL"
    yield "no sim", (opt, None, am), {}, "non-NULL"
    yield "no am", (opt, sim, None), {}, "non-NULL"
    yield "no res", (opt, sim, am), dict(res=False), "non-NULL"
    for p in (2, -1):
        yield f"payoff {p}", (opt, sim, A(payoff=p, n_train=1000)), {}, "payoff"
    for nb in (1, 5, 7):
        yield f"n_basis {nb}", (opt, sim, A(n_basis=nb, n_train=1000)), {}, "n_basis"
    yield "k = 0", (opt, sim, A(exercise_every=0, n_train=1000)), {}, "exercise_every"
    yield "k does not divide", (opt, sim, A(exercise_every=3, n_train=1000)), {}, "exercise_every"
    bad = A(n_train=1000)
    bad.reserved = 1
    yield "reserved", (opt, sim, bad), {}, "reserved"
    yield "n_train 0", (opt, sim, A(n_train=0)), {}, "n_train"
    yield "M > 4096", (opt, capi.make_sim(1000, 4097), am), {}, "4096"
    yield "precision", (opt, capi.make_sim(1000, 50, precision=16), am), {}, "precision"
    yield "window", (capi.make_option(**PUT, B=30.0, P1=0, P2=10, use_window=1), sim, am), {}, "window"
    yield "Tk", (capi.make_option(**PUT, Tk=5), sim, am), {}, "Tk"
    yield "Sk", (capi.make_option(**PUT, Sk=37.0), sim, am), {}, "Sk"
    yield "dt", (capi.make_option(**PUT, dt=0.01), sim, am), {}, "dt"
    yield "v = 0", (capi.make_option(**dict(PUT, v=0.0)), sim, am), {}, "v > 0"
    yield "v < 0", (capi.make_option(**dict(PUT, v=-0.2)), sim, am), {}, "v > 0"
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE,
                  capi.FLAG_LOG_SPACE | capi.FLAG_PRODUCT_FORM, capi.FLAG_LOG_SPACE | capi.FLAG_ANTITHETIC):
        yield f"flags {flags}", (opt, capi.make_sim(1000, 50, flags=flags), am), {}, "flags"
    yield "no d_work", (opt, sim, am), dict(work=None), "d_work"
    yield "work_bytes short by one", (opt, sim, am), dict(work_bytes=SHORT_BY_ONE), "work_bytes"


@pytest.mark.parametrize("case", list(refusals()), ids=lambda c: c[0])
def test_refusals_before_any_device_work(lib, case):
    _, args, kw, words = case
    if kw.get("work_bytes") is SHORT_BY_ONE:
        kw = dict(kw, work_bytes=capi.american_workspace_bytes(args[2], args[1]) - 1)
    rc, msg = price(lib, *args, **kw)
    assert rc == capi.ERR_INVALID and words in msg, msg


def test_workspace_query_refusals(lib):
    sim, am = capi.make_sim(1000, 50), capi.make_american(n_train=1000)
    b = C.c_uint64(7)
    assert lib.mcamd_american_workspace_bytes(None, C.byref(sim), C.byref(b)) == capi.ERR_INVALID
    assert lib.mcamd_american_workspace_bytes(C.byref(am), None, C.byref(b)) == capi.ERR_INVALID
    assert lib.mcamd_american_workspace_bytes(C.byref(am), C.byref(sim), None) == capi.ERR_INVALID
    for bad, words in ((capi.make_american(payoff=3), "payoff"), (capi.make_american(n_basis=1), "n_basis"),
                       (capi.make_american(exercise_every=7), "exercise_every"), (capi.make_american(n_train=0), "n_train")):
        assert lib.mcamd_american_workspace_bytes(C.byref(bad), C.byref(sim), C.byref(b)) == capi.ERR_INVALID
        assert words in lib.mcamd_last_error().decode() and b.value == 0
    with pytest.raises(capi.McamdError):
        capi.american_workspace_bytes(am, capi.make_sim(1000, 4097 * 2, precision=capi.F64))


@pytest.mark.parametrize("payoff", [capi.PAYOFF_CALL, capi.PAYOFF_PUT])
@pytest.mark.parametrize("flags", [0, capi.FLAG_LOG_SPACE, capi.FLAG_PRODUCT_FORM])
@pytest.mark.parametrize("n_basis,k,n_steps", [(0, 1, 50), (2, 5, 250), (3, 50, 50), (4, 1, 4096), (4, 2, 8192)])
def test_accepted_requests_reach_the_missing_context(lib, payoff, flags, n_basis, k, n_steps):
    opt = capi.make_option(**PUT)
    sim = capi.make_sim(1000, n_steps, capi.F32 if k % 2 else capi.F64, flags=flags, path_offset=3, n_paths_local=0)
    am = capi.make_american(payoff=payoff, exercise_every=k, n_basis=n_basis, n_train=999)
    need = capi.american_workspace_bytes(am, sim)
    coeffs = (C.c_double * ((n_steps // k) * ((n_basis or 3) + 1)))()
    rc, msg = price(lib, opt, sim, am, work_bytes=need, coeffs=coeffs)
    assert rc == capi.ERR_INVALID and "ctx" in msg, msg
