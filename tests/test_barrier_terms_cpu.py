"""CPU-only: what the calls that take a monitoring or a single barrier refuse of them, pinned across the calls
(csrc/capi_pathdep.cpp: check_monitoring, check_barrier_terms).  Refusals come before the context is looked at, so every
call here is given none; no kernel runs.

  1. mcamd_price_barrier, mcamd_price_lookback, mcamd_price_localvol and mcamd_price_heston_barrier refuse a monitoring of
     2 and of -1 with one code and one text, in the synchronous and in the enqueue form;
  2. mcamd_price_barrier and mcamd_price_heston_barrier refuse each defect of the barrier — reserved, the kind, the
     payoff, B = 0, B = NaN, a spot on the wrong side of a down- and of an up-barrier — with the same code and text;
  3. and in the same order: a request with two of these defects is refused for the earlier one by both calls.

The texts are the library's as it was before these checks were shared: the test passes on that library too."""
import ctypes as C
import importlib
import itertools
import os

import pytest

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
NAN = float("nan")
SPOT = 100.0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    return capi.load()


def request_(B=90.0):
    return capi.make_option(S0=SPOT, K=100.0, v=0.2, B=B, r=0.05, T=1.0), capi.make_sim(1000, 12)


def barrier_of(kind=capi.BARRIER_DOWN_OUT, payoff=capi.PAYOFF_CALL, monitoring=capi.MONITOR_CONTINUOUS, reserved=0, **_):
    b = capi.make_barrier(kind, payoff, monitoring)
    b.reserved = reserved
    return b


# Each caller takes the barrier's fields (kind, payoff, monitoring, reserved, B) and the form, and returns (code, text).
def call_barrier(lib, enqueue, **f):
    opt, sim = request_(f.get("B", 90.0))
    bar = barrier_of(**f)
    if enqueue:
        rc = lib.mcamd_price_barrier_enqueue(None, C.byref(opt), C.byref(sim), C.byref(bar), None, None)
    else:
        rc = lib.mcamd_price_barrier(None, C.byref(opt), C.byref(sim), C.byref(bar), None, C.byref(capi.Result()))
    return rc, lib.mcamd_last_error().decode()


def call_heston_barrier(lib, enqueue, **f):
    opt, sim = request_(f.get("B", 90.0))
    bar = barrier_of(**f)
    hs = capi.make_heston(capi.PAYOFF_CALL)
    if enqueue:
        rc = lib.mcamd_price_heston_barrier_enqueue(None, C.byref(opt), C.byref(sim), C.byref(hs), C.byref(bar), None, None,
                                                    None)
    else:
        rc = lib.mcamd_price_heston_barrier(None, C.byref(opt), C.byref(sim), C.byref(hs), C.byref(bar), None, None,
                                            C.byref(capi.HestonBarrierResult()))
    return rc, lib.mcamd_last_error().decode()


def call_lookback(lib, enqueue, monitoring):
    opt, sim = request_()
    lb = capi.make_lookback(capi.LOOKBACK_FLOATING, capi.PAYOFF_CALL, monitoring)
    if enqueue:
        rc = lib.mcamd_price_lookback_enqueue(None, C.byref(opt), C.byref(sim), C.byref(lb), None, None)
    else:
        rc = lib.mcamd_price_lookback(None, C.byref(opt), C.byref(sim), C.byref(lb), None, C.byref(capi.Result()))
    return rc, lib.mcamd_last_error().decode()


def call_localvol(lib, enqueue, monitoring):
    opt, sim = request_()
    lv = capi.make_localvol(capi.PAYOFF_CALL, capi.BARRIER_DOWN_OUT, monitoring)
    if enqueue:
        rc = lib.mcamd_price_localvol_enqueue(None, C.byref(opt), C.byref(sim), C.byref(lv), None, None, None)
    else:
        rc = lib.mcamd_price_localvol(None, C.byref(opt), C.byref(sim), C.byref(lv), None, None, C.byref(capi.Result()))
    return rc, lib.mcamd_last_error().decode()


# ---- 1. the monitoring ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("monitoring", [2, -1])
def test_the_four_calls_refuse_a_monitoring_with_one_code_and_one_text(lib, monitoring):
    want = (capi.ERR_INVALID,
            f"monitoring must be MCAMD_MONITOR_DISCRETE (0) or MCAMD_MONITOR_CONTINUOUS (1), got {monitoring}")
    for enqueue in (False, True):
        assert call_barrier(lib, enqueue, monitoring=monitoring) == want
        assert call_lookback(lib, enqueue, monitoring) == want
        assert call_localvol(lib, enqueue, monitoring) == want
        assert call_heston_barrier(lib, enqueue, monitoring=monitoring) == want


def test_both_monitorings_pass_the_four_calls(lib):
    """the refusal above is the monitoring's: with 0 and 1 every call goes on to its context"""
    for monitoring in (capi.MONITOR_DISCRETE, capi.MONITOR_CONTINUOUS):
        for enqueue in (False, True):
            for got in (call_barrier(lib, enqueue, monitoring=monitoring), call_lookback(lib, enqueue, monitoring),
                        call_heston_barrier(lib, enqueue, monitoring=monitoring)):
                assert got == (capi.ERR_INVALID, "ctx is NULL")
            # the local-volatility call looks at its surface first
            rc, msg = call_localvol(lib, enqueue, monitoring)
            assert rc == capi.ERR_INVALID and "surface" in msg


# ---- 2. and 3. the barrier's terms ----------------------------------------------------------------------------------------

# in the order of the refusals: (name, the fields that carry the defect, words of its text)
DEFECTS = [
    ("monitoring 2", dict(monitoring=2), "monitoring must be"),
    ("reserved 1", dict(reserved=1), "barrier->reserved must be 0, got 1"),
    ("kind 4", dict(kind=4), "barrier kind must be MCAMD_BARRIER_DOWN_OUT (0) .. MCAMD_BARRIER_UP_IN (3), got 4"),
    ("payoff 2", dict(payoff=2), "payoff"),
    ("B = 0", dict(B=0.0), "the barrier level B must be positive, got 0"),
    ("B = NaN", dict(B=NAN), "the barrier level B must be positive, got nan"),
    ("down-barrier above the spot", dict(kind=capi.BARRIER_DOWN_IN, B=110.0), "a down-barrier needs S0 > B"),
    ("up-barrier below the spot", dict(kind=capi.BARRIER_UP_OUT, B=90.0), "an up-barrier needs 0 < S0 < B"),
]


def both_calls(lib, fields):
    """the refusal of both calls in both forms, which must be one"""
    got = {(name, enqueue): call(lib, enqueue, **fields)
           for name, call in (("barrier", call_barrier), ("heston barrier", call_heston_barrier)) for enqueue in (False, True)}
    assert len(set(got.values())) == 1, got
    return got["barrier", False]


@pytest.mark.parametrize("defect", DEFECTS, ids=lambda d: d[0])
def test_both_barrier_calls_refuse_a_defect_with_the_same_code_and_text(lib, defect):
    _, fields, words = defect
    rc, msg = both_calls(lib, fields)
    assert rc == capi.ERR_INVALID and words in msg, msg


def two_defects():
    """every pair of defects that one request can carry: the later one's fields, then the earlier one's on top"""
    for (a, fa, _), (b, fb, _) in itertools.combinations(DEFECTS, 2):
        if all(fa[k] == fb[k] for k in fa.keys() & fb.keys()):
            yield f"{a}, {b}", fa, dict(fb, **fa)
    # B = 0 below an up-barrier's spot: the level is refused, not the side
    yield "B = 0, an up-barrier", dict(B=0.0), dict(kind=capi.BARRIER_UP_OUT, B=0.0)


@pytest.mark.parametrize("case", list(two_defects()), ids=lambda c: c[0])
def test_both_barrier_calls_refuse_the_earlier_of_two_defects(lib, case):
    _, earlier, both = case
    want = both_calls(lib, earlier)
    assert want[0] == capi.ERR_INVALID
    assert both_calls(lib, both) == want
