"""The inputs of the per-path Greeks tests of tests/test_gpu_greeks.py, their restatements and the tolerance taken from
them.  No kernel runs here: tests/test_greeks_cpu.py checks all of it on the CPU.

A Greeks call has no per-path output, so a path is looked at through a shard of one: with n_paths_local = 1 and
path_offset = id the record's sum[k] is that path's sample q_k and sumsq[k] is q_k^2.

Inputs: S0 = K = 100, T = 1, r = 0.1, v = 0.2; N_PATHS consecutive paths from SHALLOW (ids 5003.. under seed 77) or DEEP
(ids 2^33 + 5003.. of a job of 2^40 paths under seed 2^40 + 77) of tests/deep_inputs.py.  n_sim = n_steps - Tk of 1, 2, 3,
5, 6, 7 leaves 1, 2, 3, 1, 2, 3 steps in the last Philox block in fp32 (4 normals a block) and 1, 0, 1, 1, 0, 1 in fp64
(2 a block); n_sim < 4 (fp32) and n_sim = 1 (fp64) have no full block at all.

Tolerance (tolerance() below), per path and estimator k: the larger of
  * four times the largest elementwise difference between two restatements of tests/greeks_restate.py — float64 and
    longdouble for an fp64 kernel, float32 and float64 for an fp32 kernel — over all CASES of the method, and
  * FLOOR[prec][k] times max(|q_k|, mean |q_k| over the case's paths): the allowances of the record tests of
    tests/test_gpu_greeks.py, 1e-10 (fp64) and 2e-5 for the price, 2e-3 for the others (fp32), per path.  A sample near
    zero keeps a meaningful absolute bound through the mean.
Both kernels are compared with the float64 restatement.

Paths left out (left_out() below), fp32 only: the pathwise delta, gamma, vega, rho and theta jump where S_T crosses K,
and every windowed LR sample jumps where ln S_t crosses ln B at a step whose flip moves the count into or out of
[P1, P2].  A path whose float64 restatement has |S_T / K - 1| < NEAR, or such a step with |ln(S_t / B)| < NEAR, is left
out of those estimators (a pathwise path keeps its price sample, which is continuous at the strike); at most MAX_LEFT_OUT
of a case's N_PATHS paths.  In fp64 nothing is left out.

The windows (B = 120, the count starts at Ik): every case pays on a fifth of its paths or more and on no more than four
fifths (tests/test_greeks_cpu.py).  (P1, P2) = (1, 3) at 6 steps paid on 0.191 of the fp64 paths only, so that case takes
(1, 4): 0.277 and 0.332.  From Sk = 93.5 with Ik = 1, P1 = 2, P2 = 5 and three steps to go the window shuts on no path
(the count stays within 1..4 and is 1 on none), so a second restart case, from 110 with the window [2, 3], follows it.
The small-shard cases take the window [0, 2] at 3 steps: none of their 513 (257 deep) paths has a step within NEAR of
the barrier whose flip would matter, so their sums leave nothing out."""
import collections
import importlib

import numpy as np

import greeks_restate as gr
from deep_inputs import DEEP, SHALLOW

capi = importlib.import_module("monte-carlo-project-cuda_amd").capi

PW, LR = capi.GREEKS_PATHWISE, capi.GREEKS_LIKELIHOOD_RATIO
assert (PW, LR, capi.F32, capi.F64) == (gr.PATHWISE, gr.LIKELIHOOD_RATIO, gr.F32, gr.F64)
PRECS = (capi.F64, capi.F32)
OPTION = dict(S0=100.0, T=1.0, K=100.0, r=0.1, v=0.2)
N_PATHS = 256
NEAR, MAX_LEFT_OUT = 1e-4, 2
FLOOR = {capi.F64: (1e-10,) * 6, capi.F32: (2e-5,) + (2e-3,) * 5}
OTHER = {capi.F64: np.longdouble, capi.F32: np.float64}   # the second restatement of the spread
OWN = {capi.F64: np.float64, capi.F32: np.float32}

Case = collections.namedtuple("Case", "name method extra n_steps where")


def _window(P1, P2, **more):
    return dict(B=120.0, P1=P1, P2=P2, use_window=1, **more)


def _case(kind, method, extra, n_steps, where):
    tag = "".join(f"-{k}={v:g}" for k, v in extra.items() if k not in ("B", "use_window"))
    return Case(f"{kind}{tag}-{n_steps}" + ("-deep" if where == DEEP else ""), method, extra, n_steps, where)


PW_CASES = [_case("pw", PW, {}, n, SHALLOW) for n in (1, 2, 3, 5, 6, 7)] + [
    _case("pw", PW, {}, 7, DEEP),
    _case("pw", PW, dict(Sk=95.0, Tk=4), 7, SHALLOW),        # n_sim = 3, theta off
    _case("pw", PW, dict(dt=1.0 / 50), 6, SHALLOW)]          # theta off
LR_CASES = [_case("lr", LR, {}, n, SHALLOW) for n in (1, 2, 3, 5, 6, 7)] + [_case("lr", LR, {}, n, DEEP) for n in (3, 7)]
WINDOW_CASES = [_case("lrw", LR, _window(P1, P2), n, SHALLOW) for P1, P2, n in ((0, 1, 3), (1, 4, 6), (2, 5, 7))] + [
    _case("lrw", LR, _window(2, 5), 7, DEEP),
    _case("lrw", LR, _window(2, 5, Ik=1, Sk=93.5, Tk=4), 7, SHALLOW),   # n_sim = 3, the count starts at 1
    _case("lrw", LR, _window(2, 3, Ik=1, Sk=110.0, Tk=4), 7, SHALLOW)]  # its twin whose window shuts at both ends
ALWAYS_OPEN = WINDOW_CASES[-2]   # from 93.5 the count 1 + (steps below 120) leaves [2, 5] on none of the paths
CASES = PW_CASES + LR_CASES + WINDOW_CASES
SHARD_SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513)
SHARD_CASES = [Case("pw-3", PW, {}, 3, SHALLOW), Case("lrw-3", LR, _window(0, 2), 3, SHALLOW),
               Case("pw-3-deep", PW, {}, 3, DEEP), Case("lrw-3-deep", LR, _window(0, 2), 3, DEEP)]


def shard_sizes(case):
    return SHARD_SIZES if case.where == SHALLOW else (1, 2, 3, 4, 5, 257)


def option(case):
    return capi.make_option(**dict(OPTION, **case.extra))


def sim(case, prec, first=None, n_local=N_PATHS, n_job=None):
    """the shard of n_local paths from `first` (by default the first path of case.where) of the case's job"""
    seed, start, job = case.where
    first = start if first is None else first
    return capi.make_sim(max(job, first + n_local) if n_job is None else n_job, case.n_steps, prec, seed=seed,
                         path_offset=first, n_paths_local=n_local)


_restated = {}


def restated(case, prec, dtype, n=N_PATHS):
    """greeks_restate.restate of the case's first n paths in dtype, from the normals of prec; computed once"""
    from oracle import pyoracle
    key = (case.name, case.where, prec, np.dtype(dtype), n)
    if key not in _restated:
        _restated[key] = gr.restate(pyoracle, option(case), sim(case, prec, n_local=n), case.method, dtype)
    return _restated[key]


def left_out(case, prec, n=N_PATHS):
    """[n, 6] bool: the (path, estimator) pairs that are not compared.  From the float64 restatement alone."""
    out = np.zeros((n, 6), dtype=bool)
    if prec == capi.F64:
        return out
    r = restated(case, prec, np.float64, n)
    opt = option(case)
    if case.method == PW:
        out[:, 1:] = (np.abs(r.S_T / opt.K - 1.0) < NEAR)[:, None]
    elif opt.use_window:
        d = r.logs - np.log(opt.B / (opt.Sk if opt.Sk != 0 else opt.S0))      # ln(S_t / B)
        flipped = r.count[:, None] + np.where(d < 0, -1, 1)                    # the count with that one step flipped
        inside = lambda c: (c >= opt.P1) & (c <= opt.P2)
        out[:, :5] = ((np.abs(d) < NEAR) & (inside(flipped) != inside(r.count)[:, None])).any(axis=1)[:, None]
    return out


_spread = {}


def spreads(prec, method):
    """[6]: per estimator, the largest elementwise difference between the two restatements over the method's CASES
    (the compared pairs only)"""
    if (prec, method) not in _spread:
        worst = np.zeros(6)
        for case in CASES:
            if case.method == method:
                a, b = restated(case, prec, OWN[prec]).q, restated(case, prec, OTHER[prec]).q
                diff = np.abs(a.astype(np.longdouble) - b.astype(np.longdouble)).astype(np.float64)
                worst = np.maximum(worst, np.where(left_out(case, prec), 0.0, diff).max(axis=0))
        _spread[prec, method] = worst
    return _spread[prec, method]


def tolerance(prec, method, want):
    """[n, 6] absolute tolerance of the samples `want` ([n, 6], the float64 restatement of one case or shard)"""
    mag = np.maximum(np.abs(want), np.abs(want).mean(axis=0))
    return np.maximum(4.0 * spreads(prec, method), np.asarray(FLOOR[prec]) * mag)


def wanted(case, prec, n=N_PATHS):
    """(float64 samples to compare with [n, 6], tolerance [n, 6], left out [n, 6])"""
    want = restated(case, prec, np.float64, n).q
    return want, tolerance(prec, case.method, want), left_out(case, prec, n)
