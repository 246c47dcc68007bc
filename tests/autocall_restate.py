"""numpy restatement of the worst-of autocallable of include/mcamd.h (mcamd_price_autocall), used by
tests/test_gpu_autocall.py and tested against itself and the host closed form in tests/test_autocall_cpu.py.

samples() follows basket_restate.samples: the normals are the flat stream of a path (row i d + k is z_{i,k}, from
basket_restate.stream / the oracle's generator, or numpy's), everything is carried in one numpy dtype — float32, float64
or longdouble — in natural-log units, with numpy.linalg.cholesky for the factor and the kernel's order of fused
multiply-adds.  The levels ln L_q are narrowed once to the dtype; the payments pay_q stay doubles.  Also here: the inputs
the CPU and the GPU tests share and the records measured from them."""
import math

import numpy as np

import basket_restate as br
from basket_restate import F32, F64, NP_T, MARGIN, CAP, SHALLOW, DEEP, N_LOCAL   # noqa: F401 (shared with the tests)

KI_NONE, KI_AT_MATURITY, KI_EVERY_STEP = 0, 1, 2
MAX_DATES = 64


def tables(n_steps, observe_every, T, r, call_level, coupon, call_step_down=0.0):
    """(L_q, pay_q, t_q) for q = 1..M, each in float64 as the host builds them"""
    M = n_steps // observe_every
    assert M * observe_every == n_steps and 1 <= M <= MAX_DATES
    dt = T / n_steps
    q = np.arange(1, M + 1)
    t = np.array([float(k * observe_every) * dt for k in q])
    level = np.array([call_level - (float(k) - 1.0) * call_step_down for k in q])
    pay = np.array([(1.0 + float(k) * coupon) * math.exp(r * (T - tk)) for k, tk in zip(q, t)])
    return level, pay, t


def samples(z, n_steps, v, corr, T, r, observe_every, call_level, coupon, ki_level=0.0, ki_monitoring=KI_NONE,
            call_step_down=0.0, first_call_date=1, dtype=np.float64):
    """z: [>= n_steps d, n_paths] normals, row i d + k = z_{i,k}.  Returns a dict: y (float64 samples in maturity money,
    or longdouble when dtype is), date (the date the path is called at, 0: never), knocked (the knock-in flag, whether
    or not the path is called), live (the steps the path entered not yet called), l_n (the log of the worst performance
    at maturity) and min_abs_d: the smallest |l - ln L_q| over the observation dates and the smallest |l - ln ki_level|
    over the monitored steps, along the whole path whether or not it has been called (natural-log units)."""
    dt_ = np.dtype(dtype)
    f = dt_.type
    d = len(v)
    n = z.shape[1]
    assert z.shape[0] >= n_steps * d
    v = np.asarray(v, dtype=np.float64)
    L = np.linalg.cholesky(np.asarray(corr, dtype=np.float64)[:d, :d])
    dt = T / n_steps                                        # the host's fp64 set-up, narrowed once
    drift = ((r - 0.5 * v * v) * dt).astype(dt_)
    coef = (v[:, None] * math.sqrt(dt) * L).astype(dt_)
    level, pay, _ = tables(n_steps, observe_every, T, r, call_level, coupon, call_step_down)
    log_level = np.log(level).astype(dt_)
    log_ki = f(math.log(ki_level)) if ki_monitoring != KI_NONE else None
    wide = np.longdouble if dt_ == np.dtype(np.longdouble) else np.float64

    X = [np.zeros(n, dtype=dt_) for _ in range(d)]
    date = np.zeros(n, dtype=np.int64)
    knocked = np.zeros(n, dtype=bool)
    min_abs_d = np.full(n, np.inf)
    l = None
    for i in range(1, n_steps + 1):
        x = [np.full(n, drift[j], dtype=dt_) for j in range(d)]
        for k in range(d):
            zk = z[(i - 1) * d + k].astype(dt_)
            for j in range(k, d):
                x[j] = br._fma(coef[j, k], zk, x[j], dt_)
        X = [X[j] + x[j] for j in range(d)]
        l = X[0]
        for j in range(1, d):
            l = np.minimum(l, X[j])
        if ki_monitoring == KI_EVERY_STEP or (ki_monitoring == KI_AT_MATURITY and i == n_steps):
            knocked |= l <= log_ki
            min_abs_d = np.minimum(min_abs_d, np.abs((l - log_ki).astype(np.float64)))
        if i % observe_every == 0:
            q = i // observe_every
            min_abs_d = np.minimum(min_abs_d, np.abs((l - log_level[q - 1]).astype(np.float64)))
            if q >= first_call_date:
                date = np.where((date == 0) & (l >= log_level[q - 1]), q, date)
    called = date > 0
    A = np.exp(l).astype(wide)
    y = np.where(knocked, np.minimum(A, wide(1)), wide(1))
    y = np.where(called, pay[np.maximum(date, 1) - 1].astype(wide), y)   # at date M the call test comes first
    live = np.where(called, date * observe_every, n_steps)
    return dict(y=y, date=date, knocked=knocked, live=live, l_n=l, min_abs_d=min_abs_d)


def single_date_by_quadrature(T, r, v, call_level, coupon, ki_level, ki_monitoring, panels=400, reach=10.0):
    """e^{-rT} E[y] of the note on one asset with one date, by Gauss-Legendre over the normal that makes S_T / S_0,
    with panel edges on the two kinks of the payoff — written without reference to the C code"""
    s = v * math.sqrt(T)
    mu = (r - 0.5 * v * v) * T
    kinks = [(math.log(call_level) - mu) / s]
    if ki_monitoring != KI_NONE:
        kinks.append((math.log(ki_level) - mu) / s)
    edges = np.unique(np.concatenate([np.linspace(-reach, reach, panels + 1), [k for k in kinks if abs(k) < reach]]))
    gx, gw = np.polynomial.legendre.leggauss(16)
    h, c = 0.5 * np.diff(edges), 0.5 * (edges[:-1] + edges[1:])
    zq = (c[:, None] + h[:, None] * gx[None, :]).ravel()
    wq = (h[:, None] * gw[None, :]).ravel() * np.exp(-0.5 * zq * zq) / math.sqrt(2.0 * math.pi)
    perf = np.exp(mu + s * zq)
    y = np.ones_like(perf)
    if ki_monitoring != KI_NONE:
        y = np.where(perf <= ki_level, np.minimum(perf, 1.0), y)
    y = np.where(perf >= call_level, 1.0 + coupon, y)
    return math.exp(-r * T) * float(np.dot(wq, y))


# ---- what the CPU and the GPU tests share --------------------------------------------------------------------------------

R, T_ = br.R, br.T_
COUPON = 0.03
KI_LEVEL = 0.7
KI_MODES = (KI_AT_MATURITY, KI_EVERY_STEP)
DS = tuple(range(1, 9))
# (n_steps, observe_every): with G = 2 and G = 4 steps a group these leave every remainder but the whole group, put
# observation dates inside a group, and (50, 10) — the case with a non-zero call_step_down — has five dates.
SHAPES = ((1, 1), (2, 1), (7, 1), (7, 7), (6, 3), (50, 10))
STEP_DOWN = {(50, 10): 0.02}
DEEP_SHAPE = (7, 1)


def inputs(d):
    """v_j = 0.15 + 0.05 j and corr_jk = 0.6^|j - k|: the basket tests' assets, without their spots"""
    _, v, corr = br.inputs(d)
    return v, corr


def call_level(d, shape):
    """The first autocall level of a case.  The worst of d performances falls with d, and a note of one date is called
    less often than one of several, so one level cannot leave both more than 5 % of the paths called and more than 5 %
    not called at every width and shape: 1.05 at d = 1, then lower with d (0.93 at d = 8)."""
    return round(1.05 - 0.12 * math.log2(d) / 3.0, 4)


def terms(d, shape, ki):
    n_steps, every = shape
    return dict(observe_every=every, call_level=call_level(d, shape), coupon=COUPON, ki_level=KI_LEVEL, ki_monitoring=ki,
                call_step_down=STEP_DOWN.get(shape, 0.0), first_call_date=1)


CASES = [(d, ki, shape, SHALLOW) for d in DS for ki in KI_MODES for shape in SHAPES] + \
        [(d, ki, DEEP_SHAPE, DEEP) for d in DS for ki in KI_MODES]

_restated = {}


def compare(prec, d, ki, shape, where=SHALLOW):
    """The restatement of one case of the GPU test's elementwise comparison on its inputs, CPU only: (the restatement
    in the kernel's precision, the wider one, paths kept, largest difference of the two over the kept paths).  A path is
    kept if min_abs_d >= MARGIN in both."""
    key = (prec, d, ki, shape, where)
    if key not in _restated:
        v, corr = inputs(d)
        n_steps = shape[0]
        z = br.stream(prec) if where == SHALLOW else br.stream(prec, where[0], where[1], n_normals=max(br.DS) * br.DEEP_STEPS)
        t = terms(d, shape, ki)
        own = samples(z, n_steps, v, corr, T_, R, dtype=NP_T[prec], **t)
        other = samples(z, n_steps, v, corr, T_, R, dtype=np.longdouble if prec == F64 else np.float64, **t)
        keep = (own["min_abs_d"] >= MARGIN) & (other["min_abs_d"] >= MARGIN)
        spread = float(np.abs(own["y"] - other["y"])[keep].max())
        _restated[key] = (own, other, keep, spread)
    return _restated[key]


# Largest elementwise difference between two restatements over CASES (float64 against longdouble for the fp64 kernels,
# float32 against float64 for the fp32 kernels; margin paths left out), and the largest share of paths a case leaves
# out, measured by tests/test_autocall_cpu.py on an x86-64 CPU (80-bit longdouble) and recorded in DESIGN section 17.
# The test there fails if a measurement exceeds its record.
SPREAD = {F64: 4.8e-16, F32: 2.4e-7}
EXCLUDED = {F64: 0.0032, F32: 0.0027}


def elementwise_tolerance(prec, want):
    """Absolute tolerance per element of a path not called: 4 x SPREAD, floored at 1e-11 of the sample (fp64) / 2e-5
    (fp32: the project's 2e-3 on prices of size 100, on samples of size 1)."""
    if prec == F64:
        return np.maximum(4.0 * SPREAD[F64], 1e-11 * np.abs(want))
    return np.full(np.shape(want), max(4.0 * SPREAD[F32], 2e-5))


# The record price: a 3-asset quarterly one-year note priced by the restatement in float64 on numpy's normals.
NOTE = dict(d=3, n_steps=12, observe_every=3, call_level=1.0, coupon=0.02, ki_level=0.7, ki_monitoring=KI_EVERY_STEP,
            call_step_down=0.0, first_call_date=1)
NOTE_SEED, NOTE_PATHS = 20261018, 400_000
NOTE_RECORD = (0.9485140352431516, 0.00018403664564582722)   # (price, SE)


def price_note():
    p = dict(NOTE)
    d, n_steps = p.pop("d"), p.pop("n_steps")
    v, corr = inputs(d)
    z = np.random.default_rng(NOTE_SEED).standard_normal((n_steps * d, NOTE_PATHS))
    y = samples(z, n_steps, v, corr, T_, R, **p)["y"]
    disc = math.exp(-R * T_)
    return disc * float(y.mean()), disc * float(y.std(ddof=1)) / math.sqrt(NOTE_PATHS)
