"""numpy restatement of the worst-of autocallable under per-asset local-volatility surfaces of include/mcamd.h
(mcamd_price_autocall_localvol), used by tests/test_gpu_autocall_localvol.py and tested against the restatements it
collapses onto in tests/test_autocall_localvol_cpu.py.  Written from the header text.

samples() carries everything in one numpy dtype — float32, float64 or longdouble — in natural-log units: the pair tables,
the lookup and the slice rule are localvol_restate's (tables / lookup / row_of), asset by asset; the normals are the flat
stream of a path (row i d + k is z_{i,k}, from basket_restate.stream or numpy's); the correlated normal w_j is the chain
of fused multiply-adds from 0 in ascending k (basket_restate._fma); the dates, levels and payments are
autocall_restate.tables'.  Also here: the inputs the CPU and the GPU tests share, the records measured from them, and the
mistakes the GPU test module restates to show which of its tests refuses each."""
import math

import numpy as np

import autocall_restate as ar
import basket_restate as br
import localvol_restate as lr
from autocall_restate import (F32, F64, NP_T, MARGIN, CAP, SHALLOW, DEEP, N_LOCAL, KI_NONE, KI_AT_MATURITY,   # noqa: F401
                              KI_EVERY_STEP, DS, KI_MODES, SHAPES, STEP_DOWN, DEEP_SHAPE, COUPON, KI_LEVEL, R, T_)

# the mistakes samples() can make on request (test 8 of the GPU module)
TABLE_BASE_OF_ASSET_0, SHARED_ROW_CARRY, NO_DIVIDEND, W_FROM_DRIFT = "base0", "row0", "no_q", "w_drift"


def samples(z, n_steps, grids, sigmas, q, corr, T, r, observe_every, call_level, coupon, ki_level=0.0,
            ki_monitoring=KI_NONE, call_step_down=0.0, first_call_date=1, dtype=np.float64, mistake=None):
    """z: [>= n_steps d, n_paths] normals, row i d + k = z_{i,k}.  grids[j] = (n_t, n_x, x_min, x_max) and sigmas[j] =
    n_t rows of n_x volatilities: asset j's surface.  Returns a dict: y (float64 samples in maturity money, or longdouble
    when dtype is), date (the date the path is called at, 0: never), knocked (the knock-in flag, whether or not the path
    is called), live (the steps the path entered not yet called), X ([d, n_paths] log-performances at maturity), l_n
    (their minimum) and min_abs_d: the smallest |l - ln L_q| over the observation dates and the smallest
    |l - ln ki_level| over the monitored steps, along the whole path whether or not it has been called."""
    dt_ = np.dtype(dtype)
    f = dt_.type
    d = len(grids)
    n = z.shape[1]
    assert z.shape[0] >= n_steps * d and len(sigmas) == d and len(q) >= d
    chol = np.linalg.cholesky(np.asarray(corr, dtype=np.float64)[:d, :d]).astype(dt_)   # narrowed once
    tabs = [lr.tables(grids[j], sigmas[j], dt_) for j in range(d)]
    dt = T / n_steps                                        # the host's fp64 set-up, narrowed once
    qq = np.zeros(d) if mistake == NO_DIVIDEND else np.asarray(q, dtype=np.float64)[:d]
    mu_dt = ((r - qq) * dt).astype(dt_)
    half_dt, sqrt_dt = f(0.5 * dt), f(math.sqrt(dt))
    level, pay, _ = ar.tables(n_steps, observe_every, T, r, call_level, coupon, call_step_down)
    log_level = np.log(level).astype(dt_)
    log_ki = f(math.log(ki_level)) if ki_monitoring != KI_NONE else None
    wide = np.longdouble if dt_ == np.dtype(np.longdouble) else np.float64
    if mistake == TABLE_BASE_OF_ASSET_0:
        # the d tables back to back, as the kernel holds them; asset j then indexes from entry 0 with its own strides
        flat_sigma = np.concatenate([t[0].ravel() for t in tabs])
        flat_slope = np.concatenate([t[1].ravel() for t in tabs])

    def sigma(j, i, X):
        n_t, n_x = grids[j][0], grids[j][1]
        row = lr.row_of(i, grids[0][0] if mistake == SHARED_ROW_CARRY else n_t, n_steps)
        row = min(row, n_t - 1)   # (the shared carry can run past a shorter table; the mistake is shown without that)
        if mistake != TABLE_BASE_OF_ASSET_0:
            return lr.lookup(tabs[j], n_x, row, X)
        _, _, x_min, inv_dx = tabs[j]
        u = np.minimum(np.maximum((X - x_min) * inv_dx, f(0)), f(n_x - 1))
        k = np.minimum(np.floor(u).astype(np.int64), n_x - 2)
        e = row * n_x + k
        return (u - k.astype(dt_)) * flat_slope[e] + flat_sigma[e]

    X = [np.zeros(n, dtype=dt_) for _ in range(d)]
    date = np.zeros(n, dtype=np.int64)
    knocked = np.zeros(n, dtype=bool)
    min_abs_d = np.full(n, np.inf)
    l = None
    for i in range(n_steps):
        s = [sigma(j, i, X[j]) for j in range(d)]
        w = [np.full(n, mu_dt[j] if mistake == W_FROM_DRIFT else f(0), dtype=dt_) for j in range(d)]
        for k in range(d):
            zk = z[i * d + k].astype(dt_)
            for j in range(k, d):
                w[j] = br._fma(chol[j, k], zk, w[j], dt_)
        X = [X[j] + br._fma(s[j] * sqrt_dt, w[j], br._fma(-(s[j] * s[j]), half_dt, mu_dt[j], dt_), dt_) for j in range(d)]
        l = X[0]
        for j in range(1, d):
            l = np.minimum(l, X[j])
        step = i + 1
        if ki_monitoring == KI_EVERY_STEP or (ki_monitoring == KI_AT_MATURITY and step == n_steps):
            knocked |= l <= log_ki
            min_abs_d = np.minimum(min_abs_d, np.abs((l - log_ki).astype(np.float64)))
        if step % observe_every == 0:
            k = step // observe_every
            min_abs_d = np.minimum(min_abs_d, np.abs((l - log_level[k - 1]).astype(np.float64)))
            if k >= first_call_date:
                date = np.where((date == 0) & (l >= log_level[k - 1]), k, date)
    called = date > 0
    A = np.exp(l).astype(wide)
    y = np.where(knocked, np.minimum(A, wide(1)), wide(1))
    y = np.where(called, pay[np.maximum(date, 1) - 1].astype(wide), y)   # at date M the call test comes first
    live = np.where(called, date * observe_every, n_steps)
    return dict(y=y, date=date, knocked=knocked, live=live, X=np.stack(X), l_n=l, min_abs_d=min_abs_d)


# ---- what the CPU and the GPU tests share --------------------------------------------------------------------------------

Q = (0.0, 0.03, 0.01, 0.02, 0.0, 0.04, 0.015, 0.025)
# Asset j takes GRIDS[j % 4]: rows that do not divide the step counts (4 and 3 of 7; 7 of 50), rows that exceed them
# (7 of 1, 2 and 6 steps), a two-node table, and a different table base per asset.  496 nodes at d = 8.
GRIDS = ((4, 33, -1.5, 1.5), (1, 2, -0.5, 0.5), (3, 17, -1.0, 1.0), (7, 9, -0.8, 0.8))


def grid(j):
    return GRIDS[j % 4]


def skewed(j):
    """asset j's surface: sigma_j(t, x_k) = (0.15 + 0.05 j) (0.9 + 0.07 t) (1 + 0.5 e^{-x_k}) / 1.5, t the slice index"""
    n_t, n_x, x_min, x_max = grid(j)
    x = x_min + np.arange(n_x) * ((x_max - x_min) / (n_x - 1))
    t = np.arange(n_t)
    return (0.15 + 0.05 * j) * (0.9 + 0.07 * t)[:, None] * (1.0 + 0.5 * np.exp(-x))[None, :] / 1.5


def flat(j, v=None):
    """asset j's grid with one volatility everywhere (v_j = 0.15 + 0.05 j, the autocall tests' assets, by default)"""
    n_t, n_x = grid(j)[:2]
    return np.full((n_t, n_x), 0.15 + 0.05 * j if v is None else v)


def corr(d):
    return ar.inputs(d)[1]   # 0.6^|j - k|


def surfaces(d, kind=skewed):
    return [grid(j) for j in range(d)], [kind(j) for j in range(d)]


def call_level(d, shape=None):
    return ar.call_level(d, shape)


def terms(d, shape, ki):
    return ar.terms(d, shape, ki)


CASES = ar.CASES   # d = 1..8 x both knock-in modes x the six shapes on SHALLOW, and DEEP_SHAPE on DEEP

_restated = {}


def stream_of(prec, where):
    return br.stream(prec) if where == SHALLOW else br.stream(prec, where[0], where[1], n_normals=max(br.DS) * br.DEEP_STEPS)


def compare(prec, d, ki, shape, where=SHALLOW):
    """The restatement of one case of the GPU test's elementwise comparison on its inputs, CPU only: (the restatement
    in the kernel's precision, the wider one, paths kept, largest difference of the two over the kept paths not
    called).  A path is kept if min_abs_d >= MARGIN in both."""
    key = (prec, d, ki, shape, where)
    if key not in _restated:
        grids, sig = surfaces(d)
        z = stream_of(prec, where)
        t = terms(d, shape, ki)
        own = samples(z, shape[0], grids, sig, Q, corr(d), T_, R, dtype=NP_T[prec], **t)
        other = samples(z, shape[0], grids, sig, Q, corr(d), T_, R, dtype=np.longdouble if prec == F64 else np.float64, **t)
        keep = (own["min_abs_d"] >= MARGIN) & (other["min_abs_d"] >= MARGIN)
        spread = float(np.abs(own["y"] - other["y"])[keep].max())
        _restated[key] = (own, other, keep, spread)
    return _restated[key]


# Largest elementwise difference between two restatements over CASES (float64 against longdouble for the fp64 kernels,
# float32 against float64 for the fp32 kernels; margin paths left out), and the largest share of paths a case leaves
# out, measured by tests/test_autocall_localvol_cpu.py on an x86-64 CPU (80-bit longdouble) and recorded in DESIGN
# section 20.  The test there fails if a measurement exceeds its record.
SPREAD = {F64: 3.8e-16, F32: 2.2e-7}
EXCLUDED = {F64: 0.0035, F32: 0.0042}


def elementwise_tolerance(prec, want):
    """Absolute tolerance per element of a path not called: 4 x SPREAD, floored at 1e-11 of the sample (fp64) / 2e-5
    (fp32: the project's 2e-3 on prices of size 100, on samples of size 1)."""
    if prec == F64:
        return np.maximum(4.0 * SPREAD[F64], 1e-11 * np.abs(want))
    return np.full(np.shape(want), max(4.0 * SPREAD[F32], 2e-5))


# The record price: a 3-asset quarterly one-year note under the skewed surfaces and Q, priced by the restatement in
# float64 on numpy's normals.
NOTE = dict(d=3, n_steps=12, observe_every=3, call_level=1.0, coupon=0.02, ki_level=0.7, ki_monitoring=KI_EVERY_STEP,
            call_step_down=0.0, first_call_date=1)
NOTE_SEED, NOTE_PATHS = 20261019, 400_000
NOTE_RECORD = (0.9445786887980654, 0.00019531261464888447)   # (price, SE)


def price_note():
    p = dict(NOTE)
    d, n_steps = p.pop("d"), p.pop("n_steps")
    grids, sig = surfaces(d)
    z = np.random.default_rng(NOTE_SEED).standard_normal((n_steps * d, NOTE_PATHS))
    y = samples(z, n_steps, grids, sig, Q, corr(d), T_, R, **p)["y"]
    disc = math.exp(-R * T_)
    return disc * float(y.mean()), disc * float(y.std(ddof=1)) / math.sqrt(NOTE_PATHS)


# One asset, one date, a surface that varies in time only: S_T / S_0 is lognormal with the rms volatility of the rows
# the steps use, and mcamd_autocall_single_date_price_f64 prices the note.
TIME_ONLY_GRID = (4, 2, -1.0, 1.0)
TIME_ONLY_SIGMA = ((0.15, 0.15), (0.2, 0.2), (0.3, 0.3), (0.25, 0.25))


def rms_volatility(n_steps):
    rows = [lr.row_of(i, TIME_ONLY_GRID[0], n_steps) for i in range(n_steps)]
    return math.sqrt(sum(TIME_ONLY_SIGMA[k][0] ** 2 for k in rows) / n_steps)
