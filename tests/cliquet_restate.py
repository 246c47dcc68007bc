"""numpy restatement of the cliquet definitions of include/mcamd.h (mcamd_price_cliquet), used by
tests/test_gpu_cliquet.py and tests/test_cliquet_cpu.py.  Written from the header text: one numpy dtype throughout —
float32, float64 or longdouble — for the tables, the lookup, the step, the period log-returns, the local clip and the
accumulated A; the two logarithms of the compounding form and the variance factor 1 / (P tau) are formed in float64 as
the host forms them; the sample y, the global clip and the counter flags are formed in float64 (longdouble when the
dtype is).  The walk is localvol_restate's: the same tables, lookup, slice rule and step."""
import numpy as np

from localvol_restate import lookup, row_of, tables

SUM, COMPOUND, VARIANCE = 0, 1, 2
KINDS = (SUM, COMPOUND, VARIANCE)
INF = float("inf")


def samples(z, T, r, q, grid, sigma, kind, reset_every, first_period=1, local_floor=-INF, local_cap=INF,
            global_floor=-INF, global_cap=INF, dtype=np.float64):
    """z: [n_steps, n_paths] normals.  Returns a dict: y (float64 samples, or longdouble when dtype is), A (the value
    that is clipped, same type as y), floored and capped (the per-path counter flags), D (the period log-returns,
    [M, n_paths], of the dtype)."""
    dt_ = np.dtype(dtype)
    n_steps, n = z.shape
    assert reset_every >= 1 and n_steps % reset_every == 0
    M = n_steps // reset_every
    assert 1 <= first_period <= M
    n_t, n_x = grid[0], grid[1]
    f = dt_.type
    wide = np.longdouble if dt_ == np.dtype(np.longdouble) else np.float64
    z = z.astype(dt_)
    tabs = tables(grid, sigma, dt_)
    dt = f(T) / f(n_steps)
    sqrt_dt = np.sqrt(dt)
    mu = f(r) - f(q)
    if kind == COMPOUND:
        with np.errstate(divide="ignore"):
            lo, hi = f(np.log(np.float64(1.0) + np.float64(local_floor))), f(np.log(np.float64(1.0) + np.float64(local_cap)))
    else:
        lo, hi = f(local_floor), f(local_cap)
    X = np.zeros(n, dtype=dt_)
    X_reset = np.zeros(n, dtype=dt_)
    acc = np.zeros(n, dtype=dt_)
    D_all = np.empty((M, n), dtype=dt_)
    for i in range(n_steps):
        s = lookup(tabs, n_x, row_of(i, n_t, n_steps), X)
        X = X + ((mu - s * s / f(2)) * dt + (s * sqrt_dt) * z[i])
        if (i + 1) % reset_every:
            continue
        p = (i + 1) // reset_every
        D = X - X_reset
        X_reset = X
        D_all[p - 1] = D
        if p < first_period:
            continue
        if kind == SUM:
            acc = acc + np.minimum(np.maximum(np.exp(D) - f(1), lo), hi)
        elif kind == COMPOUND:
            acc = acc + np.minimum(np.maximum(D, lo), hi)
        else:
            acc = acc + D * D
    if kind == SUM:
        A = acc.astype(wide)
    elif kind == COMPOUND:
        A = np.exp(acc).astype(wide) - wide(1)
    else:
        P = M - first_period + 1
        scale = np.float64(1.0) / (np.float64(P) * (np.float64(reset_every) * (np.float64(T) / np.float64(n_steps))))
        A = acc.astype(wide) * wide(scale)
    y = np.minimum(np.maximum(A, wide(global_floor)), wide(global_cap))
    floored = (A <= wide(global_floor)) if global_floor > -INF else np.zeros(n, dtype=bool)
    capped = (A >= wide(global_cap)) if global_cap < INF else np.zeros(n, dtype=bool)
    return dict(y=y, A=A, floored=floored, capped=capped, D=D_all)
