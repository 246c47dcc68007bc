"""numpy restatement of the Heston cliquet definitions of include/mcamd.h (mcamd_price_heston_cliquet), used by
tests/test_gpu_heston_cliquet.py and tests/test_heston_cliquet_cpu.py.  Written from the header text: the step and the
draws are heston_restate's (the same lines, the same grouping, the same two normal streams), the period rule is
cliquet_restate's.  One numpy dtype throughout — float32, float64 or longdouble — for the step, the period log-returns,
the local clip and the accumulated A; sqrt(1 - rho^2), the two logarithms of the compounding form and the variance
factor 1 / (P tau) are formed in float64 as the host forms them; the sample y, the global clip, the counter flags and
the factor 1 / n of the average variance are formed in float64 (longdouble when the dtype is)."""
import numpy as np

from cliquet_restate import COMPOUND, INF, KINDS, SUM, VARIANCE   # noqa: F401  (the kinds, for the users of this file)


def samples(z, zv, T, r, heston_params, kind, reset_every, first_period=1, local_floor=-INF, local_cap=INF,
            global_floor=-INF, global_cap=INF, dtype=np.float64):
    """z, zv: [n_steps, n_paths] normals of the log-price and of the variance.  heston_params = (q, v0, kappa, theta,
    xi, rho).  Returns a dict: y (float64 samples, or longdouble when dtype is), A (the value that is clipped, same
    type as y), floored and capped (the per-path counter flags), D (the period log-returns, [M, n_paths], of the
    dtype), X and v_n (the final log-price and raw variance, of the dtype), trunc (steps each path entered with v < 0),
    rv (the path's average variance, same type as y), min_abs_v (smallest |v_i| over the steps entered, float64)."""
    q, v0, kappa, theta, xi, rho = heston_params
    dt_ = np.dtype(dtype)
    n_steps, n = z.shape
    assert zv.shape == z.shape
    assert reset_every >= 1 and n_steps % reset_every == 0
    M = n_steps // reset_every
    assert 1 <= first_period <= M
    f = dt_.type
    wide = np.longdouble if dt_ == np.dtype(np.longdouble) else np.float64
    z, zv = z.astype(dt_), zv.astype(dt_)
    dt = f(T) / f(n_steps)
    sqrt_dt = np.sqrt(dt)
    mu = f(r) - f(q)
    rho_c = f(np.sqrt(np.float64(1.0) - np.float64(rho) * np.float64(rho)))
    rho, kappa, theta, xi = f(rho), f(kappa), f(theta), f(xi)
    if kind == COMPOUND:
        with np.errstate(divide="ignore"):
            lo, hi = f(np.log(np.float64(1.0) + np.float64(local_floor))), f(np.log(np.float64(1.0) + np.float64(local_cap)))
    else:
        lo, hi = f(local_floor), f(local_cap)
    X = np.zeros(n, dtype=dt_)
    v = np.full(n, f(v0), dtype=dt_)
    v_sum = np.zeros(n, dtype=dt_)
    trunc = np.zeros(n, dtype=np.int64)
    min_abs_v = np.full(n, np.inf)
    X_reset = np.zeros(n, dtype=dt_)
    acc = np.zeros(n, dtype=dt_)
    D_all = np.empty((M, n), dtype=dt_)
    for i in range(n_steps):
        # heston_restate's step
        trunc += v < f(0)
        min_abs_v = np.minimum(min_abs_v, np.abs(v).astype(np.float64))
        vp = np.maximum(v, f(0))
        s = np.sqrt(vp)
        w = rho * z[i] + rho_c * zv[i]
        X = X + ((mu - vp / f(2)) * dt + (s * sqrt_dt) * z[i])
        v = v + (kappa * (theta - vp) * dt + (xi * s * sqrt_dt) * w)
        v_sum = v_sum + vp
        # cliquet_restate's period rule
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
    return dict(y=y, A=A, floored=floored, capped=capped, D=D_all, X=X, v_n=v, trunc=trunc,
                rv=v_sum.astype(wide) * (wide(1) / wide(n_steps)), min_abs_v=min_abs_v)


def price_f64(seed, n_paths, n_steps, T, r, heston_params, kind, reset_every, first_period=1, local_floor=-INF,
              local_cap=INF, chunk=125_000):
    """(discounted mean, its standard error) of the float64 restatement over the paths 0..n_paths-1 under seed, on
    heston_restate's vectorised Philox draws, a chunk of paths at a time"""
    from heston_restate import VARIANCE_BLOCKS, philox_normals_f64
    total = total_sq = 0.0
    for first in range(0, n_paths, chunk):
        m = min(chunk, n_paths - first)
        z = philox_normals_f64(seed, first, m, n_steps)
        zv = philox_normals_f64(seed, first, m, n_steps, VARIANCE_BLOCKS)
        y = samples(z, zv, T, r, heston_params, kind, reset_every, first_period, local_floor, local_cap)["y"]
        total += float(y.sum())
        total_sq += float((y * y).sum())
    mean = total / n_paths
    var = max(total_sq / n_paths - mean * mean, 0.0) * n_paths / (n_paths - 1)
    disc = float(np.exp(-r * T))
    return disc * mean, disc * float(np.sqrt(var / n_paths))
