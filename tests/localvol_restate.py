"""numpy restatement of the local-volatility definitions of include/mcamd.h (mcamd_price_localvol), used by
tests/test_gpu_localvol.py and tested against the barrier restatement, the host lookup and closed forms in
tests/test_localvol_cpu.py.  Written from the header text: one numpy dtype throughout — float32, float64 or longdouble
— for the tables, the lookup, the step, the barrier distances and the bridge factors; the sample itself is formed in
float64 (longdouble when the dtype is) from the path-precision w and h, as the header says."""
import numpy as np

NO_BARRIER = -1
DOWN_OUT, DOWN_IN, UP_OUT, UP_IN = 0, 1, 2, 3
CALL, PUT = 0, 1
DISCRETE, CONTINUOUS = 0, 1
KINDS = (DOWN_OUT, DOWN_IN, UP_OUT, UP_IN)
Q_CUT = {np.dtype(np.float64): 38.0, np.dtype(np.longdouble): 38.0, np.dtype(np.float32): 18.0}


def is_up(kind):
    return kind in (UP_OUT, UP_IN)


def is_out(kind):
    return kind in (DOWN_OUT, UP_OUT)


def row_of(step, n_t, n_steps):
    """the slice step `step` of n_steps uses: floor(step n_t / n_steps), in integers"""
    return (int(step) * int(n_t)) // int(n_steps)


def tables(grid, sigma, dtype):
    """grid = (n_t, n_x, x_min, x_max), sigma: n_t rows of n_x.  Returns (sigma_k, slope_k, x_min, 1 / dx) narrowed to
    dtype; the slopes and 1 / dx are formed in float64 first."""
    n_t, n_x, x_min, x_max = grid
    f = np.dtype(dtype).type
    s = np.asarray(sigma, dtype=np.float64).reshape(n_t, n_x)
    slope = np.zeros_like(s)
    slope[:, :-1] = s[:, 1:] - s[:, :-1]
    dx = (np.float64(x_max) - np.float64(x_min)) / np.float64(n_x - 1)
    return s.astype(dtype), slope.astype(dtype), f(np.float64(x_min)), f(np.float64(1.0) / dx)


def lookup(tabs, n_x, row, X):
    """sigma(row, X) for an array X of the tables' dtype"""
    sig, slope, x_min, inv_dx = tabs
    f = sig.dtype.type
    u = np.minimum(np.maximum((X - x_min) * inv_dx, f(0)), f(n_x - 1))
    k = np.minimum(np.floor(u).astype(np.int64), n_x - 2)
    frac = u - k.astype(sig.dtype)
    return frac * slope[row][k] + sig[row][k]


def sigma_at(grid, sigma, n_steps, step, x, dtype=np.float64):
    """what mcamd_localvol_sigma_f64 returns, from the definition"""
    tabs = tables(grid, sigma, dtype)
    X = np.asarray([x], dtype=dtype)
    return lookup(tabs, grid[1], row_of(step, grid[0], n_steps), X)[0]


def samples(z, S0, K, B, T, r, q, grid, sigma, barrier, payoff, monitoring, dtype=np.float64):
    """z: [n_steps, n_paths] normals.  Returns a dict: y (float64 samples, or longdouble when dtype is), w, S_T, h,
    min_abs_d (smallest |d_i| over the step ends, float64; inf without a barrier), live (steps each path entered not
    yet knocked)."""
    dt_ = np.dtype(dtype)
    n_steps, n = z.shape
    n_t, n_x = grid[0], grid[1]
    f = dt_.type
    z = z.astype(dt_)
    tabs = tables(grid, sigma, dt_)
    dt = f(T) / f(n_steps)
    sqrt_dt = np.sqrt(dt)
    mu = f(r) - f(q)
    has_barrier = barrier != NO_BARRIER
    up = has_barrier and is_up(barrier)
    b = np.log(f(B) / f(S0)) if has_barrier else f(0)
    q_cut = f(Q_CUT[dt_])
    X = np.zeros(n, dtype=dt_)
    d_prev = np.full(n, abs(b), dtype=dt_)
    w = np.ones(n, dtype=dt_)
    alive = np.ones(n, dtype=bool)
    live = np.zeros(n, dtype=np.int64)
    min_abs_d = np.full(n, np.inf)
    for i in range(n_steps):
        live += alive
        s = lookup(tabs, n_x, row_of(i, n_t, n_steps), X)
        X = X + ((mu - s * s / f(2)) * dt + (s * sqrt_dt) * z[i])
        if not has_barrier:
            continue
        hit = (X > b) if up else (b > X)
        d = (b - X) if up else (X - b)
        alive &= ~hit
        min_abs_d = np.minimum(min_abs_d, np.abs(d).astype(np.float64))
        if monitoring == CONTINUOUS:
            qi = f(2) * d_prev * d / (s * s * dt)
            take = alive & (qi < q_cut)            # f_i is exactly 1 elsewhere: part of the definition
            with np.errstate(over="ignore", invalid="ignore"):
                fac = f(1) - np.exp(-qi)
            w = np.where(take, w * fac, w)
            d_prev = d
    w = np.where(alive, w, f(0))
    S_T = f(S0) * np.exp(X)
    h = np.maximum(f(K) - S_T, f(0)) if payoff == PUT else np.maximum(S_T - f(K), f(0))
    wide = np.longdouble if dt_ == np.dtype(np.longdouble) else np.float64
    ww, hh = w.astype(wide), h.astype(wide)
    if not has_barrier:
        y = hh
    else:
        y = ww * hh if is_out(barrier) else (wide(1) - ww) * hh
    return dict(y=y, w=w, S_T=S_T, h=h, min_abs_d=min_abs_d, live=live)
