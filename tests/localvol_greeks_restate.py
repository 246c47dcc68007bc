"""numpy restatement of the local-volatility Greeks of include/mcamd.h (mcamd_price_localvol_greeks), used by
tests/test_gpu_localvol_greeks.py and tested against finite differences and closed forms in
tests/test_localvol_greeks_cpu.py.  Written from the header text: one numpy dtype throughout — float32, float64 or
longdouble — for the tables, the lookup, the step and the tangents; the samples are formed in float64 (longdouble when
the dtype is).  The path itself is walked with the very operations of tests/localvol_restate.py, so the price sample is
that module's, bit for bit.  numpy has no fused multiply-add: every fma of the header is a product and a sum here,
which is part of what the tolerances of the GPU test measure."""
import numpy as np

import localvol_restate as lv

CALL, PUT = lv.CALL, lv.PUT
N_EST = 6   # price, delta, gamma, vega, rho, rho_q
PRICE, DELTA, GAMMA, VEGA, RHO, RHO_Q = range(6)
NAMES = ("price", "delta", "gamma", "vega", "rho", "rho_q")


def bucket_of(step, n_buckets, n_steps):
    """the time bucket of step `step`: floor(step B / n_steps), in integers (the rule the rows use)"""
    return (int(step) * int(n_buckets)) // int(n_steps)


def lookup_slope(tabs, n_x, row, X):
    """(s, s') at X: the volatility localvol_restate.lookup gives, and slope_k (1 / dx) strictly inside the axis, else 0"""
    sig, slope, x_min, inv_dx = tabs
    f = sig.dtype.type
    with np.errstate(invalid="ignore"):
        u_raw = (X - x_min) * inv_dx
        u = np.minimum(np.maximum(u_raw, f(0)), f(n_x - 1))
        k = np.minimum(np.floor(u).astype(np.int64), n_x - 2)
        frac = u - k.astype(sig.dtype)
        s = frac * slope[row][k] + sig[row][k]
        inside = (u_raw > f(0)) & (u_raw < f(n_x - 1))   # a NaN compares false
    return s, np.where(inside, slope[row][k] * inv_dx, f(0))


def walk(z, T, r, q, grid, sigma, n_buckets=0, x0=0.0, dtype=np.float64, tangents=True):
    """z: [n_steps, n_paths] normals.  One walk from X_0 = x0: dict of X (final), J, U, R ([n]) and Ub ([B, n])."""
    dt_ = np.dtype(dtype)
    n_steps, n = z.shape
    n_t, n_x = grid[0], grid[1]
    f = dt_.type
    z = z.astype(dt_)
    tabs = lv.tables(grid, sigma, dt_)
    dt = f(T) / f(n_steps)
    sqrt_dt = np.sqrt(dt)
    mu = f(r) - f(q)
    X = np.full(n, f(x0), dtype=dt_)
    J = np.ones(n, dtype=dt_)
    U = np.zeros(n, dtype=dt_)
    R = np.zeros(n, dtype=dt_)
    Ub = np.zeros((n_buckets, n), dtype=dt_)
    for i in range(n_steps):
        row = lv.row_of(i, n_t, n_steps)
        if tangents:
            s, sp = lookup_slope(tabs, n_x, row, X)
            c = sqrt_dt * z[i] - s * dt
            g = sp * c + f(1)
            J = J * g
            U = U * g + c
            R = R * g + dt
            if n_buckets:
                cur = bucket_of(i, n_buckets, n_steps)
                for b in range(cur):
                    Ub[b] = Ub[b] * g
                Ub[cur] = Ub[cur] * g + c
        else:
            s = lv.lookup(tabs, n_x, row, X)
        X = X + ((mu - s * s / f(2)) * dt + (s * sqrt_dt) * z[i])
    return dict(X=X, J=J, U=U, R=R, Ub=Ub)


def wide_of(dtype):
    return np.longdouble if np.dtype(dtype) == np.dtype(np.longdouble) else np.float64


def path_end(X, S0, K, payoff, dtype):
    """(y, m, S_T): the price sample and omega 1{omega (S_T - K) > 0} S_T in the wide type, S_T in the path dtype"""
    f = np.dtype(dtype).type
    wide = wide_of(dtype)
    S_T = f(S0) * np.exp(X)
    h = np.maximum(f(K) - S_T, f(0)) if payoff == PUT else np.maximum(S_T - f(K), f(0))
    omega = wide(-1) if payoff == PUT else wide(1)
    return h.astype(wide), np.where(h > f(0), omega * S_T.astype(wide), wide(0)), S_T


def form(main, S0, K, T, payoff, dtype, up=None, down=None, gamma_bump=0.0):
    """The samples of one option on walks already made: dict with q ([6 + B, n] in the wide type), y, S_T, and margin
    (each path's smallest |S_T / K - 1| over the main walk, and margin3 over its one or three walks)."""
    wide = wide_of(dtype)
    f = np.dtype(dtype).type
    y, m, S_T = path_end(main["X"], S0, K, payoff, dtype)
    n_b = main["Ub"].shape[0]
    q = np.zeros((N_EST + n_b, y.size), dtype=wide)
    mR = m * main["R"].astype(wide)
    q[PRICE] = y
    q[DELTA] = m * main["J"].astype(wide) / wide(S0)
    q[VEGA] = m * main["U"].astype(wide)
    q[RHO] = mR - wide(T) * y
    q[RHO_Q] = -mR
    for b in range(n_b):
        q[N_EST + b] = m * main["Ub"][b].astype(wide)
    margin = np.abs(S_T.astype(np.float64) / K - 1.0)
    margin3 = margin
    if up is not None:
        eta = wide(f(gamma_bump))
        S_up, S_dn = wide(S0) * np.exp(eta), wide(S0) * np.exp(-eta)
        _, m_up, St_up = path_end(up["X"], S0, K, payoff, dtype)
        _, m_dn, St_dn = path_end(down["X"], S0, K, payoff, dtype)
        d_up = m_up * up["J"].astype(wide) / S_up
        d_dn = m_dn * down["J"].astype(wide) / S_dn
        q[GAMMA] = (d_up - d_dn) / (S_up - S_dn)
        for St in (St_up, St_dn):
            margin3 = np.minimum(margin3, np.abs(St.astype(np.float64) / K - 1.0))
    return dict(q=q, y=y, S_T=S_T, J=main["J"], U=main["U"], R=main["R"], Ub=main["Ub"], margin=margin, margin3=margin3)


def walks(z, T, r, q, grid, sigma, n_buckets=0, gamma_bump=0.0, dtype=np.float64):
    """(main, up, down): the walk from X_0 = 0 and, with gamma_bump > 0, those from +-eta on the same normals"""
    main = walk(z, T, r, q, grid, sigma, n_buckets, 0.0, dtype)
    if not gamma_bump > 0.0:
        return main, None, None
    eta = np.dtype(dtype).type(gamma_bump)
    return main, walk(z, T, r, q, grid, sigma, 0, eta, dtype), walk(z, T, r, q, grid, sigma, 0, -eta, dtype)


def samples(z, S0, K, T, r, q, grid, sigma, payoff, n_buckets=0, gamma_bump=0.0, dtype=np.float64):
    main, up, down = walks(z, T, r, q, grid, sigma, n_buckets, gamma_bump, dtype)
    return form(main, S0, K, T, payoff, dtype, up, down, gamma_bump)


def price_samples(z, S0, K, T, r, q, grid, sigma, payoff, x0=0.0, dtype=np.float64):
    """h(S_T) of the walk from X_0 = x0 with no tangents: what a bump-and-reprice run evaluates"""
    return path_end(walk(z, T, r, q, grid, sigma, 0, x0, dtype, tangents=False)["X"], S0, K, payoff, dtype)[0]
