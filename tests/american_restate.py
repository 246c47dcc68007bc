"""numpy restatement of the least-squares Monte Carlo definitions of include/mcamd.h (mcamd_price_american), used by
tests/test_gpu_american.py, and a Cox-Ross-Rubinstein tree that exercises at the same dates."""
import math

import numpy as np


def dates(T, r, n_steps, k):
    """M, t_j and d_j = exp(-r t_j) of dates j = 1..M (index j - 1), as the engine forms them"""
    M = n_steps // k
    dt = T / n_steps
    t = np.array([float(j * k) * dt for j in range(1, M + 1)])
    return M, t, np.exp(-r * t)


def payoff(S, K, put):
    return np.maximum(K - S, 0.0) if put else np.maximum(S - K, 0.0)


def basis(S, K, m):
    return np.vander(S / K - 1.0, m, increasing=True)


def fit(S, V, K, m):
    """(regressed, beta) of one date from its in-the-money points: normal equations, Jacobi-scaled, pivot rule"""
    if len(S) < 4 * m:
        return False, None
    X = basis(S, K, m)
    A = X.T @ X
    D = 1.0 / np.sqrt(np.diag(A))
    As = A * D[:, None] * D[None, :]
    L = np.zeros_like(As)
    for c in range(m):   # Cholesky with the pivots exposed
        s = As[c, c] - L[c, :c] @ L[c, :c]
        if not s > 1e-12:
            return False, None
        L[c, c] = math.sqrt(s)
        for r_ in range(c + 1, m):
            L[r_, c] = (As[r_, c] - L[r_, :c] @ L[c, :c]) / L[c, c]
    beta, *_ = np.linalg.lstsq(X * D[None, :], V, rcond=None)
    return True, beta * D


def sweep(rows, K, put, k, m, disc, beta_gpu, flags_gpu):
    """The backward sweep on stored rows [n_steps, n] (float64), deciding with the engine's coefficients.
    Returns V and, per date j = M-1..1, (j, regressed, in-the-money mask, numpy continuation, engine continuation)."""
    M = len(disc)
    V = disc[M - 1] * payoff(rows[M * k - 1], K, put)
    out = []
    for j in range(M - 1, 0, -1):
        S = rows[j * k - 1]
        h = payoff(S, K, put)
        itm = h > 0
        ok, beta = fit(S[itm], V[itm], K, m)
        X = basis(S[itm], K, m)
        c_np = X @ beta if ok else None
        c_gpu = X @ beta_gpu[j - 1] if flags_gpu[j - 1] else None
        out.append((j, ok, itm, c_np, c_gpu))
        if flags_gpu[j - 1]:
            ex = disc[j - 1] * h[itm] > c_gpu
            idx = np.flatnonzero(itm)[ex]
            V[idx] = disc[j - 1] * h[idx]
    return V, out


def forward(rows, K, put, k, m, disc, t, beta_gpu, flags_gpu):
    """The pricing rule applied forward on rows [n_steps, n]: samples, date of early exercise (0: none), exercise
    time, and the smallest relative distance of a decision to its boundary"""
    M = len(disc)
    n = rows.shape[1]
    y = np.zeros(n)
    ex_date = np.zeros(n, dtype=np.int64)
    live = np.ones(n, dtype=bool)
    margin = np.inf
    for j in range(1, M):
        if not flags_gpu[j - 1]:
            continue
        S = rows[j * k - 1]
        h = payoff(S, K, put)
        cand = live & (h > 0)
        e = disc[j - 1] * h[cand]
        c = basis(S[cand], K, m) @ beta_gpu[j - 1]
        if e.size:
            margin = min(margin, float(np.min(np.abs(e - c) / np.maximum(np.abs(e), 1e-300))))
        go = np.flatnonzero(cand)[e > c]
        y[go] = disc[j - 1] * h[go]
        ex_date[go] = j
        live[go] = False
    y[live] = disc[M - 1] * payoff(rows[M * k - 1, live], K, put)
    t_ex = np.where(ex_date > 0, t[np.maximum(ex_date - 1, 0)], 0.0)
    return y, ex_date, t_ex, margin


def crr_bermudan(S0, K, r, v, T, n_dates, per_date=200, put=True):
    """Bermudan option on a Cox-Ross-Rubinstein tree that may be exercised at t = 0 and at the n_dates equally spaced
    dates only (per_date tree steps between dates)"""
    N = n_dates * per_date
    dt = T / N
    u = math.exp(v * math.sqrt(dt))
    d = 1.0 / u
    p = (math.exp(r * dt) - d) / (u - d)
    disc = math.exp(-r * dt)
    a, b = disc * p, disc * (1.0 - p)
    S = S0 * u ** (N - 2.0 * np.arange(N + 1))
    V = payoff(S, K, put)
    for i in range(N - 1, -1, -1):
        V = a * V[:-1] + b * V[1:]
        if i % per_date == 0:
            V = np.maximum(V, payoff(S0 * u ** (i - 2.0 * np.arange(i + 1)), K, put))
    return float(V[0])
