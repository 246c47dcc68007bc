"""numpy restatement of the dual (upper) bound definitions of include/mcamd.h (mcamd_american_upper_bound), used by
tests/test_gpu_american_dual.py and tested against itself in tests/test_american_dual_cpu.py.

Decisions go through american_restate.decide: the vectorised comparison decides where exercise value and fitted
continuation value are further apart than rounding can bridge, and every case closer than that is handed to decide,
which emulates the device's fused multiply-adds exactly."""
import math

import numpy as np

import american_restate as ar

CLOSE = 1e-9   # relative distance below which a decision is taken by ar.decide instead of plain numpy


def align(x):
    return (x + 255) // 256 * 256


def workspace_formula(n_local, n_steps, k, prec_bits):
    """include/mcamd.h, mcamd_american_dual_workspace_bytes, restated"""
    M = n_steps // k
    elem = 4 if prec_bits == 32 else 8
    per_thread = 4 if prec_bits == 32 else 2
    groups = -(-n_local // per_thread)
    g_store = min(max(-(-groups // 256), 1), 1 << 20)
    g_cont = min(max(M * n_local, 1), 8192)
    g_scan = min(max(-(-n_local // 256), 1), 8192)
    return (256 + align(n_steps * n_local * elem) + align(8 * M * n_local) + align(8 * 8 * (M + 1))
            + align(8 * max(2 * g_store, 2 * g_cont, 4 * g_scan)))


def subsequence_base(g, j, M, n_inner):
    """Philox subsequence of continuation path 0 of point (global outer path g, date j)"""
    return (g * M + j) * n_inner


def decide_vec(beta, disc, K, put, S):
    """e (the rule says stop) for the prices S at one regressed date"""
    S = np.asarray(S, dtype=np.float64)
    h = ar.payoff(S, K, put)
    e = disc * h
    u = S / K - 1.0
    c = np.full_like(S, float(beta[-1]))
    for b in beta[-2::-1]:
        c = c * u + float(b)
    out = (h > 0) & (e > c)
    close = (h > 0) & (np.abs(e - c) <= CLOSE * np.maximum(np.abs(e), np.abs(c)))
    for i in np.flatnonzero(close):
        out[i] = ar.decide([float(b) for b in beta], disc, K, put, S[i])[0]
    return out


def follow(rows, j0, K, put, k, disc, beta, flags):
    """Samples of paths that start at date j0 and follow the rule: rows [(M - j0) k, n] holds the prices after each
    remaining step (row (i - j0) k - 1 is date i).  Returns (y, stop date of each path)."""
    M = len(disc)
    n = rows.shape[1]
    y = np.zeros(n)
    stop = np.full(n, M, dtype=np.int64)
    live = np.ones(n, dtype=bool)
    for i in range(j0 + 1, M):
        if not flags[i - 1]:
            continue
        S = rows[(i - j0) * k - 1]
        go = live & decide_vec(beta[i - 1], disc[i - 1], K, put, S)
        y[go] = disc[i - 1] * ar.payoff(S[go], K, put)
        stop[go] = i
        live[go] = False
    y[live] = disc[M - 1] * ar.payoff(rows[(M - j0) * k - 1, live], K, put)
    return y, stop


def scan(rows, Q, K, put, k, disc, beta, flags):
    """The dual samples u_p of outer paths rows [n_steps, n] given continuation values Q [M, n] (Q[j] of date j,
    j = 0..M-1): pi_0 = 0, pi_j = pi_{j-1} + L_j - Q_{j-1}, u = max_j (Z_j - pi_j), the term of a date where the rule
    says stop formed as Q_{j-1} - pi_{j-1} (its value), as the engine forms it."""
    M = len(disc)
    n = rows.shape[1]
    pi = np.zeros(n)
    u = np.full(n, -np.inf)
    q_prev = np.asarray(Q[0], dtype=np.float64).copy()
    for j in range(1, M + 1):
        S = rows[j * k - 1]
        Z = disc[j - 1] * ar.payoff(S, K, put)
        if j == M:
            e = np.ones(n, dtype=bool)
            q_j = np.zeros(n)
        else:
            q_j = np.asarray(Q[j], dtype=np.float64)
            e = decide_vec(beta[j - 1], disc[j - 1], K, put, S) if flags[j - 1] else np.zeros(n, dtype=bool)
        cand_stop = q_prev - pi
        pi = np.where(e, pi + (Z - q_prev), pi + (q_j - q_prev))
        cand = np.where(e, cand_stop, Z - pi)
        u = np.maximum(u, cand)
        q_prev = q_j
    return u


def bs_put(S, K, r, v, tau):
    """European put on GBM, value at the start of the remaining time tau (not discounted further)"""
    S = np.asarray(S, dtype=np.float64)
    erfc = np.vectorize(math.erfc)
    sq = v * math.sqrt(tau)
    d1 = (np.log(S / K) + (r + 0.5 * v * v) * tau) / sq
    d2 = d1 - sq
    return K * math.exp(-r * tau) * 0.5 * erfc(d2 / math.sqrt(2.0)) - S * 0.5 * erfc(d1 / math.sqrt(2.0))
