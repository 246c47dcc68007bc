"""numpy restatement of the single-barrier definitions of include/mcamd.h (mcamd_price_barrier), used by
tests/test_gpu_barrier.py and tested against itself and the host closed form in tests/test_barrier_cpu.py.

Two independent things live here:
  * samples(): the estimator, given a matrix of normals, in one numpy dtype throughout — float64, longdouble or
    float32 (the sample itself is formed in float64 from the path-precision w and h, as the kernel does);
  * closed_form(): the eight continuously monitored prices by the method of images on interval payoffs, written
    without reference to the C code (which combines the four Reiner-Rubinstein terms)."""
import math

import numpy as np

DOWN_OUT, DOWN_IN, UP_OUT, UP_IN = 0, 1, 2, 3
CALL, PUT = 0, 1
DISCRETE, CONTINUOUS = 0, 1
KINDS = (DOWN_OUT, DOWN_IN, UP_OUT, UP_IN)
Q_CUT = {np.dtype(np.float64): 38.0, np.dtype(np.longdouble): 38.0, np.dtype(np.float32): 18.0}


def is_up(kind):
    return kind in (UP_OUT, UP_IN)


def is_out(kind):
    return kind in (DOWN_OUT, UP_OUT)


def samples(z, S0, K, B, T, r, v, kind, payoff, monitoring, dtype=np.float64):
    """z: [n_steps, n_paths] normals.  Returns a dict: y (float64 samples, or longdouble when dtype is), w, S_T,
    min_abs_d (smallest |d_i| over the step ends, float64), live (steps each path entered not yet knocked)."""
    dt_ = np.dtype(dtype)
    n_steps, n = z.shape
    f = dt_.type
    z = z.astype(dt_)
    dt = f(T) / f(n_steps)
    drift = (f(r) - f(v) * f(v) / f(2)) * dt
    vol = f(v) * np.sqrt(dt)
    b = np.log(f(B) / f(S0))
    kq = f(2) / (f(v) * f(v) * dt)
    q_cut = f(Q_CUT[dt_])
    up = is_up(kind)
    X = np.zeros(n, dtype=dt_)
    d_prev = np.full(n, abs(b), dtype=dt_)
    w = np.ones(n, dtype=dt_)
    alive = np.ones(n, dtype=bool)
    live = np.zeros(n, dtype=np.int64)
    min_abs_d = np.full(n, np.inf)
    for i in range(n_steps):
        live += alive
        X = X + (drift + vol * z[i])
        hit = (X > b) if up else (b > X)
        d = (b - X) if up else (X - b)
        alive &= ~hit
        min_abs_d = np.minimum(min_abs_d, np.abs(d).astype(np.float64))
        if monitoring == CONTINUOUS:
            q = kq * d_prev * d
            take = alive & (q < q_cut)            # f_i is exactly 1 elsewhere: part of the definition
            with np.errstate(over="ignore", invalid="ignore"):
                fac = f(1) - np.exp(-q)
            w = np.where(take, w * fac, w)
            d_prev = d
    w = np.where(alive, w, f(0))
    S_T = f(S0) * np.exp(X)
    h = np.maximum(f(K) - S_T, f(0)) if payoff == PUT else np.maximum(S_T - f(K), f(0))
    wide = np.longdouble if dt_ == np.dtype(np.longdouble) else np.float64
    ww, hh = w.astype(wide), h.astype(wide)
    y = ww * hh if is_out(kind) else (wide(1) - ww) * hh
    return dict(y=y, w=w, S_T=S_T, h=h, min_abs_d=min_abs_d, live=live)


# ---- closed forms ----------------------------------------------------------------------------------------------------

def _N(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def _interval(s, K, lo, hi, T, r, v, payoff):
    """exp(-rT) E[h(S_T) 1{lo < S_T < hi}] for GBM from s; lo may be 0 and hi inf"""
    if payoff == CALL:
        lo = max(lo, K)
    else:
        hi = min(hi, K)
    if not lo < hi:
        return 0.0
    sd = v * math.sqrt(T)

    def tail(x):   # (P_S[S_T > x], P[S_T > x]) under the share and the risk-neutral measure
        if x <= 0.0:
            return 1.0, 1.0
        if math.isinf(x):
            return 0.0, 0.0
        d1 = (math.log(s / x) + (r + 0.5 * v * v) * T) / sd
        return _N(d1), _N(d1 - sd)
    a1, a2 = tail(lo)
    b1, b2 = tail(hi)
    val = s * (a1 - b1) - K * math.exp(-r * T) * (a2 - b2)
    return val if payoff == CALL else -val


def vanilla(S0, K, T, r, v, payoff):
    return _interval(S0, K, 0.0, math.inf, T, r, v, payoff)


def closed_form(S0, K, B, T, r, v, kind, payoff):
    """Continuously monitored single barrier, rebate 0, by the method of images: with g the payoff cut to the live
    side of B, out(S) = V_g(S) - (B / S)^(2r/v^2 - 1) V_g(B^2 / S), and in = vanilla - out.  For a down-call with
    K >= B and an up-put with K <= B the cut changes nothing and this is the reflection of the vanilla price."""
    lo, hi = (0.0, B) if is_up(kind) else (B, math.inf)
    out = (_interval(S0, K, lo, hi, T, r, v, payoff)
           - (B / S0) ** (2.0 * r / (v * v) - 1.0) * _interval(B * B / S0, K, lo, hi, T, r, v, payoff))
    return out if is_out(kind) else vanilla(S0, K, T, r, v, payoff) - out
