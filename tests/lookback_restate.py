"""numpy restatement of the lookback definitions of include/mcamd.h (mcamd_price_lookback), used by
tests/test_gpu_lookback.py and tested against itself and the host closed form in tests/test_lookback_cpu.py.

Two independent things live here:
  * samples(): the estimator, given a matrix of normals and one of uniforms, in one numpy dtype throughout — float64,
    longdouble or float32 (the sample itself is formed in float64 from the path-precision S_T and S_E, as the kernel
    does);
  * closed_form(): the four continuously monitored prices by quadrature of the payoff against the law of the running
    maximum of a drifted Brownian motion (reflection principle), written without reference to the C code (which
    evaluates the Goldman-Sosin-Gatto and Conze-Viswanathan formulas)."""
import math

import numpy as np

FLOATING, FIXED = 0, 1
CALL, PUT = 0, 1
DISCRETE, CONTINUOUS = 0, 1
PRODUCTS = ((FLOATING, CALL), (FLOATING, PUT), (FIXED, CALL), (FIXED, PUT))
Q_CUT = {np.dtype(np.float64): 36.75, np.dtype(np.longdouble): 36.75, np.dtype(np.float32): 22.25}


def wants_maximum(strike, payoff):
    """floating put and fixed call look at the maximum, floating call and fixed put at the minimum"""
    return (payoff == CALL) if strike == FIXED else (payoff == PUT)


def samples(z, u, S0, K, T, r, v, strike, payoff, monitoring, dtype=np.float64, q_cut=None):
    """z: [n_steps, n_paths] normals; u: [n_steps, n_paths] uniforms in (0, 1] (unused, and may be None, for discrete
    monitoring).  q_cut: Q, by default the dtype's own (to restate an fp32 kernel in float64, pass the fp32 Q).
    Returns a dict: y (float64 samples, or longdouble when dtype is), S_T, S_E, X, E, live (the steps of
    each path that formed a bridge extremum, i.e. had q < Q) and dropped (the steps with q >= Q whose bridge extremum
    would nevertheless have moved E: the Q rule says there are none)."""
    dt_ = np.dtype(dtype)
    n_steps, n = z.shape
    f = dt_.type
    z = z.astype(dt_)
    dt = f(T) / f(n_steps)
    drift = (f(r) - f(v) * f(v) / f(2)) * dt
    vol = f(v) * np.sqrt(dt)
    v2dt = f(v) * f(v) * dt
    q_cut = f(Q_CUT[dt_] if q_cut is None else q_cut)
    top = wants_maximum(strike, payoff)
    X = np.zeros(n, dtype=dt_)
    E = np.zeros(n, dtype=dt_)
    live = np.zeros(n, dtype=np.int64)
    dropped = np.zeros(n, dtype=np.int64)
    for i in range(n_steps):
        x = drift + vol * z[i]
        X_prev = X
        X = X + x
        E = np.maximum(E, X) if top else np.minimum(E, X)
        if monitoring == CONTINUOUS:
            U = u[i].astype(dt_)
            d_prev, d = (E - X_prev, E - X) if top else (X_prev - E, X - E)
            q = f(2) * d_prev * d / v2dt
            take = q < q_cut
            root = np.sqrt(x * x - f(2) * v2dt * np.log(U))
            ends = X_prev + X
            mid = f(0.5) * (ends + root if top else ends - root)
            moved = (mid > E) if top else (mid < E)
            dropped += ~take & moved
            live += take
            E = np.where(take, np.maximum(E, mid) if top else np.minimum(E, mid), E)
    S_T = f(S0) * np.exp(X)
    S_E = f(S0) * np.exp(E)
    S_E = np.where(E == X, S_T, S_E)   # one exponential routine: equal exponents give equal prices
    wide = np.longdouble if dt_ == np.dtype(np.longdouble) else np.float64
    st, se = S_T.astype(wide), S_E.astype(wide)
    if strike == FIXED:
        y = np.maximum(wide(K) - se if payoff == PUT else se - wide(K), wide(0))
    else:
        y = se - st if payoff == PUT else st - se
    return dict(y=y, S_T=S_T, S_E=S_E, X=X, E=E, live=live, dropped=dropped)


# ---- closed forms ----------------------------------------------------------------------------------------------------

def _N(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def _p_max_beyond(m, mu, v, T):
    """P[max_{t <= T} (mu t + v W_t) > m], m >= 0 (reflection principle with drift)"""
    s = v * math.sqrt(T)
    return _N((mu * T - m) / s) + math.exp(2.0 * mu * m / (v * v)) * _N((-m - mu * T) / s)


_GL_X, _GL_W = np.polynomial.legendre.leggauss(16)


def _tail_integral(lo, sign, mu, v, T, panels=96):
    """int_lo^inf e^{sign m} P[max > m] dm by composite Gauss-Legendre; the integrand is analytic on m > 0 and below
    1e-40 of its peak beyond the upper limit used"""
    s = v * math.sqrt(T)
    hi = lo + abs(mu) * T + s * s + 14.0 * s
    edges = np.linspace(lo, hi, panels + 1)
    total = 0.0
    for a, b in zip(edges[:-1], edges[1:]):
        h, c = 0.5 * (b - a), 0.5 * (a + b)
        total += h * sum(w * math.exp(sign * (c + h * x)) * _p_max_beyond(c + h * x, mu, v, T)
                         for x, w in zip(_GL_X, _GL_W))
    return total


def closed_form(S0, K, T, r, v, strike, payoff):
    """Continuously monitored, newly issued lookback, no dividends.  With M the maximum of X_t = mu t + v W_t,
    mu = r - v^2/2:  (S0 e^M - K)+ = int_k^inf S0 e^m 1{M > m} dm for k = ln(K / S0) >= 0, so its expectation is
    S0 int_k^inf e^m P[M > m] dm, and E[e^M] = 1 + int_0^inf e^m P[M > m] dm.  The minimum of X is minus the maximum
    of -X, whose drift is -mu."""
    mu, D = r - 0.5 * v * v, math.exp(-r * T)
    if wants_maximum(strike, payoff):
        if strike == FIXED and K > S0:
            return D * S0 * _tail_integral(math.log(K / S0), +1.0, mu, v, T)
        mean_max = S0 * (1.0 + _tail_integral(0.0, +1.0, mu, v, T))            # E[S_max]
        return D * (mean_max - (K if strike == FIXED else S0 * math.exp(r * T)))
    if strike == FIXED and K < S0:
        return D * S0 * _tail_integral(math.log(S0 / K), -1.0, -mu, v, T)
    mean_min = S0 * (1.0 - _tail_integral(0.0, -1.0, -mu, v, T))               # E[S_min]
    return D * ((K if strike == FIXED else S0 * math.exp(r * T)) - mean_min)
