"""numpy restatement of the Asian-option definitions of include/mcamd.h (mcamd_price_asian), used by
tests/test_gpu_asian.py and tested against itself and the host closed form in tests/test_asian_cpu.py.

Three things live here:
  * samples(): the estimator, given a matrix of normals, with the path arithmetic in one numpy dtype — float64,
    longdouble or float32 — and the average, the sample and the sums in float64 (longdouble when the dtype is), as the
    kernel does;
  * closed_form(): the discrete geometric-average prices, written from the moments of the lognormal without reference
    to the C code;
  * RECORD: what tests/test_asian_cpu.py measured on the CPU and the GPU tests take their tolerances from.  The CPU test
    measures again and fails if a measurement is worse than its record."""
import math

import numpy as np

from deep_inputs import DEEP, SHALLOW

ARITHMETIC, GEOMETRIC = 0, 1
FIXED, FLOATING = 0, 1
CALL, PUT = 0, 1
PRODUCTS = tuple((strike, payoff, spot) for strike in (FIXED, FLOATING) for payoff in (CALL, PUT) for spot in (0, 1))


def payoff_of(avg, S_T, K, strike, payoff):
    """fixed: call (avg - K)+, put (K - avg)+; floating: call (S_T - avg)+, put (avg - S_T)+"""
    wide = avg.dtype.type
    if strike == FIXED:
        d = wide(K) - avg if payoff == PUT else avg - wide(K)
    else:
        d = avg - S_T if payoff == PUT else S_T - avg
    return np.maximum(d, wide(0))


def samples(z, S0, K, T, r, v, average, strike, payoff, include_spot, dtype=np.float64):
    """z: [n_steps, n_paths] normals.  Returns a dict: y (the sample of the job's average), g (the geometric sample of
    the same strike, payoff and include_spot: the control), A, G, S_T (the last product-form price, what the
    arithmetic sample uses) and S_T_log (S0 e^{X_n}, what the geometric sample uses)."""
    dt_ = np.dtype(dtype)
    f = dt_.type
    wide = np.longdouble if dt_ == np.dtype(np.longdouble) else np.float64
    n_steps, n = z.shape
    m = n_steps + (1 if include_spot else 0)
    z = z.astype(dt_)
    dt = f(T) / f(n_steps)
    drift = (f(r) - f(v) * f(v) / f(2)) * dt
    vol = f(v) * np.sqrt(dt)
    P = np.full(n, f(S0), dtype=dt_)
    sum_p = np.full(n, wide(S0) if include_spot else wide(0), dtype=wide)
    X = np.zeros(n, dtype=dt_)
    L = np.zeros(n, dtype=dt_)
    for i in range(n_steps):
        x = drift + vol * z[i]
        P = P * np.exp(x)
        sum_p = sum_p + P.astype(wide)
        X = X + x
        L = L + X
    A = sum_p / wide(m)
    inv_m = f(1.0 / m)   # narrowed once
    S_T_log = f(S0) * np.exp(X)
    mean_log = L * inv_m
    G = f(S0) * np.exp(mean_log)
    G = np.where(mean_log == X, S_T_log, G)   # one exponential routine: equal exponents give equal prices
    g = payoff_of(G.astype(wide), S_T_log.astype(wide), K, strike, payoff)
    y = payoff_of(A, P.astype(wide), K, strike, payoff) if average == ARITHMETIC else g
    return dict(y=y, g=g, A=A, G=G, S_T=P, S_T_log=S_T_log)


def controlled(y, g, mu_g, disc):
    """(price, standard error, beta, rho) of the control-variate estimator from samples y and controls g with known
    mean mu_g: the arithmetic of mcamd_finalize_cv"""
    y, c = np.asarray(y, dtype=np.float64), np.asarray(g, dtype=np.float64) - mu_g
    n = y.size
    cov = np.cov(y, c, ddof=1)
    beta = cov[0, 1] / cov[1, 1]
    rho = cov[0, 1] / math.sqrt(cov[0, 0] * cov[1, 1])
    var_res = max(cov[0, 0] - beta * cov[0, 1], 0.0)
    return disc * (y.mean() - beta * c.mean()), disc * math.sqrt(var_res / n), beta, rho


# ---- closed form -----------------------------------------------------------------------------------------------------

def _N(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def _exchange(F1, F2, s):
    """E[(Y1 - Y2)+] of two lognormals with means F1, F2 and Var(ln Y1 - ln Y2) = s^2"""
    d1 = (math.log(F1 / F2) + 0.5 * s * s) / s
    return F1 * _N(d1) - F2 * _N(d1 - s)


def closed_form(S0, K, T, r, v, n_steps, include_spot, strike, payoff):
    """The mean of ln S at the dates i dt, i = 1..n (plus 0 at t = 0) is normal: mean ln S0 + mu dt sum(i) / m,
    variance v^2 dt sum_{i,j} min(i, j) / m^2 = v^2 dt n(n+1)(2n+1) / (6 m^2); its covariance with ln S_T is
    v^2 dt sum(i) / m."""
    n = n_steps
    m = n + (1 if include_spot else 0)
    dt = T / n
    mu, D = r - 0.5 * v * v, math.exp(-r * T)
    tri = n * (n + 1) / 2.0
    mean = math.log(S0) + mu * dt * tri / m
    var = v * v * dt * n * (n + 1) * (2 * n + 1) / (6.0 * m * m)
    FG = math.exp(mean + 0.5 * var)
    if strike == FIXED:
        call = D * _exchange(FG, K, math.sqrt(var))
        return call - D * (FG - K) if payoff == PUT else call
    if n == 1 and not include_spot:
        return 0.0
    var_f = v * v * T + var - 2.0 * v * v * dt * tri / m
    if not var_f > 0.0:
        return 0.0
    FS = S0 * math.exp(r * T)
    call = D * _exchange(FS, FG, math.sqrt(var_f))
    return call - D * (FS - FG) if payoff == PUT else call


# ---- the inputs the GPU tests and their CPU records share ------------------------------------------------------------

BASE = dict(S0=100.0, r=0.1, v=0.2, T=1.0)
K_ATM = 100.0
N_JOB, OFFSET, N_LOCAL, SEED = 20_000, 5003, 4096, 77   # GPU test 1: 4096 paths at global ids 5003.. of a 20 000-path job
STEPS = (50, 7)                                          # fp32 ends mid-block at 50, fp64 at 7
assert SHALLOW == (SEED, OFFSET, N_JOB)   # (seed, first path, paths of the job); DEEP: tests/deep_inputs.py
# (n_steps, where) of GPU test 1: STEPS on the shallow inputs, whose spread is RECORD["spread"], and the others,
# whose spread is RECORD["spread_more"]: 5 steps leave fp32 one step of its last block of 4 (50 leaves 2, 7
# leaves 3), and 7 steps on the deep inputs
INPUTS = tuple((n, SHALLOW) for n in STEPS)
MORE_INPUTS = ((5, SHALLOW), (7, DEEP))
CV_PATHS, CV_STEPS, CV_SEED = 200_000, 50, 20261018      # GPU test 5's shape; the record's own numpy draws

_draws = {}


def oracle_normals(bits, seed, first, n, n_steps):
    """[n_steps, n] normals of global paths first..first+n-1 as the kernels of that precision (32 / 64) draw them
    (float64 values), from the oracle's rocRAND-exact generator: Philox blocks 0, 1, .. of subsequence = path id"""
    from oracle import pyoracle as o
    key = (bits, seed, first, n, n_steps)
    if key not in _draws:
        per, draw = (2, o.normal2_f64) if bits == 64 else (4, o.normal4_f32)
        blocks = -(-n_steps // per)
        z = np.empty((blocks * per, n))
        for p in range(n):
            for k in range(blocks):
                z[k * per:(k + 1) * per, p] = draw(seed, first + p, k)
        _draws[key] = z[:n_steps]
    return _draws[key]


def restate(z, average, strike, payoff, include_spot, dtype=np.float64, K=K_ATM):
    return samples(z, BASE["S0"], K, BASE["T"], BASE["r"], BASE["v"], average, strike, payoff, include_spot, dtype)


def measure_spread(bits, inputs=INPUTS):
    """largest elementwise difference between the restatement in the kernel's precision and the next wider one over
    the cases of GPU test 1 on the given (n_steps, where)"""
    own, other = (np.float64, np.longdouble) if bits == 64 else (np.float32, np.float64)
    worst = 0.0
    for n_steps, (seed, first, _) in inputs:
        z = oracle_normals(bits, seed, first, N_LOCAL, n_steps)
        for average in (ARITHMETIC, GEOMETRIC):
            for strike, payoff, spot in PRODUCTS:
                a = restate(z, average, strike, payoff, spot, own)["y"]
                b = restate(z, average, strike, payoff, spot, other)["y"]
                worst = max(worst, float(np.abs(a - b).max()))
    return worst


def measure_rho_min():
    """smallest correlation between y and g over the controlled cases of GPU test 1's inputs (float64)"""
    rho = 1.0
    for n_steps in STEPS:
        z = oracle_normals(64, SEED, OFFSET, N_LOCAL, n_steps)
        for strike, payoff, spot in PRODUCTS:
            s = restate(z, ARITHMETIC, strike, payoff, spot)
            rho = min(rho, float(np.corrcoef(s["y"], s["g"])[0, 1]))
    return rho


def measure_controlled():
    """{(strike, payoff, include_spot): (price, standard error)} of the float64-restated controlled estimator"""
    z = np.random.default_rng(CV_SEED).standard_normal((CV_STEPS, CV_PATHS))
    disc, grow = math.exp(-BASE["r"] * BASE["T"]), math.exp(BASE["r"] * BASE["T"])
    out = {}
    for strike, payoff, spot in PRODUCTS:
        s = restate(z, ARITHMETIC, strike, payoff, spot)
        mu_g = grow * closed_form(BASE["S0"], K_ATM, BASE["T"], BASE["r"], BASE["v"], CV_STEPS, spot, strike, payoff)
        out[strike, payoff, spot] = controlled(s["y"], s["g"], mu_g, disc)[:2]
    return out


# ---- what the CPU measured (tests/test_asian_cpu.py measures again and compares) -------------------------------------

RECORD = dict(
    # largest elementwise |y(float64) - y(longdouble)| and |y(float32) - y(float64)| over the 32 average x strike x
    # payoff x include_spot x n_steps cases of GPU test 1 (its own normals).  Measured on an x86-64 CPU (80-bit
    # longdouble): 1.948e-13 and 1.2911e-4, rounded up
    spread={64: 2.0e-13, 32: 1.30e-4},
    # the same over the 64 cases of MORE_INPUTS.  Measured likewise: 7.012e-14 and 4.696e-5, rounded up.  Both lie below
    # spread, so the GPU test holds these cases to the tolerance made of spread
    spread_more={64: 7.1e-14, 32: 4.8e-5},
    # smallest correlation of the arithmetic sample with its geometric control over the 16 controlled cases of the
    # same inputs (float64).  Measured: 0.999504 (floating put without the spot, 7 steps), rounded down
    rho_min=0.99950,
    # float64-restated controlled price and standard error of GPU test 5's products, (strike, payoff, include_spot):
    # CV_PATHS paths of CV_STEPS steps from numpy's default_rng(CV_SEED)
    controlled={
        (FIXED, CALL, 0): (7.165302888420202, 0.0005790530311865419),
        (FIXED, CALL, 1): (7.024797967685609, 0.0005722294352872657),
        (FIXED, PUT, 0): (2.3902662372218764, 0.00024395605094277694),
        (FIXED, PUT, 1): (2.343388293936061, 0.00023867687090459118),
        (FLOATING, CALL, 0): (7.1636602375178615, 0.0005337583076981703),
        (FLOATING, CALL, 1): (7.264563108432845, 0.0005452539388711983),
        (FLOATING, PUT, 0): (2.4212177578005147, 0.0002565971242039249),
        (FLOATING, PUT, 1): (2.428487407604303, 0.0002608051287866565),
    },
)
