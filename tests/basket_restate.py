"""numpy restatement of the basket definitions of include/mcamd.h (mcamd_price_basket), used by
tests/test_gpu_basket.py and tested against itself and the host closed forms in tests/test_basket_cpu.py.

Three things live here:
  * samples(): the estimator, given the flat stream of a path's normals (row i d + k is z_{i,k}), in one numpy dtype
    throughout — float64, longdouble or float32 — with numpy.linalg.cholesky for the factor and the kernel's order of
    fused multiply-adds (ascending k from the drift).  numpy has no fused multiply-add: float32 forms the product and
    the sum in float64 (the product is exact there) and rounds once more, float64 does the same through longdouble, and
    longdouble multiplies and adds;
  * rainbow2_by_quadrature(): the best- or worst-of-two call or put at any K, by conditioning on z_0 (then the second
    asset is lognormal and each inner expectation is a Black-Scholes-type term) and Gauss-Legendre over z_0 — the
    independent reference for K > 0, written without reference to the C code;
  * the inputs the CPU and GPU tests share, the oracle's normals for them, and the tolerances measured from them."""
import ctypes as C
import math

import numpy as np

from deep_inputs import DEEP, SHALLOW

ARITHMETIC, GEOMETRIC, BEST_OF, WORST_OF = 0, 1, 2, 3
KINDS = (ARITHMETIC, GEOMETRIC, BEST_OF, WORST_OF)
CALL, PUT = 0, 1
NO_BARRIER, DOWN_OUT, DOWN_IN, UP_OUT, UP_IN = 0, 1, 2, 3, 4
BARRIERS = (DOWN_OUT, DOWN_IN, UP_OUT, UP_IN)
F32, F64 = 32, 64
NP_T = {F64: np.float64, F32: np.float32}
PER_BLOCK = {F64: 2, F32: 4}


def _fma(a, b, c, dt_):
    if dt_ == np.dtype(np.float32):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
    if dt_ == np.dtype(np.float64):
        ld = np.longdouble
        return (np.asarray(a, ld) * np.asarray(b, ld) + np.asarray(c, ld)).astype(np.float64)
    return a * b + c


def samples(z, n_steps, S0, v, w, corr, K, T, r, kind, payoff, barrier=NO_BARRIER, B=0.0, dtype=np.float64):
    """z: [>= n_steps d, n_paths] normals, row i d + k = z_{i,k}.  Returns a dict: y (float64 samples, or longdouble
    when dtype is), X ([d, n_paths] log-returns), logA (the log aggregate at maturity; None for arithmetic), hit,
    live (the steps each path entered not yet hit; zeros without a barrier) and min_abs_d (the smallest
    |ln A_i - ln B| over the step ends, natural-log units; inf without a barrier)."""
    dt_ = np.dtype(dtype)
    f = dt_.type
    d = len(S0)
    n = z.shape[1]
    assert z.shape[0] >= n_steps * d
    S0, v, w = (np.asarray(a, dtype=np.float64) for a in (S0, v, w))
    L = np.linalg.cholesky(np.asarray(corr, dtype=np.float64)[:d, :d])
    dt = T / n_steps                                        # the host's fp64 set-up, narrowed once
    drift = ((r - 0.5 * v * v) * dt).astype(dt_)
    coef = (v[:, None] * math.sqrt(dt) * L).astype(dt_)
    monitored = barrier != NO_BARRIER
    up = barrier in (UP_OUT, UP_IN)
    log_w = np.log(w * S0).astype(dt_) if kind in (BEST_OF, WORST_OF) else None
    logB = f(math.log(B)) if monitored else None

    def extreme(X):
        l = log_w[0] + X[0]
        for j in range(1, d):
            l = np.maximum(l, log_w[j] + X[j]) if kind == BEST_OF else np.minimum(l, log_w[j] + X[j])
        return l

    X = [np.zeros(n, dtype=dt_) for _ in range(d)]
    alive = np.ones(n, dtype=bool)
    live = np.zeros(n, dtype=np.int64)
    min_abs_d = np.full(n, np.inf)
    for i in range(n_steps):
        x = [np.full(n, drift[j], dtype=dt_) for j in range(d)]
        for k in range(d):
            zk = z[i * d + k].astype(dt_)
            for j in range(k, d):
                x[j] = _fma(coef[j, k], zk, x[j], dt_)
        X = [X[j] + x[j] for j in range(d)]
        if monitored:
            live += alive
            l = extreme(X)
            alive &= ~((l >= logB) if up else (l <= logB))
            min_abs_d = np.minimum(min_abs_d, np.abs((l - logB).astype(np.float64)))
    wide = np.longdouble if dt_ == np.dtype(np.longdouble) else np.float64
    logA = None
    if kind == ARITHMETIC:
        A = np.zeros(n, dtype=wide)
        for j in range(d):
            A = A + wide(w[j]) * (f(S0[j]) * np.exp(X[j])).astype(wide)
    else:
        if kind == GEOMETRIC:
            logA = np.full(n, f(np.dot(w, np.log(S0))), dtype=dt_)
            for j in range(d):
                logA = _fma(f(w[j]), X[j], logA, dt_)
        else:
            logA = extreme(X)
        A = np.exp(logA).astype(wide)
    y = np.maximum(wide(K) - A if payoff == PUT else A - wide(K), wide(0))
    if monitored:
        pays = alive if barrier in (DOWN_OUT, UP_OUT) else ~alive
        y = np.where(pays, y, wide(0))
    return dict(y=y, X=np.stack(X), logA=logA, hit=~alive, live=live, min_abs_d=min_abs_d)


# ---- the independent reference for two assets ----------------------------------------------------------------------------

_N = np.vectorize(lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0)))
_GL_X, _GL_W = np.polynomial.legendre.leggauss(16)


def rainbow2_by_quadrature(a1, a2, v1, v2, rho, K, T, r, best, put, panels=400, reach=10.0):
    """e^{-rT} E[h(max or min(A1, A2))] with A_j = a_j exp((r - v_j^2/2) T + v_j sqrt(T) W_j), corr(W_1, W_2) = rho,
    h(A) = (A - K)+ or (K - A)+.  Given z_0 = W_1, A1 = a is known and A2 = Y is lognormal: ln Y ~ N(mu, s^2),
    mu = ln a2 + (r - v2^2/2) T + v2 sqrt(T) rho z_0, s = v2 sqrt(T (1 - rho^2)).  Best-of pays h(a) where Y <= a and
    h(Y) where Y > a; worst-of the other way round.  With P(c) = P[Y < c] = N((ln c - mu) / s) and
    M(c) = E[Y 1{Y < c}] = e^{mu + s^2/2} N((ln c - mu) / s - s), every piece is a difference of such terms.  The
    integrand has kinks (where a crosses K), so the z_0 axis is cut into panels of 16 Gauss-Legendre nodes."""
    sq = math.sqrt(T)
    edges = np.linspace(-reach, reach, panels + 1)
    h, c = 0.5 * np.diff(edges), 0.5 * (edges[:-1] + edges[1:])
    z0 = (c[:, None] + h[:, None] * _GL_X[None, :]).ravel()
    wq = (h[:, None] * _GL_W[None, :]).ravel() * np.exp(-0.5 * z0 * z0) / math.sqrt(2.0 * math.pi)
    a = a1 * np.exp((r - 0.5 * v1 * v1) * T + v1 * sq * z0)
    mu = math.log(a2) + (r - 0.5 * v2 * v2) * T + v2 * sq * rho * z0
    s = v2 * sq * math.sqrt(1.0 - rho * rho)
    mean = np.exp(mu + 0.5 * s * s)

    def P(c_):    # P[Y < c]; c = 0 gives 0
        c_ = np.asarray(c_, dtype=float)
        return np.where(c_ > 0, _N((np.log(np.maximum(c_, 1e-300)) - mu) / s), 0.0)

    def M(c_):    # E[Y 1{Y < c}]
        c_ = np.asarray(c_, dtype=float)
        return np.where(c_ > 0, mean * _N((np.log(np.maximum(c_, 1e-300)) - mu) / s - s), 0.0)

    def between(lo, hi):   # E[(Y - K) 1{lo < Y < hi}] for lo <= hi (elementwise; hi may be inf)
        p_hi = np.where(np.isinf(hi), 1.0, P(np.where(np.isinf(hi), 1.0, hi)))
        m_hi = np.where(np.isinf(hi), mean, M(np.where(np.isinf(hi), 1.0, hi)))
        return (m_hi - M(lo)) - K * (p_hi - P(lo))

    h_a = np.maximum(K - a if put else a - K, 0.0)
    inf = np.full_like(a, np.inf)
    zero = np.zeros_like(a)
    if best:       # Y <= a pays h(a); Y > a pays h(Y)
        fixed = h_a * P(a)
        lo, hi = (a, np.maximum(a, K)) if put else (np.maximum(a, K), inf)      # put: a < Y < K; call: Y > max(a, K)
    else:          # Y >= a pays h(a); Y < a pays h(Y)
        fixed = h_a * (1.0 - P(a))
        lo, hi = (zero, np.minimum(a, K)) if put else (np.minimum(a, K), a)     # put: Y < min(a, K); call: K < Y < a
    part = between(lo, hi)
    inner = fixed + (-part if put else part)
    return math.exp(-r * T) * float(np.dot(wq, inner))


def geometric_lognormal(S0, v, w, corr, K, T, r, put):
    """the geometric basket restated: ln A_T ~ N(m, s^2)"""
    S0, v, w = (np.asarray(a, dtype=np.float64) for a in (S0, v, w))
    d = len(S0)
    m = float(np.dot(w, np.log(S0) + (r - 0.5 * v * v) * T))
    cov = np.outer(v, v) * np.asarray(corr, dtype=np.float64)[:d, :d]
    s = math.sqrt(T * float(w @ cov @ w))
    N = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))
    F, D = math.exp(m + 0.5 * s * s), math.exp(-r * T)
    d1 = (m - math.log(K)) / s + s
    return D * (K * N(-(d1 - s)) - F * N(-d1)) if put else D * (F * N(d1) - K * N(d1 - s))


# ---- what the CPU and the GPU tests share --------------------------------------------------------------------------------

R, T_ = 0.05, 1.0
N_JOB, OFFSET, N_LOCAL, SEED = 20_000, 5003, 4096, 77
DS, STEPS = (1, 2, 3, 5, 8), (1, 2, 7, 50)
# The widths DS leaves out.  In fp32 d = 6 is the only width whose group is 2 steps of 3 blocks and d = 7 the only one of
# 4 steps of 7 blocks; d = 6 and 7 are also the widths with the most coefficients held in registers.
MORE_DS = (4, 6, 7)
assert SHALLOW == (SEED, OFFSET, N_JOB)   # (seed, first path, paths of the job); DEEP: tests/deep_inputs.py
DEEP_STEPS = 7                            # the step count of every case on the DEEP inputs
# A path whose restated min_i |ln A_i - ln B| is below MARGIN is left out of the elementwise comparison of a barrier
# case, and a case may leave out at most CAP of its paths: both are those of tests/test_gpu_barrier.py.
MARGIN, CAP = 2e-5, 0.01
# B = 0.8 for the down barriers.  An up barrier needs A_0 < B, and A_0 = 1 here (w_j = 1 / S0_j): it takes the mirror
# image 1 / 0.8.
LEVEL = {DOWN_OUT: 0.8, DOWN_IN: 0.8, UP_OUT: 1.25, UP_IN: 1.25}
# Largest elementwise difference between two restatements over the 480 cases of test 1 of tests/test_gpu_basket.py on
# d in DS (float64 against longdouble for the fp64 kernels, float32 against float64 for the fp32 kernels; margin paths
# of the barrier cases left out), measured by tests/test_basket_cpu.py on an x86-64 CPU (80-bit longdouble) and recorded
# in DESIGN section 15.  The test there fails if a measurement exceeds its record.  The other cases of test 1
# (MORE_CASES, DEEP_CASES) are measured there too and stay below it: they take the same tolerance.
SPREAD = {F64: 4.1e-13, F32: 2.3e-4}


def inputs(d):
    """S0_j = 80 + 10 j, v_j = 0.15 + 0.05 j, corr_jk = 0.6^|j - k| (every leading block is positive definite)"""
    j = np.arange(d)
    return 80.0 + 10.0 * j, 0.15 + 0.05 * j, 0.6 ** np.abs(j[:, None] - j[None, :])


def weights(kind, d):
    """(w, K): performances struck at 1 for best-of and worst-of, equal weights struck at 100 otherwise"""
    S0 = inputs(d)[0]
    return (1.0 / S0, 1.0) if kind in (BEST_OF, WORST_OF) else (np.full(d, 1.0 / d), 100.0)


def elementwise_tolerance(prec, want):
    """Absolute tolerance per element: 4 x SPREAD, floored at 1e-11 of the sample (fp64) / 2e-3 (fp32), the floors of
    tests/test_gpu_lookback.py."""
    if prec == F64:
        return np.maximum(4.0 * SPREAD[F64], 1e-11 * np.abs(want))
    return np.full(np.shape(want), max(4.0 * SPREAD[F32], 2e-3))


_streams = {}


def stream(prec, seed=SEED, first=OFFSET, n=N_LOCAL, n_normals=max(DS) * max(STEPS)):
    """[n_normals, n] normals of global paths first..first+n-1 as the kernels draw them (float64 values): normal q of
    a path is slot q % NB of Philox block q / NB of the path's subsequence, from the oracle's rocRAND-exact generator"""
    from oracle import pyoracle as o
    key = (prec, seed, first, n, n_normals)
    if key not in _streams:
        per = PER_BLOCK[prec]
        blocks = -(-n_normals // per)
        L = o.lib()
        if prec == F64:
            buf, fn, ct = np.empty((n, blocks * per), dtype=np.float64), L.oracle_normal2_f64, C.c_double
        else:
            buf, fn, ct = np.empty((n, blocks * per), dtype=np.float32), L.oracle_normal4_f32, C.c_float
        base, row, size = buf.ctypes.data, buf.strides[0], buf.itemsize * per
        ptr = C.POINTER(ct)
        for p in range(n):
            for k in range(blocks):
                fn(seed, first + p, k, C.cast(base + p * row + k * size, ptr))
        _streams[key] = np.ascontiguousarray(buf.T[:n_normals].astype(np.float64))
    return _streams[key]


_restated = {}


def compare(prec, kind, payoff, barrier, d, n_steps, where=SHALLOW):
    """The restatement of one case of the GPU test's elementwise comparison on its inputs, CPU only: (samples to compare
    with as float64, the restatement in the kernel's precision, paths kept, largest difference between the two
    restatements over the kept paths).  An fp64 kernel is compared with the float64 restatement and an fp32 kernel
    with the float64 one too.  where: SHALLOW or DEEP, the seed and the first path the normals are drawn for."""
    key = (prec, kind, payoff, barrier, d, n_steps, where)
    if key not in _restated:
        S0, v, corr = inputs(d)
        w, K = weights(kind, d)
        # the deep cases all have DEEP_STEPS steps: no more of the stream is drawn than they read
        z = stream(prec) if where == SHALLOW else stream(prec, where[0], where[1], n_normals=max(DS) * DEEP_STEPS)
        B = LEVEL.get(barrier, 0.0)
        own = samples(z, n_steps, S0, v, w, corr, K, T_, R, kind, payoff, barrier, B, NP_T[prec])
        other = samples(z, n_steps, S0, v, w, corr, K, T_, R, kind, payoff, barrier, B,
                        np.longdouble if prec == F64 else np.float64)
        keep = (own["min_abs_d"] >= MARGIN) & (other["min_abs_d"] >= MARGIN)
        spread = float(np.abs(own["y"] - other["y"])[keep].max())
        want = own["y"] if prec == F64 else other["y"]
        _restated[key] = (np.asarray(want, dtype=np.float64), own, keep, spread)
    return _restated[key]


def cases(ds, steps):
    """every kind without a barrier, and best-of and worst-of with every barrier direction, at each width and step count"""
    plain = [(kind, CALL if (kind + d) % 2 else PUT, NO_BARRIER, d, n) for kind in KINDS for d in ds for n in steps]
    barrier = [(kind, PUT if barrier in (DOWN_OUT, DOWN_IN) else CALL, barrier, d, n)
               for kind in (BEST_OF, WORST_OF) for barrier in BARRIERS for d in ds for n in steps]
    return plain, barrier


PLAIN_CASES, BARRIER_CASES = cases(DS, STEPS)
MORE_CASES = sum(cases(MORE_DS, STEPS), [])                       # on the SHALLOW inputs: 144 cases
DEEP_CASES = sum(cases(tuple(range(1, 9)), (DEEP_STEPS,)), [])    # on the DEEP inputs: 96 cases
