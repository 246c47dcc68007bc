"""numpy restatement of the least-squares Monte Carlo definitions of include/mcamd.h (mcamd_price_american), used by
tests/test_gpu_american.py, and a Cox-Ross-Rubinstein tree that exercises at the same dates.

For tests/test_gpu_american_solver.py and tests/test_american_solver_cpu.py: the references of the solver and the
decision of csrc/american_device.hpp, call by call — the normal equations of one 12-double record solved exactly in
rationals (solve_record), an fp64 replica of am_solve's own operation order (solve_replica), the fused multiply-add
emulated exactly (fma, continuation, decide) — and the accuracy ladder both files walk (ladder)."""
import math
from fractions import Fraction

import numpy as np

PIVOT_MIN = 1e-10          # am_solve: a scaled pivot <= this -> the date is not regressed
# The shape matrix of tests/test_gpu_american.py: (put, exercise_every, n_basis, precision, n_steps).  Every n_basis
# with every precision, every exercise_every with both payoffs; fp64 (2 steps per Philox block) with odd step counts,
# fp32 (4 per block) with every remainder: 48 -> 0, 21 and 49 -> 1, 50 -> 2, 63 -> 3
SHAPES = [(True, 1, 2, 64, 21), (False, 3, 3, 64, 21), (True, 7, 4, 64, 21), (False, 1, 3, 64, 49), (True, 1, 4, 64, 50),
          (False, 7, 2, 32, 21), (True, 3, 3, 32, 63), (False, 1, 4, 32, 63), (True, 7, 4, 32, 49), (False, 1, 2, 32, 50),
          (True, 3, 2, 32, 48), (False, 3, 4, 32, 21)]
PIVOT_MIN_FIRST = 1e-12    # the threshold first shipped; the ladder around it is what shows it to be too low
BAND = (0.5 * PIVOT_MIN, 2 * PIVOT_MIN)    # exact pivots in here: either answer of am_solve is accepted (its own pivots are rounded)


def band(pivot_min=PIVOT_MIN):
    return 0.5 * pivot_min, 2 * pivot_min


EPS = 2.0 ** -53
# The ladder's accuracy bound: |fitted - exact fit| <= C * 2^-53 / (smallest exact scaled pivot) of the fit's scale.
# C_REPLICA is the maximum of error * pivot / 2^-53 that solve_replica (fp64, am_solve's operation order, every
# operation rounded on its own) reaches over the ladder, rounded up to two digits
# (tests/test_american_solver_cpu.py holds it to the measurement).  The device contracts multiply-adds and may order
# operands differently, so it is allowed 4 times that.
C_REPLICA = 4.8
C_DEVICE = 4.0 * C_REPLICA


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
        if not s > PIVOT_MIN:
            return False, None
        L[c, c] = math.sqrt(s)
        for r_ in range(c + 1, m):
            L[r_, c] = (As[r_, c] - L[r_, :c] @ L[c, :c]) / L[c, c]
    beta, *_ = np.linalg.lstsq(X * D[None, :], V, rcond=None)
    return True, beta * D


def sweep(rows, K, put, k, m, disc, beta_gpu, flags_gpu, pivots=None):
    """The backward sweep on stored rows [n_steps, n] (float64), deciding with the engine's coefficients.
    Returns V and, per date j = M-1..1, (j, regressed, in-the-money mask, numpy continuation, engine continuation).
    pivots: a dict that receives, per date j, (|I_j|, smallest exact scaled pivot of the date's record, or None
    where |I_j| < 4 m); fit's own rounded pivots then do not decide: the date counts as regressed when the exact
    pivot is above PIVOT_MIN."""
    M = len(disc)
    V = disc[M - 1] * payoff(rows[M * k - 1], K, put)
    out = []
    for j in range(M - 1, 0, -1):
        S = rows[j * k - 1]
        h = payoff(S, K, put)
        itm = h > 0
        X = basis(S[itm], K, m)
        if pivots is None:
            ok, beta = fit(S[itm], V[itm], K, m)
        else:
            n_itm = int(itm.sum())
            piv = float(min(solve_record(record(S[itm] / K - 1.0, V[itm]), m)[1])) if n_itm >= 4 * m else None
            pivots[j] = (n_itm, piv)
            ok = piv is not None and piv > PIVOT_MIN
            beta = np.linalg.lstsq(X / np.sqrt((X * X).sum(axis=0)), V[itm], rcond=None)[0] / np.sqrt(
                (X * X).sum(axis=0)) if ok else None
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


# ---- the solver and the decision, call by call -----------------------------------------------------------------------

def record(u, V):
    """The 12-double sweep record of the points (u, V): P_0..P_6, sum V u^q (q < 4), |I| — powers by repeated
    multiplication as the sweep forms them, summed by numpy"""
    u = np.asarray(u, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    rec = np.zeros(12)
    p = np.ones_like(u)
    for q in range(7):
        rec[q] = p.sum()
        if q < 4:
            rec[7 + q] = (V * p).sum()
        p = p * u
    rec[11] = float(len(u))
    return rec


def solve_record(rec, m):
    """(beta, pivots) of a record, exactly: A = Hankel(P_0..P_{2m-2}), b = (sum V u^q) taken as the rationals the
    doubles are; pivots[c] is the c-th pivot of the Cholesky of D A D, D = diag(A)^(-1/2), which is rational: the
    c-th pivot of A itself over A[c][c].  beta is a list of Fractions, or None when a pivot is not positive (pivots
    then ends at the first such one).  The count rule is not applied here."""
    P = [Fraction(float(x)) for x in rec[:2 * m - 1]]
    b = [Fraction(float(x)) for x in rec[7:7 + m]]
    A = [[P[r + c] for c in range(m)] + [b[r]] for r in range(m)]
    pivots = []
    for c in range(m):   # elimination without exchanges: the pivots of A = L diag(p) L^T
        diag = P[2 * c]
        if diag <= 0:
            pivots.append(Fraction(0))
            return None, pivots
        pivots.append(A[c][c] / diag)
        if A[c][c] <= 0:
            return None, pivots
        for r in range(c + 1, m):
            f = A[r][c] / A[c][c]
            A[r] = [x - f * y for x, y in zip(A[r], A[c])]
    beta = [Fraction(0)] * m
    for a in range(m - 1, -1, -1):
        beta[a] = (A[a][m] - sum(A[a][q] * beta[q] for q in range(a + 1, m))) / A[a][a]
    return beta, pivots


def solve_replica(rec, m, pivot_min=PIVOT_MIN):
    """am_solve restated in Python floats: the same operations in the same order, each rounded on its own (no
    contraction).  Returns (ok, beta)."""
    rec = [float(x) for x in rec]
    inf = math.inf
    ok = rec[11] >= 4.0 * m and rec[11] < inf
    D = []
    for a in range(m):
        d = rec[2 * a]
        ok = ok and d > 0.0
        D.append(1.0 / math.sqrt(d) if d > 0.0 else 0.0)
    L = [[0.0] * m for _ in range(m)]
    for c in range(m):
        s = rec[2 * c] * D[c] * D[c]
        for q in range(c):
            s -= L[c][q] * L[c][q]
        ok = ok and s > pivot_min
        l = math.sqrt(s if s > pivot_min else 1.0)
        L[c][c] = l
        for r in range(c + 1, m):
            t = rec[r + c] * D[r] * D[c]
            for q in range(c):
                t -= L[r][q] * L[c][q]
            L[r][c] = t / l
    y = [0.0] * m
    for a in range(m):
        t = rec[7 + a] * D[a]
        for q in range(a):
            t -= L[a][q] * y[q]
        y[a] = t / L[a][a]
    beta = [0.0] * m
    for a in range(m - 1, -1, -1):
        t = y[a]
        for q in range(a + 1, m):
            t -= L[q][a] * beta[q]
        beta[a] = t / L[a][a]
    for a in range(m):
        beta[a] *= D[a]
        ok = ok and abs(beta[a]) < inf
    return ok, beta


def fit_error(beta, beta_exact, u):
    """max |phi(u) . beta - phi(u) . beta_exact| over the points u, over max |phi(u) . beta_exact|: exact arithmetic on
    the difference of the coefficients, so the cancellation between them costs nothing"""
    d = [Fraction(float(b)) - e for b, e in zip(beta, beta_exact)]
    err = scale = Fraction(0)
    for x in u:
        x = Fraction(float(x))
        e = f = Fraction(0)
        for dq, bq in zip(reversed(d), reversed(beta_exact)):
            e = e * x + dq
            f = f * x + bq
        err, scale = max(err, abs(e)), max(scale, abs(f))
    return float(err / scale)


def sample_points(u, k=33):
    """k of the points by rank, both extremes included.  The error of a fit is a polynomial of degree < 4 in u, so
    its maximum over 33 evenly ranked points is its maximum over all of them to within a few per cent."""
    u = np.sort(np.asarray(u))
    return u if len(u) <= k else u[np.unique(np.round(np.linspace(0, len(u) - 1, k)).astype(int))]


# smallest exact scaled pivots the ladder aims at: decades far from the rule's threshold, a fine ladder either side of
# it (factors of the threshold) that leaves the band out
LADDER_NEAR = [30.0, 10.0, 6.0, 4.0, 3.0, 2.5, 2.2, 0.45, 0.4, 0.3, 0.2, 0.1, 0.03]
LADDER_BIG_NEAR = [1000.0, 10.0, 4.0, 2.5, 0.4, 0.1, 0.01]   # the million-point sets


def ladder_targets(pivot_min):
    return ([0.3] + [10.0 ** -e for e in range(1, 15) if not 0.02 * pivot_min < 10.0 ** -e < 50 * pivot_min]
            + [f * pivot_min for f in LADDER_NEAR])


LADDER_CENTRES = {True: [-0.9, -0.5, -0.25, -0.05], False: [0.05, 0.5, 1.5, 2.9]}   # put: c in (-1, 0); call: (0, 3)
LADDER_BIG = {-0.25, 1.5}   # the centres that also get a million points, at the factors of LADDER_BIG_NEAR


def ladder_points(c, rho, x):
    return c + (c / rho) * x


def ladder_values(u, noise):
    return 0.1 - 0.3 * u + 0.5 * u * u - 0.2 * u ** 3 + 0.02 * noise


def ladder(pivot_min=PIVOT_MIN, near_only=False):
    """The accuracy ladder: cases (m, c, rho, n, u, rec, beta_exact, pivot) with points u = c + (c / rho) x, x fixed per
    (c, n) in [-1, 1] with both ends present, V a cubic in u plus noise, rho from 1 up to where the smallest exact
    scaled pivot is about 1e-14.  For large rho that pivot is kappa * rho^(-2 (m - 1)); kappa is measured (exactly)
    at a pivot near pivot_min, and rho is then placed at ladder_targets(pivot_min), which leave out the band either
    side of pivot_min where am_solve's own rounded pivot may fall on either side.  near_only: only the fine ladder
    from 30 to 0.03 times pivot_min, without the million-point sets — the part that tells what a threshold lets
    through."""
    cases = []
    for put in (True, False):
        for c in LADDER_CENTRES[put]:
            for m in (2, 3, 4):
                for n in [4 * m, 64, 4000] + ([1_000_000] if c in LADDER_BIG and not near_only else []):
                    rng = np.random.default_rng([int(round(abs(c) * 100)), m, n, int(put)])
                    x = rng.uniform(-1.0, 1.0, n)
                    x[0], x[1] = -1.0, 1.0
                    noise = rng.standard_normal(n)
                    power = 2 * (m - 1)

                    def case(rho):
                        u = ladder_points(c, rho, x)
                        rec = record(u, ladder_values(u, noise))
                        beta, piv = solve_record(rec, m)
                        return u, rec, beta, float(min(piv))

                    kappa = 1.0
                    for _ in range(2):
                        rho = max((kappa / pivot_min) ** (1.0 / power), 1.0)
                        kappa = max(case(rho)[3], 1e-300) * rho ** power
                    if near_only:
                        targets = [f * pivot_min for f in LADDER_NEAR]
                    elif n < 1_000_000:
                        targets = ladder_targets(pivot_min)
                    else:
                        targets = [f * pivot_min for f in LADDER_BIG_NEAR]
                    for rho in sorted({max((kappa / t) ** (1.0 / power), 1.0) for t in targets}):
                        u, rec, beta, piv = case(rho)
                        cases.append(dict(m=m, put=put, c=c, rho=rho, n=n, u=sample_points(u), rec=rec, beta=beta,
                                          pivot=piv))
    return cases


def band_share(cases, pivot_min=PIVOT_MIN):
    lo, hi = band(pivot_min)
    return sum(lo <= k["pivot"] <= hi for k in cases) / len(cases)


def fma_fraction(a, b, c):
    """a * b + c of finite doubles with one rounding, from the definition (no signed zero, no overflow)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


_TWO53 = 9007199254740992.0


def fma(a, b, c):
    """a * b + c with one rounding, exactly: fma_fraction on integers (the mantissas multiplied and added as Python
    integers, one correctly rounded conversion), with the signed zeros and the overflow of IEEE 754.  Non-finite
    operands take the plain expression, whose result is then the same."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    ma, ea = math.frexp(a)
    mb, eb = math.frexp(b)
    mc, ec = math.frexp(c)
    ep, ec = ea + eb - 106, ec - 53
    e = min(ep, ec)
    tot = ((int(ma * _TWO53) * int(mb * _TWO53)) << (ep - e)) + (int(mc * _TWO53) << (ec - e))
    if tot == 0:   # an exact zero: the common sign of product and addend if they are both zeros of one sign, else +0
        sp = math.copysign(1.0, a) * math.copysign(1.0, b)
        return -0.0 if (a == 0 or b == 0) and c == 0 and sp < 0 and math.copysign(1.0, c) < 0 else 0.0
    try:
        return float(tot << e) if e >= 0 else tot / (1 << -e)
    except OverflowError:
        return math.inf if tot > 0 else -math.inf


def continuation(beta, u):
    """am_continuation: Horner, one fused multiply-add per coefficient"""
    c = float(beta[-1])
    for b in reversed(beta[:-1]):
        c = fma(c, float(u), float(b))
    return c


def decide(beta, disc, K, put, S):
    """am_exercise and am_continuation of one case: (exercised, y or None when h = 0, continuation at
    u = S / K - 1 with its two roundings)"""
    S, K, disc = float(S), float(K), float(disc)
    cont = continuation(beta, S / K - 1.0)
    h = K - S if put else S - K
    if not h > 0.0:
        return False, None, cont
    y = disc * h
    return y > cont, y, cont
