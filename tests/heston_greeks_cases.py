"""What tests/test_heston_greeks_cpu.py and tests/test_gpu_heston_greeks.py share: the request every test makes, the
numpy restatement of include/mcamd_heston_greeks.h on top of tests/heston_restate.py (rows, record, finalize), and the
scheme bias b_k that the GPU statistical test allows for.

The rows are restated from the header text: every walk is hr.samples at its own model on the SAME normals; rows 1 and 2
are formed from the base walk's S_T in the path's dtype, each product one multiply.

SCHEME BIAS.  The kernel estimates the Greeks of the full-truncation Euler scheme at 128 steps; mcamd_heston_greeks_f64
gives the model's.  b_k = |restated value - closed form| + 4 (restated SE), per value k, measured ONCE with the float64
restatement on numpy normals (np.random.default_rng(20261021), no Philox) at input F, 128 steps, 2^22 paths in chunks of
2^17, all five bumps BUMPS and gamma_eta = ETA, by `python tests/heston_greeks_cases.py` (measure_bias below; two and a
half minutes on one x86-64 core).  b_k is itself a noisy one-run figure, which is why the GPU test allows 2 b_k beside its
own 4 SE.  BIAS holds the printed figures; the run is recorded in DESIGN.md beside them."""
import math

import numpy as np

import heston_restate as hr

PARAMS = ("v0", "kappa", "theta", "xi", "rho")          # the order of mcamd_heston_greeks_job.bump
NAMES = ("price", "delta", "gamma", "rho", "rho_q", "v0", "kappa", "theta", "xi", "corr")
BUMPS = dict(v0=0.005, kappa=0.05, theta=0.005, xi=0.05, rho=0.05)   # every bumped F, N and H is a legal model
ETA = 0.01
STATS = 32
STAT_STRIKES = ((100.0, hr.CALL), (80.0, hr.PUT))        # the GPU statistical run
STAT_STEPS = 128

# measure_bias(): {(K, payoff): [b_k for the ten values]}; see the module docstring for the run
BIAS = {
    #                 price      delta      gamma      rho        rho_q      v0         kappa      theta      xi         corr
    (100.0, hr.CALL): [2.386e-02, 1.160e-03, 2.038e-04, 1.021e-01, 1.160e-01, 2.582e-01, 3.697e-03, 3.878e-01, 3.975e-02, 2.115e-02],
    (80.0, hr.PUT):   [9.765e-03, 5.143e-04, 1.206e-04, 5.769e-02, 5.143e-02, 1.720e-01, 1.143e-03, 1.798e-01, 1.521e-02, 7.082e-03],
}


def bump_list(bumps):
    """the five half-widths in the job's order, 0 where `bumps` (a dict) names none"""
    return [float(bumps.get(p, 0.0)) for p in PARAMS]


def requested(bumps):
    return [p for p in PARAMS if bumps.get(p, 0.0) > 0.0]


def walks(name, bumps, **changes):
    """[(label, heston_params)] of the 1 + 2 P walks in the kernel's order; the bumped value is formed in float64"""
    out = [("base", hr.params(name, **changes))]
    for p in requested(bumps):
        b = dict(zip(PARAMS, hr.params(name, **changes)[1:]))[p]
        out.append((p + "+", hr.params(name, **dict(changes, **{p: b + bumps[p]}))))
        out.append((p + "-", hr.params(name, **dict(changes, **{p: b - bumps[p]}))))
    return out


def payoff_of(S, K, payoff):
    f = S.dtype.type
    return np.maximum(f(K) - S, f(0)) if payoff == hr.PUT else np.maximum(S - f(K), f(0))


def rows_from_state(S_T, h_bumped, K, payoff, eta):
    """the (3 + 2 P, n) rows in S_T's dtype from the base walk's S_T and the 2 P bumped payoff rows"""
    f = S_T.dtype.type
    u, ui = f(math.exp(eta)), f(math.exp(-eta))
    sgn = f(-1) if payoff == hr.PUT else f(1)
    h = payoff_of(S_T, K, payoff)
    d = np.where(h > 0, sgn * S_T, f(0))
    up = (payoff_of(S_T * u, K, payoff) > 0).astype(S_T.dtype)
    dn = (payoff_of(S_T * ui, K, payoff) > 0).astype(S_T.dtype)
    g = sgn * S_T * (up - dn) + f(0)   # + 0: no negative zero
    return np.stack([h, d, g] + [np.asarray(r, dtype=S_T.dtype) for r in h_bumped])


def restated_rows(z, zv, name, K, payoff, eta, bumps, dtype=np.float64, S0=hr.S0, T=hr.T_, r=hr.R):
    """(rows, base samples dict) of the restatement on the normals z, zv"""
    ws = walks(name, bumps)
    base = hr.samples(z, zv, S0, K, T, r, ws[0][1], payoff, dtype)
    bumped = [payoff_of(hr.samples(z, zv, S0, K, T, r, p, payoff, dtype)["S_T"], K, payoff) for _, p in ws[1:]]
    return rows_from_state(base["S_T"], bumped, K, payoff, eta), base


def record(rows, trunc_sum, rv_sum):
    """the 32-double record of float64 rows (3 + 2 P, n), summed by numpy"""
    rows = np.asarray(rows, dtype=np.float64)
    P = (rows.shape[0] - 3) // 2
    y, d, g = rows[0], rows[1], rows[2]
    e = d - y
    rec = [y.sum(), (y * y).sum(), d.sum(), (d * d).sum(), (e * e).sum(), g.sum(), (g * g).sum()]
    for j in range(P):
        c = rows[3 + 2 * j] - rows[4 + 2 * j]
        rec += [c.sum(), (c * c).sum()]
    rec += [float(trunc_sum), float(rv_sum), float(rows.shape[1])]
    return np.array(rec + [0.0] * (STATS - len(rec)))


def finalize(rec, S0, r, T, eta, bump5):
    """(value[10], std_err[10], truncated_steps, mean_variance) of a record, by the header's formulas"""
    rec = [float(x) for x in rec]
    P = sum(1 for b in bump5 if b > 0.0)
    N = rec[9 + 2 * P]
    disc = math.exp(-r * T)

    def est(s, ss, factor):
        mean = s / N if N else 0.0
        var = (ss - N * mean * mean) / (N - 1.0) if N > 1 else 0.0
        var = max(var, 0.0)
        return factor * (disc * mean), abs(factor) * (disc * math.sqrt(var / N) if N else 0.0)

    value, se = [0.0] * 10, [0.0] * 10
    value[0], se[0] = est(rec[0], rec[1], 1.0)
    value[1], se[1] = est(rec[2], rec[3], 1.0 / S0)
    if eta > 0.0:
        value[2], se[2] = est(rec[5], rec[6], 1.0 / (S0 * S0 * (math.exp(eta) - math.exp(-eta))))
    value[3], se[3] = est(rec[2] - rec[0], rec[4], T)
    value[4], se[4] = est(rec[2], rec[3], -T)
    j = 0
    for k, b in enumerate(bump5):
        if b > 0.0:
            value[5 + k], se[5 + k] = est(rec[7 + 2 * j], rec[8 + 2 * j], 1.0 / (2.0 * b))
            j += 1
    return value, se, rec[7 + 2 * P], (rec[8 + 2 * P] / N if N else 0.0)


def restated_estimate(n_paths, chunk, rng, name="F", n_steps=STAT_STEPS, strikes=STAT_STRIKES, eta=ETA, bumps=BUMPS):
    """{strike: (value[10], std_err[10])} of the float64 restatement on numpy normals of rng, a chunk of paths at a
    time; every strike is priced on the same paths"""
    ws = walks(name, bumps)
    total = {s: np.zeros(STATS) for s in strikes}
    for lo in range(0, n_paths, chunk):
        m = min(chunk, n_paths - lo)
        z, zv = rng.standard_normal((n_steps, m)), rng.standard_normal((n_steps, m))
        got = [hr.samples(z, zv, hr.S0, strikes[0][0], hr.T_, hr.R, p, strikes[0][1]) for _, p in ws]
        for K, payoff in strikes:
            rows = rows_from_state(got[0]["S_T"], [payoff_of(g["S_T"], K, payoff) for g in got[1:]], K, payoff, eta)
            total[(K, payoff)] += record(rows, got[0]["trunc"].sum(), got[0]["rv"].sum())
    return {s: finalize(total[s], hr.S0, hr.R, hr.T_, eta, bump_list(bumps))[:2] for s in strikes}


def measure_bias(n_paths=2 ** 22, chunk=2 ** 17, seed=20261021, closed_form=None):
    """{strike: [b_k]}: |restated - closed form| + 4 SE of the restatement at input F and STAT_STEPS steps"""
    est = restated_estimate(n_paths, chunk, np.random.default_rng(seed))
    out = {}
    for (K, payoff), (value, se) in est.items():
        want = closed_form(K, payoff)
        out[(K, payoff)] = [abs(v - w) + 4.0 * s for v, w, s in zip(value, want, se)]
        for k, name in enumerate(NAMES):
            print(f"K {K} payoff {payoff} {name:6s}: closed {want[k]:+.6f} restated {value[k]:+.6f} SE {se[k]:.6f} "
                  f"b {out[(K, payoff)][k]:.6f}")
    return out


if __name__ == "__main__":
    import importlib
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    hg = importlib.import_module("monte-carlo-project-cuda_amd.heston_greeks")
    q, v0, kappa, theta, xi, rho = hr.params("F")
    b = measure_bias(closed_form=lambda K, payoff: hg.greeks_closed_form(
        hr.S0, K, hr.T_, hr.R, q, v0, kappa, theta, xi, rho, payoff, ETA, bump_list(BUMPS)))
    for s, v in b.items():
        print(f"    {s}: [" + ", ".join(f"{x:.3e}" for x in v) + "],")
