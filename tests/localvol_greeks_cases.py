"""The inputs, the restatements and the tolerance of the elementwise tests of mcamd_price_localvol_greeks, shared by
tests/test_gpu_localvol_greeks.py (which runs the kernels on them) and tests/test_localvol_greeks_cpu.py (which checks,
without a device, that the restatement's own rounding stays under half the tolerance and under the exclusion cap).

Inputs.  1024 paths per case on normals drawn from the oracle's rocRAND-exact generator for (seed, global path id,
block).  BASE: the surface SKEW (4 x 65 on [-1.47, 1.53], so that X_0 = 0 lies mid-cell) at 50, 1, 2, 3 and 5 steps on
the shallow ids and 7 steps on the deep ones — every remainder of a Philox block in both precisions — with r = 0.1,
q = 0.03, S0 = K = 100, call and put, gamma_bump in {0, 0.01}, n_vega_buckets in {0, 3, 8} (3 does not divide 50; 8
exceeds 5 steps).  MORE: [-0.047, 0.053], which more than 40 % of the paths leave (s' = 0), 1 x 2, 16 x 128, and the
on-node grid [-1.5, 1.5], where delta and gamma are compared with the restatement of the kernel's own precision only.

Tolerance per path and estimator (tolerance()): the larger of
  4 x spread_e x mean |q_e| of the case, spread_e the largest difference between two restatements (float64 against
      longdouble for fp64 kernels, float32 against float64 for fp32 kernels) over the kept paths of the 50-step BASE
      cases, relative to the mean |q_e| of its case, and
  floor x max(|q_e|, mean |q_e|), floor = 1e-10 (fp64), 2e-5 for the price and 2e-3 for the others (fp32);
gamma is held to 2 tol_delta / (S+ - S-) in either precision.  Everything comes from the restatement alone.
A path is left out of an estimator when S_T of any walk its sample uses lies within MARGIN = 1e-4 K of the strike in
either restatement (the indicator is a discontinuity no arithmetic reproduces to the last bit): at most 1 % of a case."""
import itertools

import numpy as np

import localvol_greeks_restate as gr
from deep_inputs import DEEP, SHALLOW

F32, F64 = 32, 64
NP_T = {F64: np.float64, F32: np.float32}
OTHER_T = {F64: np.longdouble, F32: np.float64}
BASE = dict(S0=100.0, K=100.0, r=0.1, T=1.0)
Q_DIV = 0.03
N_LOCAL = 1024
MARGIN, CAP = 1e-4, 0.01
ETA = 0.01
FLOOR = {F64: (1e-10, 1e-10), F32: (2e-5, 2e-3)}   # (price, the others)
INPUTS = ((50, SHALLOW), (1, SHALLOW), (2, SHALLOW), (3, SHALLOW), (5, SHALLOW), (7, DEEP))


def skew(n_t, n_x, x_min, x_max, lo=0.18, step=0.04):
    x = np.linspace(x_min, x_max, n_x)
    return (n_t, n_x, x_min, x_max), np.array([(lo + step * j) * (1.0 + 0.5 * np.exp(-x)) / 1.5 for j in range(n_t)])


SURFACES = {
    "skew": skew(4, 65, -1.47, 1.53),
    "narrow": skew(4, 65, -0.047, 0.053),
    "two": ((1, 2, -1.5, 1.5), np.array([[0.30, 0.14]])),
    "full": skew(16, 128, -1.47, 1.53, 0.15, 0.01),
    "node": skew(4, 65, -1.5, 1.5),
}

# (surface, n_steps, where, prec, payoff, eta, n_buckets)
BASE_CASES = [("skew", n_steps, where, prec, payoff, eta, B)
              for (n_steps, where), prec, payoff, eta, B in
              itertools.product(INPUTS, (F64, F32), (gr.CALL, gr.PUT), (0.0, ETA), (0, 3, 8))]
MORE_CASES = [(surface, 50, SHALLOW, prec, payoff, eta, B)
              for surface in ("narrow", "two", "full") for prec in (F64, F32) for payoff in (gr.CALL, gr.PUT)
              for eta, B in ((ETA, 3), (0.0, 8))] + \
             [("node", 50, SHALLOW, prec, payoff, ETA, 0) for prec in (F64, F32) for payoff in (gr.CALL, gr.PUT)]
ALL_CASES = BASE_CASES + MORE_CASES


def case_id(case):
    surface, n_steps, where, prec, payoff, eta, B = case
    return f"{surface}-{n_steps}{'-deep' if where == DEEP else ''}-f{prec}-{'put' if payoff else 'call'}-eta{eta}-B{B}"


_normals = {}


def normals(prec, seed, first, n, n_steps):
    """[n_steps, n] normals of global paths first..first+n-1, as the kernels draw them (as float64 values)"""
    from oracle import pyoracle as o
    key = (prec, seed, first, n, n_steps)
    if key not in _normals:
        per, draw = (2, o.normal2_f64) if prec == F64 else (4, o.normal4_f32)
        blocks = -(-n_steps // per)
        z = np.empty((blocks * per, n))
        for p in range(n):
            for k in range(blocks):
                z[k * per:(k + 1) * per, p] = draw(seed, first + p, k)
        _normals[key] = z[:n_steps]
    return _normals[key]


_walks, _formed = {}, {}


def restate(surface, n_steps, where, prec, payoff, B, dtype):
    """one restatement per (inputs, buckets, payoff, dtype), always with the gamma walks, shared and left unchanged"""
    name = np.dtype(dtype).name
    wkey = (surface, n_steps, where, prec, B, name)
    if wkey not in _walks:
        grid, sigma = SURFACES[surface]
        z = normals(prec, where[0], where[1], N_LOCAL, n_steps)
        _walks[wkey] = gr.walks(z, BASE["T"], BASE["r"], Q_DIV, grid, sigma, B, ETA, dtype)
    key = wkey + (payoff,)
    if key not in _formed:
        main, up, down = _walks[wkey]
        _formed[key] = gr.form(main, BASE["S0"], BASE["K"], BASE["T"], payoff, dtype, up, down, ETA)
    return _formed[key]


def rows_of(eta, B):
    """the sample rows a case compares: gamma only with a bump"""
    return [e for e in range(gr.N_EST + B) if e != gr.GAMMA or eta > 0.0]


def compare(case):
    """(own, other, keep, keep3): the restatements in the kernel's precision and in the wider one, and the paths kept
    for the estimators of the main walk and for gamma"""
    surface, n_steps, where, prec, payoff, eta, B = case
    own = restate(surface, n_steps, where, prec, payoff, B, NP_T[prec])
    other = restate(surface, n_steps, where, prec, payoff, B, OTHER_T[prec])
    keep = (own["margin"] >= MARGIN) & (other["margin"] >= MARGIN)
    keep3 = (own["margin3"] >= MARGIN) & (other["margin3"] >= MARGIN)
    return own, other, keep, keep3


def want_of(case):
    """what a kernel's samples are compared with: an fp64 kernel with the float64 restatement, an fp32 kernel with the
    float64 one too — but delta and gamma on the on-node grid with the restatement of the kernel's own precision"""
    own, other, _, _ = compare(case)
    prec = case[3]
    want = np.array((own if prec == F64 else other)["q"], dtype=np.float64)
    if case[0] == "node":
        want[gr.DELTA], want[gr.GAMMA] = own["q"][gr.DELTA], own["q"][gr.GAMMA]
    return want


def klass(e):
    return min(e, gr.N_EST)   # every bucket shares one spread


def relative_spread(case):
    """per estimator class: the largest kept |own - other| over mean |q_e| of the case (0 where the mean is 0)"""
    own, other, keep, keep3 = compare(case)
    eta, B = case[5], case[6]
    out = np.zeros(gr.N_EST + 1)
    for e in rows_of(eta, B):
        k = keep3 if e == gr.GAMMA else keep
        scale = float(np.abs(np.asarray(other["q"][e], dtype=np.float64)).mean())
        if scale > 0.0 and k.any():
            d = float(np.abs(np.asarray(own["q"][e] - other["q"][e], dtype=np.float64))[k].max())
            out[klass(e)] = max(out[klass(e)], d / scale)
    return out


_spread = {}


def measured_spread(prec):
    """the largest relative restatement difference per estimator class over the 50-step BASE cases of one precision"""
    if prec not in _spread:
        cases = [c for c in BASE_CASES if c[1] == 50 and c[3] == prec and c[5] > 0.0]
        _spread[prec] = np.max([relative_spread(c) for c in cases], axis=0)
    return _spread[prec]


def tolerance(case, want):
    """[rows, paths] absolute tolerances for `want` (all 6 + B rows; the gamma row is meaningless without a bump)"""
    prec, eta = case[3], case[5]
    spread = measured_spread(prec)
    tol = np.zeros_like(want)
    for e in range(want.shape[0]):
        mean = np.abs(want[e]).mean()
        floor = FLOOR[prec][0 if e == gr.PRICE else 1]
        tol[e] = np.maximum(4.0 * spread[klass(e)] * mean, floor * np.maximum(np.abs(want[e]), mean))
    S_up, S_dn = BASE["S0"] * np.exp(ETA), BASE["S0"] * np.exp(-ETA)
    tol[gr.GAMMA] = 2.0 * tol[gr.DELTA] / (S_up - S_dn)
    return tol
