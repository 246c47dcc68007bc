"""What tests/test_heston_cpu.py and tests/test_gpu_heston.py share beyond the restatement: the precision spread of the
restatement on each input, measured on the CPU, and the elementwise tolerances of the GPU tests taken from it.

The rule: a kernel is compared with the float64 restatement, and may differ from it by four
times what the restatement itself moves when its precision changes — float64 against longdouble for an fp64 kernel,
float32 against float64 for an fp32 kernel — on 256 paths x 50 steps of that input under the kernel's own draws, with a
floor per quantity.  The floors: 1e-11 S0 (fp64) and 2e-3 (fp32) for S_T and y, which are prices at a spot of 100; for
the variance v_n and the average variance, which are pure numbers of the order of 0.04, the same floors per unit of
notional, 1e-11 and 2e-5."""
import numpy as np

import heston_restate as hr
from deep_inputs import SHALLOW

F64, F32 = 64, 32
NP_T = {F64: np.float64, F32: np.float32}
WIDER = {F64: np.longdouble, F32: np.float64}
FLOOR = {F64: {"S_T": 1e-11 * hr.S0, "y": 1e-11 * hr.S0, "v_n": 1e-11, "rv": 1e-11},
         F32: {"S_T": 2e-3, "y": 2e-3, "v_n": 2e-5, "rv": 2e-5}}
SPREAD_PATHS, SPREAD_STEPS = 256, 50
NEAR_ZERO = 1e-6   # a path whose restated |v_i| comes this close to 0 may count another number of truncated steps in fp32
NEAR_CAP = 0.02    # at most this share of a case may be such paths

_restated = {}


def restate(prec, name, n_steps, where, n, strike, dtype, **changes):
    """one restatement per (case, dtype), shared by every test that needs it and left unchanged.  where: (seed, first
    global path id, ..); strike: (K, payoff)"""
    key = (prec, name, n_steps, where[:2], n, strike, np.dtype(dtype).name, tuple(sorted(changes.items())))
    if key not in _restated:
        z, zv = hr.draws(prec, where[0], where[1], n, n_steps)
        _restated[key] = hr.samples(z, zv, hr.S0, strike[0], hr.T_, hr.R, hr.params(name, **changes), strike[1], dtype)
    return _restated[key]


_spread = {}


def spread(prec, name):
    """{quantity: largest difference between the restatement in the kernel's precision and in the wider one} over the
    three strikes on 256 paths x 50 steps of the input under the draws of that precision"""
    if (prec, name) not in _spread:
        worst = dict.fromkeys(("S_T", "y", "v_n", "rv"), 0.0)
        for strike in hr.STRIKES:
            own = restate(prec, name, SPREAD_STEPS, SHALLOW, SPREAD_PATHS, strike, NP_T[prec])
            wide = restate(prec, name, SPREAD_STEPS, SHALLOW, SPREAD_PATHS, strike, WIDER[prec])
            for k in worst:
                d = np.abs(own[k].astype(np.longdouble) - wide[k].astype(np.longdouble))
                worst[k] = max(worst[k], float(d.max()))
        _spread[(prec, name)] = worst
    return _spread[(prec, name)]


def tolerance(prec, name):
    """{quantity: absolute tolerance per element}: 4 x the spread of that input, floored"""
    s = spread(prec, name)
    return {k: max(4.0 * s[k], FLOOR[prec][k]) for k in s}
