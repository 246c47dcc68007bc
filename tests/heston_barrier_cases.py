"""What tests/test_heston_barrier_cpu.py and tests/test_gpu_heston_barrier.py share beyond the restatement: the inputs,
one cached restatement per case, the left-out rule, and the precision spread of the restatement, measured on the CPU,
from which the elementwise tolerances of the GPU tests are taken.

Inputs: heston_restate's market and models F, N and H; B = 90 for the down kinds and 110 for the up kinds; K = 100, call
and put; 1024 paths at global ids 5003.. under seed 77 with 50, 3, 5 and 1 steps, and 7 steps on the deep ids and seed
of tests/deep_inputs.py.  H is compared elementwise in fp64 only.

The left-out rule: the hit test is a strict comparison, so a path whose restated X_i comes
within MARGIN = 2e-5 of b at any step end, in either of the two restatement precisions compared, may be hit in one
precision and not in the other; it is left out of elementwise comparisons.  At most LEFT_CAP = 3 % of a case may be.

The tolerances (section 13's rule): a kernel is compared with the float64 restatement and may differ from it by four
times what the restatement itself moves when its precision changes — float64 against longdouble for an fp64 kernel,
float32 against float64 for an fp32 kernel — over the kept paths of the 16 kind x monitoring x payoff cases at 1024
paths x 50 steps of that input, floored at heston_cases.FLOOR's values for y, S_T and v_n and at 1e-11 / 2e-5 for the
weight w and the mean variance."""
import numpy as np

import barrier_restate as br
import heston_barrier_restate as hbr
import heston_cases as hc
import heston_restate as hr
from deep_inputs import DEEP, SHALLOW

F64, F32 = hc.F64, hc.F32
NP_T, WIDER = hc.NP_T, hc.WIDER
MARGIN = 2e-5
LEFT_CAP = 0.03
N_PATHS = 1024
STRIKE = 100.0
LEVEL = {br.DOWN_OUT: 90.0, br.DOWN_IN: 90.0, br.UP_OUT: 110.0, br.UP_IN: 110.0}
# (n_steps, where)
SHAPES = ((50, SHALLOW), (3, SHALLOW), (5, SHALLOW), (7, DEEP), (1, SHALLOW))
# (input, the precisions it is compared in elementwise)
ELEMENTWISE = (("F", (F64, F32)), ("N", (F64, F32)), ("H", (F64,)))
# (kind, monitoring, payoff)
CASES = tuple((kind, mon, payoff) for kind in br.KINDS for mon in (br.DISCRETE, br.CONTINUOUS)
              for payoff in (br.CALL, br.PUT))
FLOOR = {F64: dict(hc.FLOOR[F64], w=1e-11, mv=1e-11), F32: dict(hc.FLOOR[F32], w=2e-5, mv=2e-5)}
QUANTITIES = ("y", "S_T", "v_n", "w", "mv")
SPREAD_SHAPE = SHAPES[0]

_restated = {}


def restate(prec, name, n_steps, where, n, case, dtype, level=None, **changes):
    """one restatement per (case, dtype), shared by every test that needs it and left unchanged.  where: (seed, first
    global path id, ..); case: (kind, monitoring, payoff); the level is LEVEL's unless given"""
    kind, mon, payoff = case
    B = LEVEL[kind] if level is None else level
    key = (prec, name, n_steps, where[:2], n, case, np.dtype(dtype).name, B, tuple(sorted(changes.items())))
    if key not in _restated:
        z, zv = hr.draws(prec, where[0], where[1], n, n_steps)
        _restated[key] = hbr.samples(z, zv, hr.S0, STRIKE, B, hr.T_, hr.R, hr.params(name, **changes), kind, payoff,
                                     mon, dtype)
    return _restated[key]


def mean_variance_per_path(got):
    """vs / the counted steps of each path, in float64 (longdouble stays): every path counts its first step"""
    wide = np.longdouble if got["vs"].dtype == np.dtype(np.longdouble) else np.float64
    return got["vs"].astype(wide) / got["counted"].astype(wide)


def kept(prec, name, n_steps, where, n, case, **changes):
    """the paths of a case that elementwise comparisons keep: min_i |X_i - b| >= MARGIN in the kernel's precision and in
    the wider one (the two restatements the spread compares), and in float64 (what the kernel is compared with).  The
    distances depend on the path and the level alone, so one case per side of the spot serves all eight of that side."""
    side = (br.UP_OUT if br.is_up(case[0]) else br.DOWN_OUT, br.DISCRETE, br.CALL)
    keep = np.ones(n, dtype=bool)
    for dtype in {NP_T[prec], WIDER[prec], np.float64}:
        keep &= restate(prec, name, n_steps, where, n, side, dtype, **changes)["min_abs_d"] >= MARGIN
    return keep


def exact_inputs(name):
    """the input with rho = 0 and r = q = 0.02: the variance path reads z' alone, and given it X is a Brownian motion
    with drift -1/2 in the clock sum_i v+_i dt.  Returns (r, heston_params)"""
    return 0.02, hr.params(name, q=0.02, rho=0.0)


def conditional_expectation(capi, clock, kind, payoff):
    """E[y | variance path] of the continuously monitored sample at rho = 0, r = q, per path: the closed form of the
    constant-volatility barrier (mcamd_barrier_price_f64) at r = 0 and v = sqrt(clock / T)"""
    import ctypes as C
    L, p, out = capi.load(), C.c_double(), np.empty(len(clock))
    B, price = LEVEL[kind], C.byref(p)
    for j, v in enumerate(np.sqrt(np.asarray(clock, dtype=np.float64) / hr.T_).tolist()):
        rc = L.mcamd_barrier_price_f64(hr.S0, STRIKE, B, hr.T_, 0.0, v, kind, payoff, price)
        assert rc == 0, (rc, v)
        out[j] = p.value
    return out


def mean_in_standard_errors(y, c):
    """(mean(y - c), its standard error) on the same paths"""
    d = np.asarray(y, dtype=np.float64) - c
    return float(d.mean()), float(d.std(ddof=1) / np.sqrt(len(d)))


_spread = {}


def spread(prec, name):
    """{quantity: largest difference between the restatement in the kernel's precision and in the wider one} over the
    kept paths of the 16 cases at 1024 paths x 50 steps of the input under the draws of that precision"""
    if (prec, name) not in _spread:
        n_steps, where = SPREAD_SHAPE
        worst = dict.fromkeys(QUANTITIES, 0.0)
        for case in CASES:
            own = restate(prec, name, n_steps, where, N_PATHS, case, NP_T[prec])
            wide = restate(prec, name, n_steps, where, N_PATHS, case, WIDER[prec])
            keep = kept(prec, name, n_steps, where, N_PATHS, case)
            pairs = {k: (own[k], wide[k]) for k in ("y", "S_T", "v_n", "w")}
            pairs["mv"] = (mean_variance_per_path(own), mean_variance_per_path(wide))
            for k, (a, b) in pairs.items():
                d = np.abs(a.astype(np.longdouble) - b.astype(np.longdouble))[keep]
                worst[k] = max(worst[k], float(d.max()))
        _spread[(prec, name)] = worst
    return _spread[(prec, name)]


def tolerance(prec, name):
    """{quantity: absolute tolerance per element}: 4 x the spread of that input, floored"""
    s = spread(prec, name)
    return {k: max(4.0 * s[k], FLOOR[prec][k]) for k in s}
