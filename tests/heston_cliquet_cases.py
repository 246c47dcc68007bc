"""What tests/test_heston_cliquet_cpu.py and tests/test_gpu_heston_cliquet.py share beyond the restatement: the shapes,
the jobs, one restatement per case, and the elementwise tolerance of the GPU tests, taken from the restatement alone.

The rule (as tests/test_gpu_cliquet.py applies it): a kernel is compared with the float64
restatement and may differ from it by four times the largest difference between the two restatements — float64 against
longdouble for an fp64 kernel, float32 against float64 for an fp32 kernel — over all jobs on the first shape of that
input under the kernel's own draws, floored at tests/test_gpu_cliquet.py's 1e-13 (fp64) / 2e-5 (fp32) per unit of
notional.  A path whose restated A lies within that tolerance of a global bound may be counted either way; such paths
are at most 2 % of any case."""
import numpy as np

import heston_cliquet_restate as hq
import heston_restate as hr
from deep_inputs import DEEP, SHALLOW

F64, F32 = 64, 32
NP_T = {F64: np.float64, F32: np.float32}
WIDER = {F64: np.longdouble, F32: np.float64}
FLOOR = {F64: 1e-13, F32: 2e-5}
N_LOCAL = 256
NEAR_CAP = 0.02
INF = float("inf")
T_, R = hr.T_, hr.R

# (n_steps, reset_every, first_period, where); the tolerance is taken from the first
FIRST_SHAPE = (48, 4, 1, SHALLOW)
SHAPES = (FIRST_SHAPE,
          (6, 1, 1, SHALLOW), (6, 2, 2, SHALLOW), (6, 3, 1, SHALLOW), (6, 6, 1, SHALLOW),   # a reset on every position of
                                                                                            # a Philox block; a period longer than one
          (5, 5, 1, SHALLOW), (3, 1, 3, SHALLOW), (1, 1, 1, SHALLOW),   # every remainder of the last block; shorter than a block
          (50, 10, 5, SHALLOW), (7, 1, 2, DEEP))
# (kind, local_floor, local_cap, global_floor, global_cap).  The local bounds bind on a fair share of the periods
# (a month at a volatility of 0.2 moves by 0.058); no sum of them is a global bound, so a path lands on a global bound
# only through the clip of A itself.
JOBS = ((hq.SUM, -0.03, 0.05, 0.013, 0.107),      # both global bounds
        (hq.SUM, 0.0, 0.04, -INF, INF),
        (hq.SUM, -INF, INF, -INF, INF),
        (hq.COMPOUND, -0.03, 0.05, 0.013, INF),
        (hq.COMPOUND, -1.0, INF, -INF, INF),
        (hq.VARIANCE, -INF, INF, -INF, 0.047),
        (hq.VARIANCE, -INF, INF, -INF, INF))
# input -> the precisions it runs elementwise in (under H's truncation fp32 paths diverge pathwise)
MODELS = (("F", (F64, F32)), ("N", (F64, F32)), ("H", (F64,)))


def shape_name(shape):
    return f"{shape[0]}-{shape[1]}-{shape[2]}" + ("-deep" if shape[3] == DEEP else "")


def job_name(job):
    return "-".join(str(x) for x in job)


_restated = {}


def restate(prec, name, job, shape, dtype, n=N_LOCAL, **changes):
    """one restatement per (case, dtype), shared by every test that needs it and left unchanged"""
    n_steps, reset_every, first, where = shape
    key = (prec, name, job, shape[:3], where[:2], n, np.dtype(dtype).name, tuple(sorted(changes.items())))
    if key not in _restated:
        z, zv = hr.draws(prec, where[0], where[1], n, n_steps)
        _restated[key] = hq.samples(z, zv, T_, R, hr.params(name, **changes), job[0], reset_every, first, *job[1:],
                                    dtype=dtype)
    return _restated[key]


def compare(prec, name, job, shape):
    """(restated samples to compare with, restatement in the kernel's precision, largest difference between the two
    restatements) — CPU only.  Every kernel is compared with the float64 restatement."""
    own, other = restate(prec, name, job, shape, NP_T[prec]), restate(prec, name, job, shape, WIDER[prec])
    spread = float(np.abs(own["y"].astype(np.longdouble) - other["y"].astype(np.longdouble)).max())
    return (own if prec == F64 else other), own, spread


_spread = {}


def measured_spread(prec, name):
    """the largest restatement difference over all jobs on the first shape"""
    if (prec, name) not in _spread:
        _spread[(prec, name)] = max(compare(prec, name, job, FIRST_SHAPE)[2] for job in JOBS)
    return _spread[(prec, name)]


def tolerance(prec, name):
    """absolute tolerance per element, per unit of notional.  From the restatement alone."""
    return max(4.0 * measured_spread(prec, name), FLOOR[prec])


def near(want, job, tol):
    """per path: the restated A lies within tol of the global floor / of the global cap"""
    A = np.asarray(want["A"], dtype=np.float64)
    return np.abs(A - job[3]) <= tol, np.abs(A - job[4]) <= tol
