"""The inputs of the path-by-path window tests of tests/test_gpu_window.py, their restatements (tests/window_restate.py),
the margin around the barrier, the tolerances and the caps.  No kernel runs here: tests/test_window_cpu.py checks all of
it on the CPU.

mcamd_price_paths has no per-path output, so a path is looked at through a shard of one: with n_paths_local = 1 and
path_offset = id the record is (y, y^2, c, c^2, y c, 1) of that path's sample.

Option: S0 = K = 100, r = 0.1, v = 0.2, T = 1.  N_PATHS consecutive paths from SHALLOW, DEEP (tests/deep_inputs.py) or
STRADDLE (ids 2^32 - 101 .. of tests/test_gpu_philox_head.py's job: one wavefront walks the plain Philox rounds).

  simulated steps    window     B     where
  1, 2, 3, 5, 6, 7   [1, 2] up to 3 steps, else [1, 4]   104   all six SHALLOW, 3 and 7 DEEP, 2 and 6 STRADDLE
  33                 [2, 9]     104   SHALLOW, STRADDLE   (the first length that takes one path per thread)
  61                 [2, 9]     104   SHALLOW; DEEP with B = 102.75 (below)   (the nested-MC shape of tests/test_gpu_parity.py)
  100                [10, 50]   120   SHALLOW, DEEP, STRADDLE   (the reference's bullet window)
  63 of 100          [5, 60]    120   SHALLOW, restart from Ik = 4, Sk = 93.5, Tk = 37
  33, dt = 1/50      [2, 9]     104   SHALLOW
1, 2, 3, 5, 6, 7 steps leave 1, 2, 3, 1, 2, 3 steps in the last Philox block in fp32 and 1, 0, 1, 1, 0, 1 in fp64;
fewer than 4 (fp32) or 2 (fp64) steps have no full block.  Forms: {log form, MCAMD_FLAG_PRODUCT_FORM} x {plain,
antithetic, control variate, both}; the window-less antithetic forms at 1, 3, 7 steps (SHALLOW; 3 also DEEP).

Nested-MC cases (B = 104; outer rows under OUTER_SEED of the place, inner streams under the place's seed):
  edges        paths 3 .. 11 of 20 (a partial first and last pool of 8), 13 steps (0 .. 12 to go: every remainder, no
               full block up to 3 / 1 to go), 130 inner paths (two wavefronts and two lanes), window [1, 4], both layouts
  compaction   9 paths x 30 steps x 130 inner, window [2, 6], step-major: a pool of 1040 paths hands over, parks,
               resumes full wavefronts and drains
  deep         paths 2^33 + 12 345 .. + 2 of 2^40, 7 steps, 70 inner, window [1, 4]
  windowless   edges with use_window = 0

MARGIN (natural-log units): a step with |ln(S_t / B)| < MARGIN may be compared either way (window_restate.walk).  2e-5,
the figure of tests/test_gpu_barrier.py; it has to be at least four times the largest |ln S_t| difference between the two
restatements of any case (log_spread(); asserted in tests/test_window_cpu.py, which prints the measured values).

Tolerance of a sample (greeks_cases' rule, per case): the larger of four times the largest elementwise difference
between the two restatements of the case over its decided samples — float64 and longdouble for an fp64 kernel, float32
and float64 for an fp32 kernel — and FLOOR (1e-10 / 2e-5) times max(|y|, mean |y| of the case).  The control c takes the
same rule on the scale of S_T; c^2 and y c take what follows from the two: 2 |c| tol_c + tol_c^2 and
|y| tol_c + |c| tol_y + tol_y tol_c.  Tolerance of a nested-MC point: exp(-rT) times the mean of its inner paths'
tolerances plus one ulp of the output type at the price; the point passes when lo - tol <= price <= hi + tol.

Caps (conditions on the inputs, asserted on the restatement alone): at most MAX_UNDECIDED of a price_paths case's samples
undecided; at least MIN_FREE of a nested-MC case's priced points without an undecided inner path; the summed width
hi - lo of a case (a sample's largest minus its smallest candidate, a point's interval) at most MAX_WIDTH of its summed
hi, for every price_paths case and form and every nested-MC case; at least MIN_PAYING of a price_paths case's samples
non-zero; a non-zero point at every step count to go >= 1 of a nested-MC case."""
import collections
import importlib

import numpy as np

import window_restate as wr
from deep_inputs import DEEP, DEEP_SEED, SEED, SHALLOW

capi = importlib.import_module("monte-carlo-project-cuda_amd").capi

assert (capi.F32, capi.F64, capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE) == (wr.F32, wr.F64, wr.ANTITHETIC,
                                                                                 wr.CONTROL_VARIATE)
PRECS = (capi.F64, capi.F32)
OPTION = dict(S0=100.0, T=1.0, K=100.0, r=0.1, v=0.2)
N_PATHS = 256
STRADDLE = (2 ** 40 + 77, 2 ** 32 - 101, 2 ** 33)    # SEED, FIRST, JOB of tests/test_gpu_philox_head.py
PLACE_NAMES = {SHALLOW: "", DEEP: "-deep", STRADDLE: "-straddle"}
MARGIN = 2e-5
FLOOR = {capi.F64: 1e-10, capi.F32: 2e-5}
OTHER = {capi.F64: np.longdouble, capi.F32: np.float64}   # the second restatement of the spread
OWN = {capi.F64: np.float64, capi.F32: np.float32}
MAX_UNDECIDED, MIN_FREE, MAX_WIDTH, MIN_PAYING = 0.005, 0.80, 0.01, 0.02

A, CV, PF = capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_PRODUCT_FORM
VR = {"plain": 0, "anti": A, "cv": CV, "anti-cv": A | CV}
FORMS = {f"{vr}{'-product' if pf else ''}": flags | pf for pf in (0, PF) for vr, flags in VR.items()}
WINDOWLESS_FORMS = {k: v for k, v in FORMS.items() if v & A}

Case = collections.namedtuple("Case", "name extra n_steps where")


def _window(P1, P2, B, **more):
    return dict(B=B, P1=P1, P2=P2, use_window=1, **more)


def _case(kind, extra, n_steps, where):
    return Case(f"{kind}-{n_steps}{PLACE_NAMES[where]}", extra, n_steps, where)


def _short(n):
    return _window(1, 2 if n <= 3 else 4, 104.0)


# at B = 104 one undecided fp64 sample of the deep 61-step case alone is 2.1 % of the case's summed candidates: beyond
# MAX_WIDTH, so the input moves (not the cap).  At 102.75 fp64 has no undecided sample and fp32 has one under the
# antithetic forms, 0.85 % of the sum: the one price_paths case whose fp32 kernels meet the candidate branch
B_61_DEEP = 102.75
WINDOW_CASES = (
    [_case("w", _short(n), n, SHALLOW) for n in (1, 2, 3, 5, 6, 7)] +
    [_case("w", _short(n), n, DEEP) for n in (3, 7)] + [_case("w", _short(n), n, STRADDLE) for n in (2, 6)] +
    [_case("w", _window(2, 9, 104.0), 33, w) for w in (SHALLOW, STRADDLE)] +
    [_case("w", _window(2, 9, 104.0), 61, SHALLOW), _case("w", _window(2, 9, B_61_DEEP), 61, DEEP)] +
    [_case("w", _window(10, 50, 120.0), 100, w) for w in (SHALLOW, DEEP, STRADDLE)])
RESTART_CASE = _case("restart", _window(5, 60, 120.0, Ik=4, Sk=93.5, Tk=37), 100, SHALLOW)
DT_CASE = _case("dt", _window(2, 9, 104.0, dt=1.0 / 50), 33, SHALLOW)
WINDOW_CASES += [RESTART_CASE, DT_CASE]
WINDOWLESS_CASES = [_case("nw", {}, n, SHALLOW) for n in (1, 3, 7)] + [_case("nw", {}, 3, DEEP)]
PP_CASES = [(c, f) for c in WINDOW_CASES for f in FORMS] + [(c, f) for c in WINDOWLESS_CASES for f in WINDOWLESS_FORMS]
CASE_BY_NAME = {c.name: c for c in WINDOW_CASES + WINDOWLESS_CASES}


def option(case):
    return capi.make_option(**dict(OPTION, **case.extra))


def sim(case, prec, flags=0, first=None, n_local=N_PATHS):
    seed, start, job = case.where
    first = start if first is None else first
    return capi.make_sim(max(job, first + n_local), case.n_steps, prec, seed=seed, path_offset=first,
                         n_paths_local=n_local, flags=flags)


_restated = {}


def restated(case, prec, form, dtype, mutate=0):
    """window_restate.price_paths of the case's N_PATHS paths in dtype under the form's variance reduction (the product
    form restates as the log form does); computed once"""
    from oracle import pyoracle
    vr = FORMS[form] & (A | CV)
    key = (case.name, prec, vr, np.dtype(dtype), mutate)
    if key not in _restated:
        _restated[key] = wr.price_paths(pyoracle, option(case), sim(case, prec, vr), dtype, MARGIN, mutate)
    return _restated[key]


def log_spread(case, prec):
    """the largest |ln(S_t / S_start)| difference between the two restatements, over the case's paths, twins and steps"""
    a, b = restated(case, prec, "anti", OWN[prec]), restated(case, prec, "anti", OTHER[prec])
    return max(float(np.abs(m.logs.astype(np.longdouble) - o.logs.astype(np.longdouble)).max())
               for m, o in zip(a.members, b.members))


def _diff(a, b, keep):
    d = np.abs(a.astype(np.longdouble) - b.astype(np.longdouble)).astype(np.float64)
    return float(np.where(keep, d, 0.0).max()) if d.size else 0.0


PPWanted = collections.namedtuple("PPWanted", "want tol_y tol_c spread_y spread_c")


def wanted(case, prec, form):
    """PPWanted: the float64 Samples to compare with, the tolerance of y [n] and of c [n] (None without the control
    variate), and the two measured spreads.  From the restatements alone."""
    want, own, other = restated(case, prec, form, np.float64), restated(case, prec, form, OWN[prec]), \
        restated(case, prec, form, OTHER[prec])
    keep = want.decided
    spread_y = _diff(own.y, other.y, keep)
    y_hi = np.abs(want.cands).max(axis=1)
    tol_y = np.maximum(4.0 * spread_y, FLOOR[prec] * np.maximum(y_hi, np.abs(want.y).mean()))
    tol_c, spread_c = None, 0.0
    if want.c is not None:
        spread_c = _diff(own.c, other.c, np.ones_like(keep))
        tol_c = np.maximum(4.0 * spread_c, FLOOR[prec] * np.maximum(np.abs(want.ctrl), np.abs(want.ctrl).mean()))
    return PPWanted(want, tol_y, tol_c, spread_y, spread_c)


def outside(got, w):
    """[n] bool: the samples `got` [n] that lie beyond tol_y of every candidate of w (a PPWanted)"""
    return (np.abs(got[:, None] - w.want.cands.astype(np.float64)) > w.tol_y[:, None]).all(axis=1)


def nearest_candidate(got, w):
    c = w.want.cands.astype(np.float64)
    return c[np.arange(len(got)), np.abs(got[:, None] - c).argmin(axis=1)]


# ---------------- nested MC ----------------
NmcCase = collections.namedtuple("NmcCase", "name window n_job first n_local n_steps n_inner seed layouts")
OUTER_SEED = {SEED: 4242, DEEP_SEED: 2 ** 41 + 4242}
NMC_EDGES = NmcCase("edges", _window(1, 4, 104.0), 20, 3, 9, 13, 130, SEED, (capi.STEP_MAJOR, capi.PATH_MAJOR))
NMC_COMPACTION = NmcCase("compaction", _window(2, 6, 104.0), 9, 0, 9, 30, 130, SEED, (capi.STEP_MAJOR,))
NMC_DEEP = NmcCase("deep", _window(1, 4, 104.0), 2 ** 40, 2 ** 33 + 12_345, 3, 7, 70, DEEP_SEED, (capi.STEP_MAJOR,))
NMC_WINDOWLESS = NMC_EDGES._replace(name="windowless", window=dict(B=104.0, P1=1, P2=4, use_window=0),
                                    layouts=(capi.STEP_MAJOR,))
NMC_CASES = [NMC_EDGES, NMC_COMPACTION, NMC_DEEP, NMC_WINDOWLESS]
NMC_ROUTES = {"wave": capi.NMC_WAVE_PER_POINT, "block": capi.NMC_BLOCK_PER_POINT,
              "block-plain": capi.NMC_BLOCK_PER_POINT_PLAIN, "fused": None}


def nmc_option(case):
    return capi.make_option(**dict(OPTION, **case.window))


def nmc_outer_sim(case, prec):
    return capi.make_sim(case.n_job, case.n_steps, prec, seed=OUTER_SEED[case.seed], path_offset=case.first,
                         n_paths_local=case.n_local)


def nmc_inner_sim(case, prec, flags=0):
    return capi.make_sim(case.n_job, case.n_steps, prec, seed=case.seed, path_offset=case.first,
                         n_paths_local=case.n_local, n_paths_inner=case.n_inner, flags=flags)


def oracle_params(oracle, opt, sim):
    return oracle.make_params(S0=opt.S0, T=opt.T, K=opt.K, r=opt.r, v=opt.v, B=opt.B, P1=opt.P1, P2=opt.P2,
                              n_paths=sim.n_paths, n_steps=sim.n_steps, n_paths_inner=sim.n_paths_inner, seed=sim.seed,
                              use_window=opt.use_window, Ik=opt.Ik, Sk=opt.Sk, Tk=opt.Tk, dt=opt.dt)


def oracle_rows(oracle, case, prec):
    """(St, counts) [n_local, n_steps]: the outer rows as the oracle stores them (the GPU tests feed the GPU's own).
    The count is kept with use_window = 0 too, where nothing reads it."""
    opt = capi.make_option(**dict(OPTION, **dict(case.window, use_window=1)))
    ref = oracle.mc_paths(oracle_params(oracle, opt, nmc_outer_sim(case, prec)), prec, case.first, case.n_local,
                          want_traj=True, want_counts=True)
    St = ref["traj"].T.astype(OWN[prec])
    return np.ascontiguousarray(St), np.ascontiguousarray(ref["counts"].T)


NmcWanted = collections.namedtuple("NmcWanted", "want tol spread free")


def nmc_wanted(oracle, case, prec, St, counts):
    """NmcWanted of the case's shard from the stored rows St, counts [n_local, n_steps]: the float64 Points, the
    tolerance of every point [n_local, n_steps], the measured spread of the inner payoffs and the points that are held
    to a zero-width interval (priced, no undecided inner path)."""
    opt, sm = nmc_option(case), nmc_inner_sim(case, prec)
    want, own, other = (wr.nmc_points(oracle, opt, sm, St, counts, t, MARGIN) for t in (np.float64, OWN[prec], OTHER[prec]))
    spread = _diff(own.y, other.y, want.decided)
    live = ~want.closed
    mean_y = float(np.abs(want.y[live]).mean()) if live.any() else 0.0
    tol_inner = np.maximum(4.0 * spread, FLOOR[prec] * np.maximum(want.y_hi, mean_y))
    out_t = OWN[prec]
    ulp = np.spacing(np.maximum(np.abs(want.hi), np.abs(want.price)).astype(out_t)).astype(np.float64)
    tol = np.where(live, tol_inner.mean(axis=2) * np.exp(-opt.r * opt.T) + ulp, 0.0)
    return NmcWanted(want, tol, spread, live & (want.undecided == 0))


def nmc_outside(got, w):
    """[n_local, n_steps] bool: the point prices `got` outside [lo - tol, hi + tol]"""
    got = np.asarray(got, dtype=np.float64)
    return (got < w.want.lo - w.tol) | (got > w.want.hi + w.tol)
