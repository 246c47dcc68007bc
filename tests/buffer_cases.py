"""The inputs of tests/test_gpu_buffers.py: where the caller-owned buffers of the array-driven pricer, the bulk normal
fill, the trajectory store, the store pattern and the reductions are placed (alignment, tail, guard bands), the numpy
restatements the results are compared with and the tolerances.  No kernel runs here: tests/test_buffer_cpu.py checks
all of it on the CPU.

placed() puts a buffer of n elements anywhere inside a larger tensor: the slice starts at a chosen `skew` = address
mod 128 and has at least GUARD bytes of poison on each side.  guards() copies the two guard bands as integers and
untouched() compares them with such a copy bit for bit (NaN != NaN, so not as floats).  Poison: NaN for float buffers
(an input kernel that consumed an element beyond n leaves a NaN; an output kernel never produces one), and for the int32
counts the bits of the float -777.25, a negative count.

Array-driven pricer (csrc/aux.hip from_normals_kernel).  Option S0 = K = 100, r = 0.1, v = 0.2, T = 1; N_PATHS = 130
paths (two full 64-row tiles and one of two rows), also the first 1 and 64 of them at 4 and 252 steps; normals
oracle.generate_normals(77, 130 * n_sim, precision), row p = elements p * n_sim .. of them.  A step count is on the VEC
path when a row is a multiple of 16 bytes AND the buffer is 16-byte aligned; rows of 16, 112, 128, 144, 240, 1008 (and
2016) bytes sit at, just under, on, just over, and far from a multiple of the 128-byte line, 1 and 33 steps take the
scalar path whatever the address.  Windows (B = 104): [1, 2] up to 4 steps, [2, 9] for 5 .. 60, [20, 120] from 100;
every case with use_window 0 and 1.  Restart (window_cases.RESTART_CASE's figures): 100 steps, Ik = 4, Sk = 93.5,
window [5, 60], B = 120, with Tk = 37 (63 simulated steps: scalar) and Tk = 36 (64: VEC); a row has n_sim = n_steps - Tk
normals.  Skews of the normals: every multiple of 16 below 128 (VEC with every a.skew) and 4, 8, 12, 20 (fp32) / 8, 24,
120 (fp64), which force the scalar path at a VEC step count.

Tolerance of a payoff (window_cases' rule): the larger of four times the largest difference between the two
restatements of the case over its decided samples (float32 / float64 for fp32, float64 / longdouble for fp64) and FLOOR
times max(|y|, mean |y|); a sample with a step within MARGIN of the barrier whose flip moves its count across P1 or P2 is
undecided and has to equal one of its two candidates.

Trajectory store (csrc/store.hip): V = 4 (fp32) / 2 (fp64) paths per thread, one workgroup covers 256 V paths;
n_local in {1, V - 1, V, V + 1, 2 V - 1, 256 V, 256 V + 1, 256 V + V - 1} x n_steps in {1, 3, 5, 9} (every remainder of
both Philox block sizes), window [1, 4], B = 104, paths 3 .. of a job 10 paths larger, both layouts; the three output
buffers aligned, each alone off by one element, all off, counts absent, payoffs absent.  The rows of 256 V + 1 paths x 9
steps are compared with window_restate.price_paths: a price at the larger of four times the spread of the two
restatements' prices and FLOOR times the price, a per-step flag wherever |ln(S_t / B)| >= MARGIN, payoffs as above."""
import collections
import importlib

import numpy as np

import window_cases as wc
import window_restate as wr

capi = importlib.import_module("monte-carlo-project-cuda_amd").capi

GUARD = 256                    # bytes of poison on each side of a placed buffer, at least
COUNT_POISON = int(np.float32(-777.25).view(np.int32))
ITEM = {capi.F64: 8, capi.F32: 4}
VEC = {capi.F64: 2, capi.F32: 4}   # elements of a 16-byte vector
NP_T = {capi.F64: np.float64, capi.F32: np.float32}


def start_of(base, itemsize, skew):
    """element index at which a buffer inside a tensor at address `base` starts so that its address is `skew` mod 128
    and at least GUARD bytes lie before it"""
    assert skew % itemsize == 0 and base % itemsize == 0 and 0 <= skew < 128
    return (GUARD + (skew - base - GUARD) % 128) // itemsize


def placed(n, torch_dtype, skew, poison, device="cuda"):
    """(whole, view): one tensor filled with `poison` and its n-element slice at address `skew` mod 128, with at least
    GUARD bytes of the tensor on each side.  The start is computed from the tensor's actual address."""
    import torch
    item = torch.empty(0, dtype=torch_dtype).element_size()
    total = int(n) + (2 * GUARD + 128) // item
    if torch_dtype == torch.int32:
        whole = torch.full((total,), int(poison), dtype=torch_dtype, device=device)
    else:
        whole = torch.full((total,), float(poison), dtype=torch_dtype, device=device)
    s = start_of(whole.data_ptr(), item, skew)
    view = whole[s:s + int(n)]
    assert view.data_ptr() % 128 == skew and s * item >= GUARD and (total - s - int(n)) * item >= GUARD
    return whole, view


def _as_int(t):
    import torch
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def guards(whole, view):
    """copies of the two guard bands of `whole` around `view`, as integers"""
    s = view.storage_offset() - whole.storage_offset()
    w = _as_int(whole)
    return w[:s].clone(), w[s + view.numel():].clone()


def untouched(whole, view, before):
    """both guard bands of `whole` around `view` equal `before` = guards(whole, view) taken earlier, bit for bit"""
    import torch
    lo, hi = guards(whole, view)
    return lo.numel() * whole.element_size() >= GUARD and hi.numel() * whole.element_size() >= GUARD and \
        torch.equal(lo, before[0]) and torch.equal(hi, before[1])


# ---------------- array-driven pricer ----------------
N_PATHS = 130
NORMALS_SEED = 77
FN_STEPS = {capi.F32: (4, 28, 32, 36, 60, 252, 1, 33), capi.F64: (2, 14, 16, 18, 30, 126, 252, 1, 33, 4)}
SMALL_JOBS = (1, 64)            # path counts beside N_PATHS ...
SMALL_JOB_STEPS = (4, 252)      # ... at these step counts
SKEWS_16 = tuple(range(0, 128, 16))
SKEWS_ELEMENT = {capi.F32: (4, 8, 12, 20), capi.F64: (8, 24, 120)}

FnCase = collections.namedtuple("FnCase", "name n_steps extra")


def _window_of(n_steps):
    if n_steps <= 4:
        return dict(B=104.0, P1=1, P2=2)
    return dict(B=104.0, P1=2, P2=9) if n_steps <= 60 else dict(B=104.0, P1=20, P2=120)


def fn_cases(prec):
    restart = {k: v for k, v in wc.RESTART_CASE.extra.items() if k != "use_window"}
    assert restart == dict(B=120.0, P1=5, P2=60, Ik=4, Sk=93.5, Tk=37) and wc.RESTART_CASE.n_steps == 100
    return [FnCase(f"n-{n}", n, _window_of(n)) for n in FN_STEPS[prec]] + \
        [FnCase(f"restart-{100 - tk}-of-100", 100, dict(restart, Tk=tk)) for tk in (37, 36)]


def n_sim(case):
    return case.n_steps - case.extra.get("Tk", 0)


def on_vec_path(case, prec, skew):
    return n_sim(case) % VEC[prec] == 0 and skew % 16 == 0


def job_sizes(case):
    return (N_PATHS,) + (SMALL_JOBS if case.n_steps in SMALL_JOB_STEPS and "Tk" not in case.extra else ())


def fn_option(case, use_window):
    return capi.make_option(**dict(wc.OPTION, use_window=use_window, **case.extra))


def fn_sim(case, prec, n=N_PATHS):
    return capi.make_sim(n, case.n_steps, prec)


_normals = {}


def fn_normals(case, prec):
    """[N_PATHS, n_sim] the case's normals in the precision's own type; row p is the buffer's elements p n_sim .."""
    from oracle import pyoracle
    key = (n_sim(case), prec)
    if key not in _normals:
        z = pyoracle.generate_normals(NORMALS_SEED, N_PATHS * n_sim(case), prec).reshape(N_PATHS, n_sim(case))
        assert z.dtype == NP_T[prec]
        z.setflags(write=False)
        _normals[key] = z
    return _normals[key]


def samples_of(case, z, use_window, dtype, mutate=0, count0=None):
    """window_restate.samples of the paths whose normals are z [n, steps], under the case's option (count0: the count
    the paths start from, by default the option's Ik)"""
    opt = fn_option(case, use_window)
    return wr.samples(z.astype(np.float64), opt.Sk if opt.Sk != 0 else opt.S0, opt.Ik if count0 is None else count0, wr.step_time(opt, case.n_steps, dtype),
                      opt.r, opt.v, opt.K, opt.B, opt.P1, opt.P2, use_window, False, None, dtype, wc.MARGIN, mutate)


_restated = {}


def fn_restated(case, prec, use_window, dtype):
    key = (case.name, prec, use_window, np.dtype(dtype))
    if key not in _restated:
        _restated[key] = samples_of(case, fn_normals(case, prec), use_window, dtype)
    return _restated[key]


def fn_log_spread(case, prec):
    a, b = (fn_restated(case, prec, 1, t).members[0].logs.astype(np.longdouble) for t in (wc.OWN[prec], wc.OTHER[prec]))
    return float(np.abs(a - b).max())


def _wanted(want, own, other, prec):
    spread = wc._diff(own.y, other.y, want.decided)
    y_hi = np.abs(want.cands).max(axis=1)
    tol = np.maximum(4.0 * spread, wc.FLOOR[prec] * np.maximum(y_hi, np.abs(want.y).mean()))
    return wc.PPWanted(want, tol, None, spread, 0.0)


def fn_wanted(case, prec, use_window):
    """window_cases.PPWanted of the case's N_PATHS payoffs, from the restatements alone"""
    return _wanted(*(fn_restated(case, prec, use_window, t) for t in (np.float64, wc.OWN[prec], wc.OTHER[prec])), prec)


def first(w, n):
    """the PPWanted of the first n paths of w's (the tolerance stays the case's)"""
    s = w.want
    return w._replace(want=s._replace(y=s.y[:n], cands=s.cands[:n], decided=s.decided[:n], ctrl=s.ctrl[:n]), tol_y=w.tol_y[:n])


# three ways the cache-line-tiled VEC loop could be wrong, restated on the row layout of the buffer
(ROW_ONE_VECTOR_LATE,       # a row read from one 16-byte vector after its start (the last one runs on into the first row)
 LAST_VECTOR_DROPPED,       # the last 16-byte vector of a row not consumed
 COUNT_TAKES_NEIGHBOUR,     # the count also takes the neighbouring row's vectors that share the row's first line: a
                            # comparison at the start price for each of their elements (a dead vector leaves the price
                            # where it is).  A 16-byte-aligned buffer of rows of whole lines shares none
 ) = ("late", "dropped", "neighbour")


def mistaken(case, prec, use_window, mistake, skew=0):
    """[N_PATHS] float64 payoffs of the case under the mistake (skew: the address of the normals mod 128, which decides
    what a row shares its first line with)"""
    V, z = VEC[prec], fn_normals(case, prec)
    n, steps = z.shape
    assert steps % V == 0
    if mistake == ROW_ONE_VECTOR_LATE:
        flat = z.ravel()
        return samples_of(case, np.concatenate([flat[V:], flat[:V]]).reshape(n, steps), use_window, np.float64).y
    if mistake == LAST_VECTOR_DROPPED:
        return samples_of(case, z[:, :steps - V], use_window, np.float64).y
    assert mistake == COUNT_TAKES_NEIGHBOUR and use_window
    opt = fn_option(case, 1)
    S_start = opt.Sk if opt.Sk != 0 else opt.S0
    shared = ((skew + np.arange(n) * steps * ITEM[prec]) % 128) // 16     # vectors of the row's first line before the row
    return samples_of(case, z, 1, np.float64, count0=opt.Ik + V * shared * int(opt.B > S_start)).y


# ---------------- bulk normals ----------------
BULK_SEED = 1234
BULK_SIZES = {capi.F32: (1, 3, 4, 5, 1023, 1024, 1025), capi.F64: (1, 2, 3, 511, 513)}
BULK_SKEWS = {capi.F32: (0, 16, 4, 12), capi.F64: (0, 16, 8)}

# ---------------- trajectory store ----------------
STORE_SEED, STORE_FIRST, STORE_BEYOND = 555, 3, 7     # paths 3 .. 3 + n_local - 1 of a job of n_local + 10
STORE_WINDOW = dict(B=104.0, P1=1, P2=4, use_window=1)
STORE_STEPS = (1, 3, 5, 9)
WIDE = (2 ** 29, 2 ** 29 + 1)      # n_local from 2^29 - 4 on takes 64-bit row offsets (store_kernel's `narrow`)
WIDE_WINDOW = dict(B=104.0, P1=1, P2=2, use_window=1)


def store_sizes(prec):
    V = VEC[prec]
    # in fp64 (V = 2) three of the eight coincide with their neighbours
    return tuple(dict.fromkeys((1, V - 1, V, V + 1, 2 * V - 1, 256 * V, 256 * V + 1, 256 * V + V - 1)))


def restated_size(prec):
    return 256 * VEC[prec] + 1


# name: the skews of d_traj, d_counts, d_payoffs in elements (None: the buffer is not passed)
STORE_PLACEMENTS = collections.OrderedDict([
    ("aligned", (0, 0, 0)), ("traj-off", (1, 0, 0)), ("counts-off", (0, 1, 0)), ("payoffs-off", (0, 0, 1)),
    ("all-off", (1, 1, 1)), ("no-counts", (0, None, 0)), ("no-payoffs", (0, 0, None))])


def store_option(window=None):
    return capi.make_option(**dict(wc.OPTION, **(STORE_WINDOW if window is None else window)))


def store_sim(prec, n_local, n_steps, first=STORE_FIRST, n_job=None, seed=STORE_SEED):
    return capi.make_sim(first + n_local + STORE_BEYOND if n_job is None else n_job, n_steps, prec, seed=seed,
                         path_offset=first, n_paths_local=n_local)


StoreWanted = collections.namedtuple("StoreWanted", "pp rows tol_rows spread_rows below clear")
StoreWanted.__doc__ = """pp: the PPWanted of the payoffs; rows [n_local, n_steps] float64 prices and their tolerance;
spread_rows: the largest price difference between the two restatements; below [n_local, n_steps] the comparisons
B > S_t and clear: where |ln(S_t / B)| >= MARGIN, so that the comparison has to come out as restated."""

_store = {}


def store_wanted(prec, n_steps=9):
    from oracle import pyoracle
    key = (prec, n_steps)
    if key not in _store:
        opt, sim = store_option(), store_sim(prec, restated_size(prec), n_steps)
        want, own, other = (wr.price_paths(pyoracle, opt, sim, t, wc.MARGIN) for t in (np.float64, wc.OWN[prec], wc.OTHER[prec]))
        rows_of = lambda s: (np.asarray(opt.S0, dtype=s.y.dtype) * np.exp(s.members[0].logs)).astype(np.longdouble)
        spread = float(np.abs(rows_of(own) - rows_of(other)).max())
        rows = rows_of(want).astype(np.float64)
        d = want.members[0].logs - np.log(opt.B / opt.S0)
        _store[key] = StoreWanted(_wanted(want, own, other, prec), rows, np.maximum(4.0 * spread, wc.FLOOR[prec] * rows),
                                  spread, want.members[0].below, np.abs(d) >= wc.MARGIN)
    return _store[key]


# ---------------- store pattern, reductions ----------------
def pattern_size(prec):
    return 256 * VEC[prec] + VEC[prec]


PATTERN_STEPS = 3
PATTERN_REFUSAL = "the store pattern is the vector store path's"
REDUCE_VARIANTS = (capi.REDUCE_SEQUENTIAL, capi.REDUCE_FIRST_ADD, capi.REDUCE_UNROLL_LAST, capi.REDUCE_GRID_STRIDE)


def reduce_sizes(prec):
    return (1, VEC[prec] - 1, VEC[prec] + 1, 511, 1025, 10_001)


def reduce_skews(prec):
    return (0, 16) + tuple(range(ITEM[prec], 16, ITEM[prec]))


def reduce_input(prec, n):
    """n values in [0.5, 1.5): every term has the sum's sign, so an fp64 sum in any order of at most a few hundred terms
    per thread and a tree above them is within 1e-13 of the exact one, and one element too few or too many moves it by
    at least 0.5 / (1.5 n) = 3e-5 of itself at the largest n"""
    rng = np.random.default_rng(1000 * prec + n)
    return (0.5 + rng.random(n)).astype(NP_T[prec])
