"""numpy restatement of the window samples of mcamd_price_paths (plain, antithetic, control variate) and of the points
of the nested-MC inner stage (include/mcamd.h; csrc/mc_device.hpp simulate_sample, csrc/price_impl.hpp, csrc/nmc.hip),
used by tests/window_cases.py and tests/test_gpu_window.py and checked in tests/test_window_cpu.py.  No kernel runs here.

  * normals(): full Philox blocks 0, 1, .. of consecutive subsequences from the oracle's rocRAND-exact generator;
  * walk(): one member (a path or its antithetic twin) in one numpy dtype throughout — float32, float64 or longdouble:
    the step exponents summed to ln(S_t / S_start), the barrier comparisons, the payoff;
  * samples(): the sample of a path (the pair's mean with `antithetic`), its control and its candidates;
  * price_paths(): the job semantics of mcamd_price_paths; nmc_points(): those of mcamd_nmc_inner / mcamd_nmc_fused.

A barrier comparison B > S_t, restated as ln(B / S_start) > ln(S_t / S_start), is not a continuous function of the
arithmetic: within rounding of the barrier an fp32 kernel may decide it the other way.  So beside its own count a member
carries the interval [cnt_lo, cnt_hi] of the counts that are possible when every step with |ln(S_t / B)| < margin may
go either way, and is *decided* when P1 <= count <= P2 has one outcome over the whole interval.  An undecided member
has two candidate payoffs, 0 and max(S_T - K, 0); a sample's candidates are the means over its members' candidates.

Mistakes (the `mutate` argument): each restates one way a kernel could be wrong; tests/test_window_cpu.py shows that
every one of them lies beyond the tolerance the GPU tests allow."""
import collections

import numpy as np

F32, F64 = 32, 64
PER_BLOCK = {F32: 4, F64: 2}   # normals of one Philox block
ANTITHETIC, CONTROL_VARIATE = 2, 4   # MCAMD_FLAG_ANTITHETIC, MCAMD_FLAG_CONTROL_VARIATE

(LAST_BLOCK_SHORT,     # the partial last Philox block takes one step too few
 LAST_BLOCK_LONG,      # ... one too many
 P1_STRICT,            # count > P1 for >=
 P2_STRICT,            # count < P2 for <=
 TWIN_DRIFT,           # the twin's step exponent drift - x for 2 drift - x
 TWIN_SHARES_COUNT,    # the twin paid on the path's count
 COUNT_FROM_ZERO,      # an inner path started from count 0, not from the stored count
 DISCOUNT_TIME_TO_GO,  # a point discounted over its remaining time, not over T
 SUBSEQUENCE_STRIDED,  # inner path j of point q draws subsequence q + j n_points for q n_inner + j
 CLOSED_POINT_PRICED,  # a point whose stored count is beyond P2 priced as if the count stood at P2
 CONTROL_MEAN_AT_T,    # the control centred on S_start exp(r T) for S_start exp(r n_sim dt)
 ) = range(1, 12)

Walk = collections.namedtuple("Walk", "logs S_T below min_abs_d cnt cnt_lo cnt_hi decided y full")
Walk.__doc__ = """one member: logs [n, n_sim] ln(S_t / S_start); S_T [n]; below [n, n_sim] the comparisons B > S_t;
min_abs_d [n] min_t |ln(S_t / B)| (inf without a window or a step); cnt its own count, [cnt_lo, cnt_hi] the possible
ones; decided [n]; y [n] its payoff; full [n] max(S_T - K, 0)."""

Samples = collections.namedtuple("Samples", "y c cands decided ctrl members")
Samples.__doc__ = """y [n] samples; c [n] centred control (None without control_mean); cands [n, k] candidate samples
(all equal to y where decided; k = 2, or 4 for a pair); decided [n]; ctrl [n] S_T (the pair's mean); members: the one
or two Walks."""

Points = collections.namedtuple("Points", "price lo hi undecided closed to_go y y_hi decided")
Points.__doc__ = """nested-MC points of a shard, [n_local, n_steps]: price (the restatement's own), [lo, hi] the
interval of the discounted mean over the undecided inner paths' candidates, undecided: their number, closed: stored
count > P2, to_go: steps to go.  Per inner path, [n_local, n_steps, n_inner]: y its payoff (dtype), y_hi its largest
candidate (float64), decided.  The inner paths of a closed point are not run: 0 and decided."""


def normals(oracle, prec, seed, first, n, n_sim):
    """[n, blocks * per_block] float64: the WHOLE blocks 0 .. ceil(n_sim / per_block) - 1 of subsequences first ..
    first + n - 1 (a caller takes the first n_sim columns; LAST_BLOCK_LONG reads one more)"""
    nb = PER_BLOCK[prec]
    blocks = (n_sim + nb - 1) // nb
    if blocks == 0 or n == 0:
        return np.zeros((n, 0))
    return oracle.normals_of_subsequences(seed, int(first), int(n), blocks, prec).astype(np.float64)


def normals_of(oracle, prec, seed, subsequences, n_sim):
    """normals() for arbitrary subsequences, one per-block call each"""
    nb = PER_BLOCK[prec]
    blocks = (n_sim + nb - 1) // nb
    gen = oracle.normal2_f64 if prec == F64 else oracle.normal4_f32
    z = np.zeros((len(subsequences), blocks * nb))
    for i, s in enumerate(subsequences):
        for b in range(blocks):
            z[i, b * nb:(b + 1) * nb] = gen(seed, int(s), b)
    return z


def steps_taken(n_sim, prec, mutate):
    """the steps a path of n_sim steps takes: n_sim, unless the mistake is in the partial last block and there is one"""
    rem = n_sim % PER_BLOCK[prec]
    if rem and mutate == LAST_BLOCK_SHORT:
        return n_sim - 1
    if rem and mutate == LAST_BLOCK_LONG:
        return n_sim + 1
    return n_sim


def inside(count, P1, P2, mutate=0):
    lo = count > P1 if mutate == P1_STRICT else count >= P1
    hi = count < P2 if mutate == P2_STRICT else count <= P2
    return lo & hi


def walk(x, S_start, count0, K, B, P1, P2, use_window, dtype, margin, mutate=0):
    """Walk of the members whose step exponents are x [n, steps] (dtype), from S_start and count0 (scalars or [n])"""
    f = np.dtype(dtype).type
    n, steps = x.shape
    S_start = np.broadcast_to(np.asarray(S_start, dtype=dtype), (n,))
    count0 = np.broadcast_to(np.asarray(count0, dtype=np.int64), (n,))
    logs = np.cumsum(x, axis=1, dtype=dtype)
    L = logs[:, -1] if steps else np.zeros(n, dtype=dtype)
    S_T = S_start * np.exp(L)
    full = np.maximum(S_T - f(K), f(0))
    if not use_window:
        none = np.zeros((n, steps), dtype=bool)
        return Walk(logs, S_T, none, np.full(n, np.inf), count0, count0, count0, np.ones(n, dtype=bool), full, full)
    logB = np.log(f(B) / S_start) if B > 0 else np.full(n, -np.inf, dtype=dtype)
    d = logs - logB[:, None]                       # ln(S_t / B)
    below = d < 0                                  # ln(B / S_start) > ln(S_t / S_start)
    near = np.abs(d) < margin
    cnt = count0 + below.sum(axis=1)
    cnt_lo = count0 + (below & ~near).sum(axis=1)
    cnt_hi = cnt_lo + near.sum(axis=1)
    # the window test is monotone at each end, so it is the same over [cnt_lo, cnt_hi] iff the interval lies inside
    # the window or beside it
    decided = ((cnt_lo >= P1) & (cnt_hi <= P2)) | (cnt_hi < P1) | (cnt_lo > P2)
    y = np.where(inside(cnt, P1, P2, mutate), full, f(0))
    min_abs_d = np.abs(d).min(axis=1).astype(np.float64) if steps else np.full(n, np.inf)
    return Walk(logs, S_T, below, min_abs_d, cnt, cnt_lo, cnt_hi, decided, y, full)


def samples(z, S_start, count0, dt, r, v, K, B, P1, P2, use_window, antithetic, control_mean, dtype, margin, mutate=0):
    """Samples of the paths whose normals are z [n, steps]: every column of z is stepped"""
    f = np.dtype(dtype).type
    dt, r, v = f(dt), f(r), f(v)
    half, zero = f(0.5), f(0)
    drift = (r - half * v * v) * dt
    x = drift + v * np.sqrt(dt) * z.astype(dtype)
    a = walk(x, S_start, count0, K, B, P1, P2, use_window, dtype, margin, mutate)
    cand = lambda m: np.stack([np.where(m.decided, m.y, zero), np.where(m.decided, m.y, m.full)], axis=1)
    y, ctrl, cands, decided, members = a.y, a.S_T, cand(a), a.decided, (a,)
    if antithetic:
        x2 = (drift - x) if mutate == TWIN_DRIFT else (drift + drift) - x
        b = walk(x2, S_start, count0, K, B, P1, P2, use_window, dtype, margin, mutate)
        if mutate == TWIN_SHARES_COUNT and use_window:
            b = b._replace(y=np.where(inside(a.cnt, P1, P2), b.full, zero))
        y, ctrl, decided, members = half * (a.y + b.y), half * (a.S_T + b.S_T), a.decided & b.decided, (a, b)
        ca, cb = cand(a), cand(b)
        cands = np.stack([half * (ca[:, i] + cb[:, j]) for i in (0, 1) for j in (0, 1)], axis=1)
    c = None if control_mean is None else ctrl - f(control_mean)
    return Samples(y, c, cands, decided, ctrl, members)


def step_time(opt, n_steps, dtype=np.float64):
    f = np.dtype(dtype).type
    return f(opt.dt) if opt.dt > 0 else f(opt.T) / f(n_steps)


def control_mean_of(opt, sim, mutate=0):
    """E[S_T] of the simulated segment, as csrc/price_impl.hpp documents control_mean: S_start exp(r n_sim dt)"""
    S_start = opt.Sk if opt.Sk != 0 else opt.S0
    span = opt.T if mutate == CONTROL_MEAN_AT_T else (sim.n_steps - opt.Tk) * float(step_time(opt, sim.n_steps))
    return S_start * np.exp(opt.r * span)


def price_paths(oracle, opt, sim, dtype=np.float64, margin=0.0, mutate=0):
    """Samples of the sim's shard of mcamd_price_paths: subsequence = global path id; the restart triple (Ik, Sk, Tk)
    leaves n_sim = n_steps - Tk steps from Sk (0: S0) and the count Ik; opt.dt overrides T / n_steps; no discount."""
    n_sim = sim.n_steps - opt.Tk
    z = normals(oracle, sim.precision, sim.seed, sim.path_offset, sim.n_paths_local, n_sim)
    z = z[:, :steps_taken(n_sim, sim.precision, mutate)]
    cm = control_mean_of(opt, sim, mutate) if sim.flags & CONTROL_VARIATE else None
    return samples(z, opt.Sk if opt.Sk != 0 else opt.S0, opt.Ik, step_time(opt, sim.n_steps, dtype), opt.r, opt.v, opt.K,
                   opt.B, opt.P1, opt.P2, opt.use_window, bool(sim.flags & ANTITHETIC), cm, dtype, margin, mutate)


def nmc_points(oracle, opt, sim, St, counts, dtype=np.float64, margin=0.0, mutate=0, paths=None):
    """Points of the sim's shard of the nested-MC inner stage from the stored rows St, counts [n_local, n_steps]:
    point id = global path * n_steps + step; inner path j draws subsequence point id * n_inner + j from block 0 and
    takes n_steps - 1 - step steps from the stored (St, count); a point whose stored count exceeds P2 is 0; price =
    exp(-r T) (the full T) * mean over n_inner.  paths: the local paths to price (default: all)."""
    f = np.dtype(dtype).type
    n_steps, n_inner, prec = sim.n_steps, sim.n_paths_inner, sim.precision
    paths = np.arange(sim.n_paths_local) if paths is None else np.asarray(paths)
    m = len(paths)
    St = np.asarray(St)[paths].astype(dtype)
    counts = np.asarray(counts)[paths].astype(np.int64) if opt.use_window else np.zeros((m, n_steps), dtype=np.int64)
    dt = step_time(opt, n_steps, dtype)
    shape = (m, n_steps)
    price, lo, hi = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    undecided = np.zeros(shape, dtype=np.int64)
    closed = (counts > opt.P2) if opt.use_window else np.zeros(shape, dtype=bool)
    to_go = np.broadcast_to(n_steps - 1 - np.arange(n_steps), shape)
    y = np.zeros(shape + (n_inner,), dtype=dtype)
    y_hi = np.zeros(shape + (n_inner,))
    decided = np.ones(shape + (n_inner,), dtype=bool)
    point_id = (sim.path_offset + paths)[:, None].astype(object) * n_steps + np.arange(n_steps)[None, :]
    n_points = sim.n_paths * n_steps
    for step in range(n_steps):
        remaining = n_steps - 1 - step
        taken = steps_taken(remaining, prec, mutate)
        zs = []
        for p in range(m):
            q = int(point_id[p, step])
            if mutate == SUBSEQUENCE_STRIDED:
                zs.append(normals_of(oracle, prec, sim.seed, [q + j * n_points for j in range(n_inner)], remaining))
            else:
                zs.append(normals(oracle, prec, sim.seed, q * n_inner, n_inner, remaining))
        z = np.concatenate(zs, axis=0)[:, :taken] if m else np.zeros((0, taken))
        c0 = np.repeat(counts[:, step], n_inner)
        if mutate == COUNT_FROM_ZERO:
            c0 = np.zeros_like(c0)
        if mutate == CLOSED_POINT_PRICED:
            c0 = np.minimum(c0, opt.P2)
        s = samples(z, np.repeat(St[:, step], n_inner), c0, dt, opt.r, opt.v, opt.K, opt.B, opt.P1, opt.P2,
                    opt.use_window, False, None, dtype, margin, mutate)
        span = float(remaining * float(dt)) if mutate == DISCOUNT_TIME_TO_GO else opt.T
        scale = np.exp(-opt.r * span) / n_inner
        live = ~closed[:, step] | (mutate == CLOSED_POINT_PRICED)
        per = lambda a: np.where(live, a.astype(np.float64).reshape(m, n_inner).sum(axis=1) * scale, 0.0)
        price[:, step] = per(s.y)
        lo[:, step], hi[:, step] = per(s.cands.min(axis=1)), per(s.cands.max(axis=1))
        undecided[:, step] = np.where(live, (~s.decided).reshape(m, n_inner).sum(axis=1), 0)
        y[:, step] = np.where(live[:, None], s.y.reshape(m, n_inner), f(0))
        y_hi[:, step] = np.where(live[:, None], s.cands.max(axis=1).astype(np.float64).reshape(m, n_inner), 0.0)
        decided[:, step] = s.decided.reshape(m, n_inner) | ~live[:, None]
    return Points(price, lo, hi, undecided, closed, to_go, y, y_hi, decided)
