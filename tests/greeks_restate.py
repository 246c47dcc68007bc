"""numpy restatement of the Greeks samples of include/mcamd.h (mcamd_price_greeks), used by tests/test_gpu_greeks.py
and tests/greeks_cases.py and checked against itself in tests/test_greeks_cpu.py.  No kernel runs here.

  * normals(): the engine's stream for a path: subsequence = global path id, Philox blocks 0, 1, .., from the oracle's
    rocRAND-exact generator;
  * restate(): the six undiscounted samples per path — price, delta, gamma, vega, rho, theta — of the pathwise or the
    likelihood-ratio estimator, in one numpy dtype throughout (float32, float64 or longdouble): the step sums, the
    exponential, the payoff, the barrier count and the samples.  (The kernels form the samples in fp64 from the
    path-precision state; a float32 restatement rounds them to float32 as well, so it differs from the float64 one by
    no less than an fp32 kernel may.)

Notation (include/mcamd.h): S_s the start price of the simulated segment, n_sim = n_steps - Tk its steps, T_h = n_sim dt,
L = ln(S_T / S_s), z_i the normals, y the payoff."""
import collections

import numpy as np

F32, F64 = 32, 64
PATHWISE, LIKELIHOOD_RATIO = 1, 2
PER_BLOCK = {F32: 4, F64: 2}   # normals of one Philox block

Restated = collections.namedtuple("Restated", "q S_T count logs")
Restated.__doc__ = """q: [n, 6] samples; S_T: [n] terminal prices; count: [n] steps below the barrier plus Ik (None
without a window); logs: [n, n_sim] ln(S_t / S_s) after each step.  All of restate()'s dtype but the integer count."""


def normals(oracle, prec, seed, path_ids, n_sim):
    """[len(path_ids), n_sim] normals of the engine's stream: subsequence = global path id, blocks from 0"""
    nb = PER_BLOCK[prec]
    blocks = (n_sim + nb - 1) // nb
    gen = oracle.normal2_f64 if prec == F64 else oracle.normal4_f32
    z = np.empty((len(path_ids), blocks * nb))
    for i, p in enumerate(path_ids):
        for b in range(blocks):
            z[i, b * nb:(b + 1) * nb] = gen(seed, int(p), b)
    return z[:, :n_sim]


def restate(oracle, opt, sim, method, dtype=np.float64):
    """Restated(q, S_T, count, logs) of the sim's shard (paths path_offset.. of seed), formed in dtype from the
    normals of sim.precision"""
    f = np.dtype(dtype).type
    n_sim = sim.n_steps - opt.Tk
    dt = f(opt.dt) if opt.dt > 0 else f(opt.T) / f(sim.n_steps)
    S_s = f(opt.Sk if opt.Sk != 0 else opt.S0)
    r, v, T, K = f(opt.r), f(opt.v), f(opt.T), f(opt.K)
    half, zero = f(0.5), f(0)
    Th = f(n_sim) * dt
    sq = np.sqrt(dt)
    z = normals(oracle, sim.precision, sim.seed, range(sim.path_offset, sim.path_offset + sim.n_paths_local), n_sim)
    z = z.astype(dtype)
    logs = np.cumsum((r - half * v * v) * dt + v * sq * z, axis=1, dtype=dtype)
    L = logs[:, -1]
    St = S_s * np.exp(L)
    y = np.maximum(St - K, zero)
    count = None
    if opt.use_window:
        logB = np.log(f(opt.B) / S_s) if opt.B > 0 else f(-np.inf)
        count = opt.Ik + (logB > logs).sum(axis=1)
        y = np.where((count >= opt.P1) & (count <= opt.P2), y, zero)
    q = np.zeros((len(y), 6), dtype=dtype)
    q[:, 0] = y
    if method == PATHWISE:
        itm = St > K
        mu = r - v * v / f(2)
        q[:, 1] = np.where(itm, St / S_s, zero)
        q[:, 2] = np.where(itm, K * (L - mu * Th) / (S_s * S_s * v * v * Th), zero)
        q[:, 3] = np.where(itm, St * (L - (r + v * v / f(2)) * Th) / v, zero)
        q[:, 4] = -T * y + np.where(itm, St * Th, zero)
        if opt.Tk == 0 and opt.dt == 0:
            q[:, 5] = r * y - np.where(itm, St * (mu + (L - mu * T) / (f(2) * T)), zero)
    else:
        z1, sz, szz = z[:, 0], z.sum(axis=1, dtype=dtype), (z * z).sum(axis=1, dtype=dtype)
        q[:, 1] = y * z1 / (S_s * v * sq)
        q[:, 2] = y * ((z1 * z1 - f(1)) / (S_s * S_s * v * v * dt) - z1 / (S_s * S_s * v * sq))
        q[:, 3] = y * ((szz - f(n_sim)) / v - sq * sz)
        q[:, 4] = y * (sz * sq / v - T)
    return Restated(q, St, count, logs)
