"""numpy restatement of the smile definitions of include/mcamd.h (mcamd_price_localvol_smile), used by
tests/test_gpu_localvol_smile.py and tested in tests/test_localvol_smile_cpu.py.  Written from the header text: the
paths are those of mcamd_price_localvol without a barrier (the tables, the lookup and the slice rule come from the
untouched tests/localvol_restate.py), walked in one numpy dtype — float32, float64 or longdouble — and read at the
expiry steps; a node's sample is formed in that dtype from the strike narrowed to it and summed in float64.

The `mutate` argument of spots() and node_sums() restates four mistakes a kernel of this shape could make; no mutated
kernel exists or is run.  tests/test_gpu_localvol_smile.py shows, on the CPU, that each moves the restated result of one
of its cases by more than that case's tolerance."""
import numpy as np

from localvol_restate import lookup, row_of, tables

CALL, PUT = 0, 1
LATE_EXPIRY, ALL_LANES, FIRST_TRIP_ADDS = "expiry one step late", "strike loop over all 64 lanes", "first trip adds"


def spots(z, S0, T, r, q, grid, sigma, n_steps, expiry_steps, dtype=np.float64, mutate=None):
    """z: [>= last expiry step, n_paths] normals; n_steps: the job's step count (dt = T / n_steps and the slice rule
    run against it, whatever the last expiry is).  Returns S[m, path] at the expiry steps, in dtype."""
    dt_ = np.dtype(dtype)
    f = dt_.type
    n_t, n_x = grid[0], grid[1]
    steps = [int(s) for s in expiry_steps]
    assert all(a < b for a, b in zip([0] + steps[:-1], steps)) and steps[-1] <= n_steps
    if mutate == LATE_EXPIRY:
        steps = [min(s + 1, n_steps) for s in steps]
    z = z.astype(dt_)
    tabs = tables(grid, sigma, dt_)
    dt = f(T) / f(n_steps)
    sqrt_dt = np.sqrt(dt)
    mu = f(r) - f(q)
    X = np.zeros(z.shape[1], dtype=dt_)
    out = np.empty((len(steps), z.shape[1]), dtype=dt_)
    m = 0
    for i in range(steps[-1]):
        s = lookup(tabs, n_x, row_of(i, n_t, n_steps), X)
        X = X + ((mu - s * s / f(2)) * dt + (s * sqrt_dt) * z[i])
        while m < len(steps) and steps[m] == i + 1:
            out[m] = f(S0) * np.exp(X)
            m += 1
    return out


def samples(S, strikes, payoff):
    """h[m, k, path] in S's dtype: max(+-(S_m - K_k), 0) with K_k narrowed to that dtype"""
    K = np.asarray(strikes, dtype=np.float64).astype(S.dtype)[None, :, None]
    h = K - S[:, None, :] if payoff == PUT else S[:, None, :] - K
    return np.maximum(h, S.dtype.type(0))


def _row_sums(S_row, K, put, chunk):
    """one expiry: (sum, sumsq, paying) over the paths for every strike, chunk paths at a time, in a fixed order"""
    total, totsq, paying = np.zeros(K.size), np.zeros(K.size), np.zeros(K.size, dtype=np.int64)
    for lo in range(0, S_row.size, chunk):
        s = S_row[None, lo:lo + chunk]
        h = np.maximum(K - s if put else s - K, S_row.dtype.type(0)).astype(np.float64, copy=False)
        total += h.sum(axis=1)
        totsq += np.einsum("kp,kp->k", h, h)
        paying += np.count_nonzero(h, axis=1)
    return total, totsq, paying


def node_sums(S, strikes, payoff, mutate=None, stale=None, threads=1):
    """(sum, sumsq, paying): [n_e, n_K] float64 sums of h and h^2 over the paths and the number of paths with h > 0.
    Every expiry is summed on its own, 2^18 samples at a time in path order, so `threads` (expiries summed side by
    side, for a large job) changes no bit.
    mutate = ALL_LANES: every wavefront's strike loop runs over 64 lanes, the lanes past the last path holding the spot
    of the path 64 before (what a lane that walks nothing would still hold); FIRST_TRIP_ADDS: the sums start from `stale`,
    what the records held before (one number per node)."""
    if mutate == ALL_LANES:
        n = S.shape[1]
        pad = (-n) % 64
        filler = S[:, -64:][:, :pad] if n >= 64 else np.repeat(S[:, -1:], pad, axis=1)
        S = np.concatenate([S, filler], axis=1)
    K = np.asarray(strikes, dtype=np.float64).astype(S.dtype)[:, None]
    chunk = max(64, (1 << 18) // K.size)
    work = lambda row: _row_sums(row, K, payoff == PUT, chunk)
    if threads > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(threads) as pool:
            rows = list(pool.map(work, S))
    else:
        rows = [work(row) for row in S]
    total, totsq, paying = (np.array([r[i] for r in rows]) for i in range(3))
    if mutate == FIRST_TRIP_ADDS:
        total, totsq = total + stale, totsq + stale
    return total, totsq, paying


def finalize(stats, n, r, T, n_steps, expiry_steps, n_strikes):
    """(price, std_err) as [n_e, n_K]: each node discounted to its own expiry t_m = s_m T / n_steps, the sample variance
    of mcamd_finalize (n - 1 in the denominator, floored at 0)"""
    n_e = len(expiry_steps)
    stats = np.asarray(stats, dtype=np.float64)
    total, totsq = stats[:n_e * n_strikes].reshape(n_e, n_strikes), stats[n_e * n_strikes:].reshape(n_e, n_strikes)
    t = np.asarray(expiry_steps, dtype=np.float64) * (T / n_steps)
    disc = np.exp(-r * t)[:, None]
    mean = total / n
    var = np.maximum((totsq - n * mean * mean) / (n - 1), 0.0) if n > 1 else np.zeros_like(mean)
    return disc * mean, disc * np.sqrt(var / n)
