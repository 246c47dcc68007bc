"""numpy restatement of the Heston definitions of include/mcamd.h (mcamd_price_heston), used by
tests/test_gpu_heston.py and tested against the barrier and local-volatility restatements, the deterministic-variance
limit and the closed form in tests/test_heston_cpu.py.  Written from the header text: one numpy dtype throughout —
float32, float64 or longdouble — for the step; sqrt(1 - rho^2) is formed in float64 and narrowed once, as the host forms
it; the sample is widened to float64 (longdouble when the dtype is), and the factor 1 / n of the average variance is
applied there.  The fused operations of the header are written as plain products and sums, grouped as the header
groups them: what contraction changes is inside the spread the GPU tolerances are taken from.

The inputs F, N and H and the market of every Heston test live here, and so do the draws: draws() fetches the two
normal streams of a few hundred paths from the oracle block by block; philox_normals_f64() is a vectorised numpy
statement of the same Philox4x32-10 and Box-Muller for the statistical tests, which need millions of paths
(tests/test_heston_cpu.py checks it against the oracle)."""
import numpy as np

CALL, PUT = 0, 1
VARIANCE_BLOCKS = 2 ** 63   # the variance normals' first Philox block

S0, T_, R, Q_DIV = 100.0, 1.0, 0.03, 0.01
STRIKES = ((80.0, PUT), (100.0, CALL), (120.0, CALL))
# (v0, kappa, theta, xi, rho)
MODELS = {
    "F": (0.04, 2.0, 0.04, 0.3, -0.7),   # Feller holds: 2 kappa theta = 0.16 >= xi^2 = 0.09
    "N": (0.04, 1.5, 0.04, 0.6, -0.7),   # Feller fails: 0.12 < 0.36
    "H": (0.01, 0.5, 0.01, 1.0, -0.9),   # mostly truncated
}


def params(name, q=Q_DIV, **changes):
    """(q, v0, kappa, theta, xi, rho) of a named input, with some of them changed"""
    p = dict(zip(("v0", "kappa", "theta", "xi", "rho"), MODELS[name]), q=q)
    p.update(changes)
    return (p["q"], p["v0"], p["kappa"], p["theta"], p["xi"], p["rho"])


def samples(z, zv, S0, K, T, r, heston_params, payoff, dtype=np.float64):
    """z, zv: [n_steps, n_paths] normals of the log-price and of the variance.  heston_params = (q, v0, kappa, theta,
    xi, rho).  Returns a dict: y (float64 samples, or longdouble when dtype is), S_T and v_n (of the dtype; v_n is the
    raw variance), trunc (steps each path entered with v < 0), rv (the path's average variance, same type as y),
    min_abs_v (smallest |v_i| over the steps entered, float64)."""
    q, v0, kappa, theta, xi, rho = heston_params
    dt_ = np.dtype(dtype)
    n_steps, n = z.shape
    assert zv.shape == z.shape
    f = dt_.type
    wide = np.longdouble if dt_ == np.dtype(np.longdouble) else np.float64
    z, zv = z.astype(dt_), zv.astype(dt_)
    dt = f(T) / f(n_steps)
    sqrt_dt = np.sqrt(dt)
    mu = f(r) - f(q)
    rho_c = f(np.sqrt(np.float64(1.0) - np.float64(rho) * np.float64(rho)))
    rho, kappa, theta, xi = f(rho), f(kappa), f(theta), f(xi)
    X = np.zeros(n, dtype=dt_)
    v = np.full(n, f(v0), dtype=dt_)
    v_sum = np.zeros(n, dtype=dt_)
    trunc = np.zeros(n, dtype=np.int64)
    min_abs_v = np.full(n, np.inf)
    for i in range(n_steps):
        trunc += v < f(0)
        min_abs_v = np.minimum(min_abs_v, np.abs(v).astype(np.float64))
        vp = np.maximum(v, f(0))
        s = np.sqrt(vp)
        w = rho * z[i] + rho_c * zv[i]
        X = X + ((mu - vp / f(2)) * dt + (s * sqrt_dt) * z[i])
        v = v + (kappa * (theta - vp) * dt + (xi * s * sqrt_dt) * w)
        v_sum = v_sum + vp
    S_T = f(S0) * np.exp(X)
    h = np.maximum(f(K) - S_T, f(0)) if payoff == PUT else np.maximum(S_T - f(K), f(0))
    return dict(y=h.astype(wide), S_T=S_T, v_n=v, trunc=trunc, rv=v_sum.astype(wide) * (wide(1) / wide(n_steps)),
                min_abs_v=min_abs_v)


_draws = {}


def draws(prec, seed, first, n, n_steps):
    """([n_steps, n] log-price normals, [n_steps, n] variance normals) of global paths first..first+n-1, as the kernels
    draw them (as float64 values): from Philox blocks 0, 1, .. and 2^63, 2^63 + 1, .. of each path's subsequence.
    prec: 64 or 32."""
    from oracle import pyoracle as o
    key = (prec, seed, first, n, n_steps)
    if key not in _draws:
        per, draw = (2, o.normal2_f64) if prec == 64 else (4, o.normal4_f32)
        blocks = -(-n_steps // per)
        z = np.empty((blocks * per, n))
        zv = np.empty((blocks * per, n))
        for p in range(n):
            for k in range(blocks):
                z[k * per:(k + 1) * per, p] = draw(seed, first + p, k)
                zv[k * per:(k + 1) * per, p] = draw(seed, first + p, VARIANCE_BLOCKS + k)
        _draws[key] = (z[:n_steps], zv[:n_steps])
    return _draws[key]


def philox4x32_10(seed, subsequence, block):
    """the four words of Philox4x32-10 for arrays (or scalars) of 64-bit subsequences and blocks, rocRAND's counter
    layout: (block_lo, block_hi, subsequence_lo, subsequence_hi), key = (seed_lo, seed_hi)"""
    u64, low = np.uint64, np.uint64(0xFFFFFFFF)
    subsequence, block = np.broadcast_arrays(np.asarray(subsequence, dtype=u64), np.asarray(block, dtype=u64))
    c0, c1 = block & low, block >> u64(32)
    c2, c3 = subsequence & low, subsequence >> u64(32)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = u64(0xD2511F53) * c0, u64(0xCD9E8D57) * c2   # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> u64(32)) ^ c1 ^ u64(k0), p1 & low, (p0 >> u64(32)) ^ c3 ^ u64(k1), p0 & low
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox_normals_f64(seed, first, n, n_steps, block0=0):
    """[n_steps, n] fp64 normals of global paths first..first+n-1 from Philox blocks block0, block0 + 1, ..: rocRAND's
    double Box-Muller, two normals per block"""
    blocks = -(-n_steps // 2)
    sub = np.uint64(first) + np.arange(n, dtype=np.uint64)
    out = np.empty((2 * blocks, n))
    for k in range(blocks):
        x, y, zz, ww = philox4x32_10(seed, sub, np.uint64(block0 + k))
        v1, v2 = x ^ (y << np.uint64(21)), zz ^ (ww << np.uint64(21))
        u = (v1.astype(np.float64) + 1.0) * 2.0 ** -53      # exact: at most 53 bits
        w = (v2.astype(np.float64) + 1.0) * 2.0 ** -52
        s = np.sqrt(-2.0 * np.log(u))
        out[2 * k] = np.sin(w * np.pi) * s
        out[2 * k + 1] = np.cos(w * np.pi) * s
    return out[:n_steps]


def prices_f64(seed, n_paths, n_steps, strikes, heston_params, chunk=250_000, S0=S0, T=T_, r=R):
    """[(discounted mean, its standard error)] per (K, payoff) of strikes, then the mean trunc per path and the mean rv,
    of the float64 restatement over the paths 0..n_paths-1 under seed, on the Philox draws, a chunk of paths at a time;
    every strike is priced on the same paths"""
    total, total_sq = np.zeros(len(strikes)), np.zeros(len(strikes))
    total_trunc = total_rv = 0.0
    for lo in range(0, n_paths, chunk):
        m = min(chunk, n_paths - lo)
        z = philox_normals_f64(seed, lo, m, n_steps)
        zv = philox_normals_f64(seed, lo, m, n_steps, VARIANCE_BLOCKS)
        got = samples(z, zv, S0, strikes[0][0], T, r, heston_params, strikes[0][1])
        for j, (K, payoff) in enumerate(strikes):
            y = np.maximum(K - got["S_T"], 0.0) if payoff == PUT else np.maximum(got["S_T"] - K, 0.0)
            total[j] += y.sum()
            total_sq[j] += (y * y).sum()
        total_trunc += float(got["trunc"].sum())
        total_rv += float(got["rv"].sum())
    disc = np.exp(-r * T)
    mean = total / n_paths
    var = np.maximum(total_sq / n_paths - mean * mean, 0.0) * n_paths / (n_paths - 1)
    return list(zip(disc * mean, disc * np.sqrt(var / n_paths))), total_trunc / n_paths, total_rv / n_paths
