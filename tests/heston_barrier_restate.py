"""numpy restatement of the Heston single-barrier definitions of include/mcamd.h (mcamd_price_heston_barrier), used by
tests/test_gpu_heston_barrier.py and tested against the Heston and barrier restatements and the exact conditional
expectation in tests/test_heston_barrier_cpu.py.  Written from the header text: the step is heston_restate.samples',
operation for operation, the barrier body is barrier_restate.samples' with b = ln(B / S0) formed in float64 and narrowed
once and, in the bridge factor, the variance v+ the step was taken at; one numpy dtype throughout (float32, float64 or
longdouble), the sample formed in float64 (longdouble when the dtype is) from the path-precision w and h.  The factor
test is the header's division-free one in natural-log units; the fp32 kernel makes it in log2 units, which is inside the
spread the GPU tolerances are taken from."""
import numpy as np

import barrier_restate as br
import heston_restate as hr

Q_CUT = br.Q_CUT


def samples(z, zv, S0, K, B, T, r, heston_params, kind, payoff, monitoring, dtype=np.float64):
    """z, zv: [n_steps, n_paths] normals of the log-price and of the variance.  heston_params = (q, v0, kappa, theta,
    xi, rho).  Returns a dict: y (float64 samples, or longdouble when dtype is), S_T, v_n (the raw variance) and w (of
    the dtype, each path walked to maturity whatever hit it), alive (no step end hit), live (steps entered not yet
    hit), trunc (counted steps entered with v < 0), vs (sum of v+ over the counted steps, of the dtype), counted (the
    number of counted steps), max_vp (the largest v+ of any step, float64), min_abs_d (smallest |X_i - b| over all step
    ends, float64), min_abs_v (smallest |v| over the counted steps at their entry, float64)."""
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
    b = f(np.log(np.float64(B) / np.float64(S0)))
    kq = f(2) / dt
    q_cut = f(Q_CUT[dt_])
    up, out = br.is_up(kind), br.is_out(kind)
    X = np.zeros(n, dtype=dt_)
    v = np.full(n, f(v0), dtype=dt_)
    d_prev = np.full(n, abs(b), dtype=dt_)
    w = np.ones(n, dtype=dt_)
    vs = np.zeros(n, dtype=dt_)
    alive = np.ones(n, dtype=bool)
    live = np.zeros(n, dtype=np.int64)
    trunc = np.zeros(n, dtype=np.int64)
    counted_steps = np.zeros(n, dtype=np.int64)
    min_abs_d = np.full(n, np.inf)
    min_abs_v = np.full(n, np.inf)
    max_vp = np.zeros(n)
    for i in range(n_steps):
        counted = alive.copy() if out else np.ones(n, dtype=bool)
        live += alive
        counted_steps += counted
        trunc += counted & (v < f(0))
        min_abs_v = np.where(counted, np.minimum(min_abs_v, np.abs(v).astype(np.float64)), min_abs_v)
        vp = np.maximum(v, f(0))
        s = np.sqrt(vp)
        wz = rho * z[i] + rho_c * zv[i]
        X = X + ((mu - vp / f(2)) * dt + (s * sqrt_dt) * z[i])
        v = v + (kappa * (theta - vp) * dt + (xi * s * sqrt_dt) * wz)
        vs = vs + np.where(counted, vp, f(0))
        max_vp = np.maximum(max_vp, vp.astype(np.float64))
        hit = (X > b) if up else (b > X)
        d = (b - X) if up else (X - b)
        alive &= ~hit
        min_abs_d = np.minimum(min_abs_d, np.abs(d).astype(np.float64))
        if monitoring == br.CONTINUOUS:
            num = kq * d_prev * d                      # q v+
            take = alive & (num < q_cut * vp)          # f_i is exactly 1 elsewhere: v+ = 0 takes none
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                fac = f(1) - np.exp(-(num / vp))
            w = np.where(take, w * fac, w)
            d_prev = d
    w = np.where(alive, w, f(0))
    S_T = f(S0) * np.exp(X)
    h = np.maximum(f(K) - S_T, f(0)) if payoff == br.PUT else np.maximum(S_T - f(K), f(0))
    ww, hh = w.astype(wide), h.astype(wide)
    y = ww * hh if out else (wide(1) - ww) * hh
    return dict(y=y, S_T=S_T, v_n=v, w=w, h=h, alive=alive, live=live, trunc=trunc, vs=vs, counted=counted_steps, max_vp=max_vp,
                min_abs_d=min_abs_d, min_abs_v=min_abs_v)


def variance_clock(zv, T, heston_params, dtype=np.float64):
    """sum_i v+_i dt of every path at rho = 0, where the variance reads zv alone: the step's variance line and nothing
    else.  zv: [n_steps, n_paths]."""
    q, v0, kappa, theta, xi, rho = heston_params
    assert rho == 0.0
    f = np.dtype(dtype).type
    n_steps, n = zv.shape
    dt = f(T) / f(n_steps)
    sqrt_dt = np.sqrt(dt)
    v = np.full(n, f(v0))
    total = np.zeros(n, dtype=dtype)
    for i in range(n_steps):
        vp = np.maximum(v, f(0))
        v = v + (f(kappa) * (f(theta) - vp) * dt + (f(xi) * np.sqrt(vp) * sqrt_dt) * zv[i].astype(dtype))
        total = total + vp
    return total * dt


def philox_normals_f32(seed, first, n, n_steps, block0=0):
    """[n_steps, n] normals of global paths first..first+n-1 from Philox blocks block0, block0 + 1, .. by rocRAND's
    single-precision Box-Muller, four per block, evaluated in float64: the fp32 kernels' normals up to fp32 rounding,
    for statistical tests only"""
    blocks = -(-n_steps // 4)
    sub = np.uint64(first) + np.arange(n, dtype=np.uint64)
    out = np.empty((4 * blocks, n))
    for k in range(blocks):
        words = hr.philox4x32_10(seed, sub, np.uint64(block0 + k))
        for pair in range(2):
            x, y = words[2 * pair].astype(np.float64), words[2 * pair + 1].astype(np.float64)
            u = np.float32((x + 1.0) * 2.0 ** -32).astype(np.float64)   # never 0: (2^32 - 1 + 1) 2^-32 rounds to 1
            a = (y + 1.0) * (2.0 * np.pi * 2.0 ** -32)
            s = np.sqrt(-2.0 * np.log(u))
            out[4 * k + 2 * pair] = np.sin(a) * s
            out[4 * k + 2 * pair + 1] = np.cos(a) * s
    return out[:n_steps]
