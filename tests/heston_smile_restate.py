"""numpy restatement of the Heston smile definitions of include/mcamd.h (mcamd_price_heston_smile), used by
tests/test_gpu_heston_smile.py and tested in tests/test_heston_smile_cpu.py.  Written from the header text: the paths
are those of mcamd_price_heston — the step loop of tests/heston_restate.py's samples(), operation for operation, in one
numpy dtype (float32, float64 or longdouble), with dt = T / n_steps over the WHOLE n_steps whatever the last expiry is —
read at the expiry steps: the spot S_m = S0 e^{X_{s_m}} and the raw variance v_{s_m}.  The draws come from
heston_restate.draws; the node sums from localvol_smile_restate.node_sums, since the strike phase is the same.

The `mutate` argument of states() restates three mistakes a kernel of this shape could make; no mutated kernel exists or
is run.  tests/test_gpu_heston_smile.py shows, on the CPU, that each moves the restated result of one of its cases by
more than that case's tolerance."""
import numpy as np

CALL, PUT = 0, 1
LATE_EXPIRY = "expiry one step late"
SAME_BLOCKS = "variance normals from blocks k, not 2^63 + k"
V_PLUS = "v recorded as v+"


def states(z, zv, S0, T, r, heston_params, n_steps, expiry_steps, dtype=np.float64, mutate=None):
    """z, zv: [>= last expiry step, n_paths] normals of the log-price and of the variance; heston_params = (q, v0, kappa,
    theta, xi, rho); n_steps: the job's step count (dt = T / n_steps, whatever the last expiry is).  Returns
    (S[m, path], v[m, path]) at the expiry steps, in dtype; v is the raw variance."""
    q, v0, kappa, theta, xi, rho = heston_params
    dt_ = np.dtype(dtype)
    f = dt_.type
    steps = [int(s) for s in expiry_steps]
    assert all(a < b for a, b in zip([0] + steps[:-1], steps)) and steps[-1] <= n_steps
    if mutate == LATE_EXPIRY:
        steps = [min(s + 1, n_steps) for s in steps]
    if mutate == SAME_BLOCKS:
        zv = z
    z, zv = z.astype(dt_), zv.astype(dt_)
    dt = f(T) / f(n_steps)
    sqrt_dt = np.sqrt(dt)
    mu = f(r) - f(q)
    rho_c = f(np.sqrt(np.float64(1.0) - np.float64(rho) * np.float64(rho)))
    rho, kappa, theta, xi = f(rho), f(kappa), f(theta), f(xi)
    n = z.shape[1]
    X = np.zeros(n, dtype=dt_)
    v = np.full(n, f(v0), dtype=dt_)
    S_out = np.empty((len(steps), n), dtype=dt_)
    v_out = np.empty((len(steps), n), dtype=dt_)
    m = 0
    for i in range(steps[-1]):
        vp = np.maximum(v, f(0))
        s = np.sqrt(vp)
        w = rho * z[i] + rho_c * zv[i]
        X = X + ((mu - vp / f(2)) * dt + (s * sqrt_dt) * z[i])
        v = v + (kappa * (theta - vp) * dt + (xi * s * sqrt_dt) * w)
        while m < len(steps) and steps[m] == i + 1:
            S_out[m] = f(S0) * np.exp(X)
            v_out[m] = np.maximum(v, f(0)) if mutate == V_PLUS else v
            m += 1
    return S_out, v_out
