"""GPU tests of the in-kernel Greeks (mcamd_price_greeks and friends).  Run with -m gpu on an MI355X.

  * exact restatement: a numpy restatement from the engine's own Philox stream (oracle.normal2_f64 / normal4_f32,
    global path id as subsequence) reproduces the 12 record sums.  The sums hold terms of both signs, so the
    tolerance is relative to the sum of the terms' magnitudes: 1e-10 in fp64; in fp32 the allowances of the
    price_paths oracle tests (2e-5 for the price, 2e-3 where a path within rounding of the strike or the barrier can
    flip an indicator);
  * statistics: |estimate - closed form| <= 4.5 SE, and every SE below a stated fraction of the value."""
import importlib
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

BENCH = dict(S0=100.0, T=1.0, K=100.0, r=0.1, v=0.2)
WINDOW = dict(B=120.0, P1=10, P2=50, use_window=1)
PW, LR = capi.GREEKS_PATHWISE, capi.GREEKS_LIKELIHOOD_RATIO


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    import os
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    c = capi.Context(0, stream.cuda_stream)
    yield c
    c.close()
    torch.cuda.set_stream(torch.cuda.default_stream())


def normals(oracle, prec, seed, path_ids, n_sim):
    """[len(path_ids), n_sim] normals of the engine's stream: subsequence = global path id, blocks from 0"""
    nb = 2 if prec == capi.F64 else 4
    blocks = (n_sim + nb - 1) // nb
    gen = oracle.normal2_f64 if prec == capi.F64 else oracle.normal4_f32
    z = np.empty((len(path_ids), blocks * nb))
    for i, p in enumerate(path_ids):
        for b in range(blocks):
            z[i, b * nb:(b + 1) * nb] = gen(seed, int(p), b)
    return z[:, :n_sim]


def restate(oracle, opt, sim, method):
    """per-path samples [n, 6] of the six estimators, in fp64 from the engine's normals"""
    n_sim = sim.n_steps - opt.Tk
    dt = opt.dt if opt.dt > 0 else opt.T / sim.n_steps
    S_s = opt.Sk if opt.Sk != 0 else opt.S0
    r, v, T, K = opt.r, opt.v, opt.T, opt.K
    Th = n_sim * dt
    z = normals(oracle, sim.precision, sim.seed, range(sim.path_offset, sim.path_offset + sim.n_paths_local), n_sim)
    logs = np.cumsum((r - 0.5 * v * v) * dt + v * math.sqrt(dt) * z, axis=1)
    L = logs[:, -1]
    St = S_s * np.exp(L)
    y = np.maximum(St - K, 0.0)
    if opt.use_window:
        logB = math.log(opt.B / S_s) if opt.B > 0 else -np.inf
        count = opt.Ik + (logB > logs).sum(axis=1)
        y = np.where((count >= opt.P1) & (count <= opt.P2), y, 0.0)
    q = np.zeros((len(y), 6))
    q[:, 0] = y
    if method == PW:
        itm = St > K
        q[:, 1] = np.where(itm, St / S_s, 0.0)
        q[:, 2] = np.where(itm, K * (L - (r - v * v / 2) * Th) / (S_s ** 2 * v * v * Th), 0.0)
        q[:, 3] = np.where(itm, St * (L - (r + v * v / 2) * Th) / v, 0.0)
        q[:, 4] = -T * y + np.where(itm, St * Th, 0.0)
        if opt.Tk == 0 and opt.dt == 0:
            q[:, 5] = r * y - np.where(itm, St * ((r - v * v / 2) + (L - (r - v * v / 2) * T) / (2 * T)), 0.0)
    else:
        z1, sz, szz, sq = z[:, 0], z.sum(axis=1), (z * z).sum(axis=1), math.sqrt(dt)
        q[:, 1] = y * z1 / (S_s * v * sq)
        q[:, 2] = y * ((z1 * z1 - 1) / (S_s ** 2 * v * v * dt) - z1 / (S_s ** 2 * v * sq))
        q[:, 3] = y * ((szz - n_sim) / v - sq * sz)
        q[:, 4] = y * (sz * sq / v - T)
    return q


def assert_record(got, q, prec, window):
    rt_price = 1e-10 if prec == capi.F64 else (2e-3 if window else 2e-5)
    rt = 1e-10 if prec == capi.F64 else 2e-3
    for k, name in enumerate(capi.GREEK_NAMES):
        tol = (rt_price if k == 0 else rt)
        s1, s2 = q[:, k].sum(), (q[:, k] ** 2).sum()
        assert abs(got.sum[k] - s1) <= tol * np.abs(q[:, k]).sum() + 1e-300, (name, got.sum[k], s1)
        assert abs(got.sumsq[k] - s2) <= 2 * tol * s2 + 1e-300, (name, got.sumsq[k], s2)


CASES = [   # (method, option overrides, n_steps, paths, path_offset)
    (PW, {}, 1, 2001, 0),
    (PW, {}, 7, 2001, 0),
    (PW, {}, 64, 3000, 1_000_003),
    (PW, {}, 253, 1501, 0),
    (PW, dict(Sk=95.0, Tk=20), 64, 2001, 0),
    (PW, dict(dt=1.0 / 50), 64, 1501, 0),
    (LR, {}, 7, 2001, 0),
    (LR, {}, 64, 2001, 77),
    (LR, WINDOW, 64, 3000, 0),
    (LR, WINDOW, 253, 1501, 5),
    (LR, dict(WINDOW, Ik=4, Sk=93.5, Tk=37, P1=5, P2=60), 100, 2001, 0),
]


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("method,extra,n_steps,n,lo", CASES)
def test_record_restates_exactly(ctx, oracle, prec, method, extra, n_steps, n, lo):
    opt = capi.make_option(**dict(BENCH, **extra))
    sim = capi.make_sim(lo + n + 10, n_steps, prec, seed=4321, path_offset=lo, n_paths_local=n)
    got = ctx.price_greeks(opt, sim, method)
    assert got.n == n and got.method == method and got.kernel_ms > 0 and got.grid >= 1 and got.block == 256
    assert_record(got, restate(oracle, opt, sim, method), prec, bool(opt.use_window))


# fp32 LR without a window steps another loop than the pair-sum pricer (rounding ~1e-6 per path): fp64 only there.
# The 4M-path bullet job is one that mcamd_price_paths runs on its lane-compacting kernel.
@pytest.mark.parametrize("prec,method,window,n", [(p, m, w, n) for p in (capi.F64, capi.F32)
                                                  for m, w, n in ((PW, False, 1_000_003), (LR, False, 1_000_003),
                                                                  (LR, True, 200_001), (LR, True, 4_000_000))
                                                  if not (p == capi.F32 and m == LR and not w)])
def test_price_sum_equals_price_paths(ctx, prec, method, window, n):
    opt = capi.make_option(**BENCH, **(WINDOW if window else {}))
    sim = capi.make_sim(n, 100, prec, seed=99)
    g = ctx.price_greeks(opt, sim, method)
    p = ctx.price_paths(opt, sim)
    assert g.n == p.n
    assert math.isclose(g.sum[0], p.sum, rel_tol=1e-12) and math.isclose(g.sumsq[0], p.sumsq, rel_tol=1e-12)
    assert math.isclose(g.value[0], p.price, rel_tol=1e-12)
    assert math.isclose(g.std_err[0], p.std_err, rel_tol=1e-9)


CLOSED = [dict(BENCH), dict(S0=120.0, T=1.0, K=100.0, r=0.05, v=0.25), dict(S0=90.0, T=1.0, K=110.0, r=0.05, v=0.3),
          dict(S0=100.0, T=0.1, K=100.0, r=0.03, v=0.2)]


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("o", CLOSED)
def test_pathwise_within_se_of_closed_form(ctx, prec, o):
    opt = capi.make_option(**o)
    g = ctx.price_greeks(opt, capi.make_sim(10_000_000, 252, prec, seed=2024), PW)
    bs = capi.bs_greeks_f64(o["S0"], o["K"], o["T"], o["r"], o["v"])
    for k, name in enumerate(capi.GREEK_NAMES):
        assert abs(g.value[k] - bs[k]) <= 4.5 * g.std_err[k], (name, g.value[k], bs[k], g.std_err[k])
        assert 0 < g.std_err[k] < 0.02 * abs(bs[k]), (name, g.std_err[k], bs[k])


@pytest.mark.parametrize("o", CLOSED[:3])
def test_likelihood_ratio_within_se_of_closed_form(ctx, o):
    opt = capi.make_option(**o)
    sim = capi.make_sim(50_000_000, 12, capi.F64, seed=77)
    g = ctx.price_greeks(opt, sim, LR)
    bs = capi.bs_greeks_f64(o["S0"], o["K"], o["T"], o["r"], o["v"])
    for k, name in enumerate(capi.GREEK_NAMES[:5]):
        assert abs(g.value[k] - bs[k]) <= 4.5 * g.std_err[k], (name, g.value[k], bs[k], g.std_err[k])
        assert 0 < g.std_err[k] < 0.02 * abs(bs[k]), (name, g.std_err[k], bs[k])
    pw = ctx.price_greeks(opt, sim, PW)
    assert pw.std_err[capi.GREEK_DELTA] < g.std_err[capi.GREEK_DELTA]
    assert pw.std_err[capi.GREEK_GAMMA] < g.std_err[capi.GREEK_GAMMA]


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("n_steps", [12, 50])
def test_window_that_never_closes_is_the_window_less_lr(ctx, prec, n_steps):
    sim = capi.make_sim(300_001, n_steps, prec, seed=8)
    a = ctx.price_greeks(capi.make_option(**BENCH, B=120.0, P1=0, P2=n_steps, use_window=1), sim, LR)
    b = ctx.price_greeks(capi.make_option(**BENCH), sim, LR)
    for k in range(5):
        assert math.isclose(a.sum[k], b.sum[k], rel_tol=1e-13) and math.isclose(a.sumsq[k], b.sumsq[k], rel_tol=1e-13)


def test_bullet_lr_matches_crn_finite_differences(ctx):
    # the reference's bullet window (hello.cu: B = 120, P1 = 10, P2 = 50, 100 steps); common random numbers = same seed
    n, seed = 100_000_000, 31
    base = dict(BENCH, **WINDOW)
    sim = capi.make_sim(n, 100, capi.F64, seed=seed)
    g = ctx.price_greeks(capi.make_option(**base), sim)
    assert g.method == LR and math.isnan(g.value[capi.GREEK_THETA])
    for k, key, h in ((capi.GREEK_DELTA, "S0", 1.0), (capi.GREEK_VEGA, "v", 0.002), (capi.GREEK_RHO, "r", 0.001)):
        up = ctx.price_paths(capi.make_option(**dict(base, **{key: base[key] + h})), sim)
        dn = ctx.price_paths(capi.make_option(**dict(base, **{key: base[key] - h})), sim)
        fd = (up.price - dn.price) / (2 * h)
        bound = 4.5 * (g.std_err[k] + (up.std_err + dn.std_err) / (2 * h))
        assert abs(g.value[k] - fd) <= bound, (capi.GREEK_NAMES[k], g.value[k], fd, bound)


def test_shards_group_and_empty_shard(ctx):
    n = 2_000_003
    for opt, method in ((capi.make_option(**BENCH), PW), (capi.make_option(**BENCH, **WINDOW), LR)):
        whole = ctx.price_greeks(opt, capi.make_sim(n, 64, capi.F64, seed=5), method)
        stats = torch.full((2, capi.GREEKS_STATS), -1.0, dtype=torch.float64, device="cuda")
        cut = 777_777
        ctx.price_greeks_enqueue(opt, capi.make_sim(n, 64, capi.F64, seed=5, n_paths_local=cut), stats[0], method)
        ctx.price_greeks_enqueue(opt, capi.make_sim(n, 64, capi.F64, seed=5, path_offset=cut, n_paths_local=n - cut),
                                 stats[1], method)
        torch.cuda.synchronize()
        s = stats.sum(dim=0).tolist()
        assert s[12] == n and s[13:] == [0.0, 0.0, 0.0]
        fin = capi.finalize_greeks_stats(s, opt.r, opt.T, theta_defined=(method == PW))
        assert fin.n == whole.n
        for k in range(6):
            assert math.isclose(fin.sum[k], whole.sum[k], rel_tol=1e-12, abs_tol=1e-300)
            assert math.isclose(fin.sumsq[k], whole.sumsq[k], rel_tol=1e-12, abs_tol=1e-300)
        assert all(m > 0 for m in ctx.enqueued_kernel_ms(2))
        with capi.Group(0) as grp:
            gg = grp.price_greeks(opt, capi.make_sim(n, 64, capi.F64, seed=5), method)
            assert gg.n == n and gg.method == method and gg.kernel_ms > 0
            for k in range(6):
                assert math.isclose(gg.sum[k], whole.sum[k], rel_tol=1e-12, abs_tol=1e-300)
            assert math.isclose(gg.value[1], whole.value[1], rel_tol=1e-12)
            empty = grp.price_greeks(opt, capi.make_sim(10, 5, capi.F64, n_paths_local=0), method)
            assert empty.n == 0 and list(empty.sum) == [0.0] * 6
    empty = ctx.price_greeks(capi.make_option(**BENCH), capi.make_sim(10, 5, capi.F64, n_paths_local=0))
    assert empty.n == 0 and list(empty.sum) == [0.0] * 6 and list(empty.sumsq) == [0.0] * 6
    st = torch.full((capi.GREEKS_STATS,), -1.0, dtype=torch.float64, device="cuda")
    ctx.price_greeks_enqueue(capi.make_option(**BENCH), capi.make_sim(10, 5, capi.F64, n_paths_local=0), st)
    torch.cuda.synchronize()
    assert st.tolist() == [0.0] * capi.GREEKS_STATS


def test_theta_conventions_and_refusals(ctx):
    sim = capi.make_sim(100_000, 20, capi.F64, seed=3)
    assert math.isfinite(ctx.price_greeks(capi.make_option(**BENCH), sim, PW).value[capi.GREEK_THETA])
    for opt, method in ((capi.make_option(**BENCH), LR), (capi.make_option(**BENCH, **WINDOW), LR),
                        (capi.make_option(**BENCH, Sk=95.0, Tk=5), PW), (capi.make_option(**BENCH, dt=1.0 / 20), PW)):
        g = ctx.price_greeks(opt, sim, method)
        assert math.isnan(g.value[capi.GREEK_THETA]) and math.isnan(g.std_err[capi.GREEK_THETA]), (method, opt.Tk)
        assert all(math.isfinite(g.value[k]) for k in range(5))
    # AUTO: pathwise without a window, LR with one
    assert ctx.price_greeks(capi.make_option(**BENCH), sim).method == PW
    assert ctx.price_greeks(capi.make_option(**BENCH, **WINDOW), sim).method == LR
    with pytest.raises(capi.McamdError, match="pathwise"):
        ctx.price_greeks(capi.make_option(**BENCH, **WINDOW), sim, PW)
    for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_CONTROL_VARIATE, capi.FLAG_PRODUCT_FORM, capi.FLAG_SEPARATE_REDUCE):
        with pytest.raises(capi.McamdError, match="flags"):
            ctx.price_greeks(capi.make_option(**BENCH), capi.make_sim(1000, 20, capi.F64, flags=flags))
    g = ctx.price_greeks(capi.make_option(**BENCH), capi.make_sim(1000, 20, capi.F64, flags=capi.FLAG_LOG_SPACE))
    assert g.n == 1000
    with pytest.raises(capi.McamdError):   # the exponent-range check of mcamd_price_paths
        ctx.price_greeks(capi.make_option(S0=100.0, T=1.0, K=100.0, r=0.1, v=900.0), capi.make_sim(1000, 1, capi.F64))
    with pytest.raises(capi.McamdError):
        ctx.price_greeks_enqueue(capi.make_option(**BENCH), sim, None)
