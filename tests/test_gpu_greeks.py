"""GPU tests of the in-kernel Greeks (mcamd_price_greeks and friends).  Run with -m gpu on an MI355X.

  * exact restatement: a numpy restatement from the engine's own Philox stream (oracle.normal2_f64 / normal4_f32,
    global path id as subsequence) reproduces the 12 record sums.  The sums hold terms of both signs, so the
    tolerance is relative to the sum of the terms' magnitudes: 1e-10 in fp64; in fp32 the allowances of the
    price_paths oracle tests (2e-5 for the price, 2e-3 where a path within rounding of the strike or the barrier can
    flip an indicator);
  * statistics: |estimate - closed form| <= 4.5 SE, and every SE below a stated fraction of the value;
  * path by path (test_every_path_restates): a Greeks call has no per-path output, but a shard of one path is that
    path's six samples.  256 consecutive paths from ids 5003.. under seed 77 and from ids 2^33 + 5003.. of a 2^40-path
    job under seed 2^40 + 77, at 1, 2, 3, 5, 6, 7 simulated steps: every remainder of the last Philox block, and the LR
    kernel's branch for a path shorter than one block (fp32: 1 to 3 steps, fp64: 1).  Cases, restatements, tolerance
    and the paths left out in fp32: tests/greeks_cases.py; what they rest on is checked without a kernel in
    tests/test_greeks_cpu.py;
  * small shards (test_small_shards_and_what_each_adds): n_paths_local of 1..5, 63..65, 255..257 and 513, each record
    and the difference of consecutive records against exactly the restated paths;
  * the short-path launch rule (test_short_lr_paths_walk_the_grid_stride): ceil(32 / n_sim) paths a thread.

The per-path tolerance is four times the largest elementwise difference between two restatements, floored at 1e-10
(fp64) / 2e-5 for the price and 2e-3 for the others (fp32) of max(|q|, mean |q| of the case).  Largest restatement
differences, measured on an x86-64 CPU (80-bit longdouble), price delta gamma vega rho theta:
    pathwise  fp64 3.4e-14 4.2e-16 1.0e-16 2.6e-13 1.5e-14 2.9e-14    fp32 2.6e-5 2.9e-7 5.7e-8 1.6e-4 1.6e-5 2.4e-5
    LR        fp64 3.4e-14 8.5e-15 3.4e-15 2.2e-12 6.5e-13 -          fp32 2.8e-5 5.0e-6 1.1e-6 1.7e-3 4.7e-4 -
so the floor decides everywhere but for the fp32 price of the cases with a small mean price (the restarts and dt = 1/50:
4 x 2.8e-5 = 1.1e-4 against 2e-5 x 3.6 to 5.5).  Largest
deviations of the kernels from the float64 restatement on an MI355X, over all cases, same order:
    pathwise  fp64 8.5e-14 8.9e-16 1.7e-16 5.7e-13 3.7e-14 5.0e-14    fp32 4.4e-5 4.0e-7 1.2e-7 1.9e-4 1.2e-5 1.8e-5
    LR        fp64 8.5e-14 1.8e-14 5.3e-15 5.2e-12 1.4e-12 -          fp32 2.0e-5 8.2e-6 1.2e-6 1.4e-3 4.1e-4 -
The fp32 price comes closest to its tolerance, at 0.22 of it; the pathwise kernel's pair sums (about an ulp per pair off
rocRAND's two normals) fit the fp32 floors as they are, and no floor is widened."""
import importlib
import math

import numpy as np
import pytest

import greeks_cases as gc
from greeks_restate import restate

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
    assert_record(got, restate(oracle, opt, sim, method).q, prec, bool(opt.use_window))


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


# ---- path by path: shards of one path (inputs, restatements and tolerance: tests/greeks_cases.py) ---------------------------

def enqueue_records(ctx, opt, sims, method):
    """the 16-double statistics records of the shards `sims`, [len(sims), 16]: one launch each, one synchronize"""
    stats = torch.full((len(sims), capi.GREEKS_STATS), float("nan"), dtype=torch.float64, device="cuda")
    for row, sim in zip(stats, sims):
        ctx.price_greeks_enqueue(opt, sim, row, method)
    torch.cuda.synchronize()
    return stats.cpu().numpy()


def square_tolerance(want, tol):
    """what |q - want| <= tol allows q^2 to differ from want^2 by: twice the relative bound, and its square"""
    return 2.0 * tol * np.abs(want) + tol * tol


def report(name, prec, err, tol, left):
    worst = np.where(left, 0.0, err).max(axis=0)
    share = np.where(left, 0.0, err / np.maximum(tol, 1e-300)).max(axis=0)
    print(f"{name} prec {prec}: left out {left.any(axis=1).sum()}; largest deviation (and share of its tolerance) " +
          "  ".join(f"{n} {w:.2e} ({s:.3f})" for n, w, s in zip(capi.GREEK_NAMES, worst, share)))


@pytest.mark.parametrize("prec", gc.PRECS)
@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_every_path_restates(ctx, prec, case):
    """n_paths_local = 1 and path_offset = id: sum[k] is the path's sample q_k and sumsq[k] its square"""
    want, tol, left = gc.wanted(case, prec)
    assert left.any(axis=1).sum() <= gc.MAX_LEFT_OUT and not (prec == capi.F64 and left.any())
    first = case.where[1]
    rec = enqueue_records(ctx, gc.option(case), [gc.sim(case, prec, first=first + i, n_local=1) for i in range(gc.N_PATHS)],
                          case.method)
    assert np.isfinite(rec).all() and (rec[:, 12] == 1).all() and not rec[:, 13:].any()
    got, gotsq = rec[:, 0:12:2], rec[:, 1:12:2]
    err = np.abs(got - want)
    report(case.name, prec, err, tol, left)
    bad = np.argwhere(~((err <= tol) | left))
    assert len(bad) == 0, [(first + i, capi.GREEK_NAMES[k], got[i, k], want[i, k], tol[i, k]) for i, k in bad[:8]]
    assert ((np.abs(gotsq - want * want) <= square_tolerance(want, tol)) | left).all()
    assert np.allclose(gotsq, got * got, rtol=1e-15, atol=0.0)    # one path: the record's square is its sum's


@pytest.mark.parametrize("prec", gc.PRECS)
@pytest.mark.parametrize("case", gc.SHARD_CASES, ids=lambda c: c.name)
def test_small_shards_and_what_each_adds(ctx, prec, case):
    """Shards of 1.. paths from the same first path: each record against the fp64 sum of exactly its paths' restated
    samples, and the difference of two consecutive records against the paths the larger shard adds — the second path
    of a pair-sum thread, the first lane of a second wavefront, the first thread of a second block.  Tolerance: the
    per-path one, summed over the paths in question (the records are fp64 sums: their own rounding, some 1e-15 of the
    sum of magnitudes, is far below it)."""
    sizes = gc.shard_sizes(case)
    want, tol, left = gc.wanted(case, prec, max(sizes))
    assert not left.any()      # a sum leaves no path out (tests/test_greeks_cpu.py: none is near a jump)
    rec = enqueue_records(ctx, gc.option(case), [gc.sim(case, prec, n_local=m) for m in sizes], case.method)
    assert np.isfinite(rec).all() and rec[:, 12].tolist() == list(sizes) and not rec[:, 13:].any()
    sq, sqtol = want * want, square_tolerance(want, tol)
    lo, before = 0, np.zeros(12)
    for m, r in zip(sizes, rec[:, :12]):
        for a, what in ((0, "shard"), (lo, "added")):
            got, gotsq = (r - (before if a else 0.0))[0::2], (r - (before if a else 0.0))[1::2]
            err, bound = np.abs(got - want[a:m].sum(axis=0)), tol[a:m].sum(axis=0)
            print(f"{case.name} prec {prec} paths {a}..{m - 1} ({what}): largest share of the tolerance {(err / np.maximum(bound, 1e-300)).max():.3f}")
            assert (err <= bound).all(), (m, what, got, want[a:m].sum(axis=0), bound)
            assert (np.abs(gotsq - sq[a:m].sum(axis=0)) <= sqtol[a:m].sum(axis=0)).all(), (m, what)
        lo, before = m, r


@pytest.mark.parametrize("prec", gc.PRECS)
@pytest.mark.parametrize("n_steps", [1, 2, 3])
def test_short_lr_paths_walk_the_grid_stride(ctx, prec, n_steps):
    """Below 32 steps the LR launch gives each thread ceil(32 / n_sim) paths, walked by grid stride: 20 001 paths of 1, 2
    and 3 steps run on 3, 5 and 8 workgroups, 27, 16 and 10 paths a thread.  The whole job against its ten shards of
    2001 and 2000 paths (the same samples in another order of summation: 1e-12 of sqrt(n sum q^2) >= sum |q|), and the
    first shard against the restatement (per-path tolerance, summed)."""
    n, shard = 20_001, 2000
    case = gc.Case(f"lr-{n_steps}-stride", LR, {}, n_steps, gc.SHALLOW)
    opt, first = gc.option(case), case.where[1]
    per_thread = -(-32 // n_steps)
    blocks = -(-(-(-n // per_thread)) // 256)
    assert per_thread == {1: 32, 2: 16, 3: 11}[n_steps] and 1 <= blocks < 8192    # the cap of one_path_per_thread_grid is far
    whole = ctx.price_greeks(opt, gc.sim(case, prec, n_local=n), LR)
    assert whole.n == n and whole.grid == blocks and whole.block == 256
    assert -(-n // (blocks * 256)) == {1: 27, 2: 16, 3: 10}[n_steps]      # grid-stride trips of a thread
    cuts = [0, shard + 1] + [shard + 1 + shard * i for i in range(1, 10)]
    assert cuts[-1] == n and len(cuts) == 11
    rec = enqueue_records(ctx, opt, [gc.sim(case, prec, first=first + a, n_local=b - a, n_job=first + n)
                                     for a, b in zip(cuts[:-1], cuts[1:])], LR)
    assert rec[:, 12].tolist() == [b - a for a, b in zip(cuts[:-1], cuts[1:])] and not rec[:, 13:].any()
    total = rec[:, :12].sum(axis=0)
    for k in range(6):
        scale = math.sqrt(n * whole.sumsq[k])
        assert abs(total[2 * k] - whole.sum[k]) <= 1e-12 * scale, (k, total[2 * k], whole.sum[k])
        assert abs(total[2 * k + 1] - whole.sumsq[k]) <= 1e-12 * whole.sumsq[k], (k, total[2 * k + 1], whole.sumsq[k])
    assert all(whole.sumsq[k] > 0 for k in range(5)) and whole.sumsq[5] == 0.0
    want, tol, left = gc.wanted(case, prec, shard + 1)
    assert not left.any()
    err, bound = np.abs(rec[0, 0:12:2] - want.sum(axis=0)), tol.sum(axis=0)
    print(f"{case.name} prec {prec}: grid {whole.grid}; first shard, largest share of the tolerance {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all(), (rec[0, 0:12:2], want.sum(axis=0), bound)
    assert (np.abs(rec[0, 1:12:2] - (want * want).sum(axis=0)) <= square_tolerance(want, tol).sum(axis=0)).all()
