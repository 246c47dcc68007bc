"""GPU tests of the Heston pricer (mcamd_price_heston).  Run with -m gpu on an MI355X.  Everything elementwise goes
through d_samples (y) and d_state (S_T, then the raw v_n).

  1. y, S_T and v_n elementwise, truncated_steps and mean_variance against the numpy restatement
     (tests/heston_restate.py) on the two normal streams drawn from the oracle's rocRAND-exact generator for (seed,
     global path id, block): 256 paths at global ids 5003.. under seed 77 with 50, 3, 5 and 1 steps, and 7 steps on the
     deep inputs of tests/deep_inputs.py — every remainder of the last Philox block in both precisions, and a path
     shorter than one block.  Inputs F and N in both precisions and H in fp64, three strikes each; H in fp32 for
     finiteness and a truncation count within 25 % of the fp64 kernel's (under 82 % truncation fp32 paths diverge
     pathwise: tests/test_heston_cpu.py records it);
  2. xi = 0, kappa = 0 against mcamd_price_localvol's own samples on a flat 1 x 2 surface at sqrt(v0), same q, seed and
     ids: any mix-up of the two streams fails here;
  3. the streams are independent: at rho = 0 another xi changes v_n on every path and, after one step, no S_T; at rho = 1
     the variance stream is not read (the restatement fed garbage for it gives the kernel's samples);
  4. shards, repeats, the enqueue form, eight calls enqueued back to back, an empty shard;
  5. one statistical run, 2M paths x 128 steps on F in both precisions, within 4 SE of mcamd_heston_price_f64 (what 513
     paths cannot catch: the grid stride, path ids across workgroups);
  6. every refusal with a live context: MCAMD_ERR_INVALID, and the context still prices afterwards.

Tolerance of 1 to 3 (tests/heston_cases.py, from the restatement alone, computed on the CPU): four times the largest
difference between the float64 and longdouble restatements (fp64 kernels) or the float32 and float64 ones (fp32
kernels) over 256 paths x 50 steps of that input, floored at 1e-11 S0 (fp64) / 2e-3 (fp32) for S_T and y and at 1e-11 /
2e-5 for the variances.  Measured on an x86-64 CPU: S_T spreads of 2.6e-14 / 1.7e-5 (F), 3.3e-13 / 5.1e-5 (N) and
2.2e-11 / 2.8e-2 (H), so the floors decide everywhere but H in fp32, which is not compared elementwise.  No path is left
out: the step map is continuous.  In fp64 truncated_steps is exact; in fp32 it may differ by the number of paths whose
restated |v_i| comes within 1e-6 of 0, at most 2 % of a case (at most 2 of 256 paths on these inputs).
The kernels themselves, on an MI355X, over all cases of test 1: S_T within 4.4e-13 (F), 3.7e-13 (N) and 8.9e-11 (H) of
the restatement in fp64 and 2.6e-5 (F), 5.8e-5 (N) in fp32; v_n within 7.6e-16, 2.7e-15, 6.1e-13 and 4.2e-8, 2.3e-7;
truncated_steps equal to the restated count in every case of both precisions; in test 2 at most 2.8e-14 / 1.5e-5 from
mcamd_price_localvol's samples; in test 5 at most 1.42 SE from the closed form."""
import ctypes as C
import importlib

import numpy as np
import pytest

import heston_cases as hc
import heston_restate as hr
from deep_inputs import DEEP, SHALLOW

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

S0, T_, R, Q = hr.S0, hr.T_, hr.R, hr.Q_DIV
N_LOCAL = 256
PRECS = (capi.F64, capi.F32)
SUM_RTOL = 1e-13
# (n_steps, where)
SHAPES = ((50, SHALLOW), (3, SHALLOW), (5, SHALLOW), (7, DEEP), (1, SHALLOW))

torch = pytest.importorskip("torch")
TORCH_T = {capi.F64: torch.float64, capi.F32: torch.float32}


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


def option(K):
    # v and B are ignored by the call: leave something in them that any use would show
    return capi.make_option(S0=S0, K=K, r=R, T=T_, v=float("nan"), B=float("nan"))


def model(name, payoff, **changes):
    q, v0, kappa, theta, xi, rho = hr.params(name, **changes)
    return capi.make_heston(payoff, q, v0, kappa, theta, xi, rho)


def run(ctx, sim, K, hs, outputs=True):
    """(result, y, S_T, v_n as float64 numpy, or None)"""
    n = sim.n_paths_local
    y = state = None
    if outputs:
        y = torch.full((max(n, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
        state = torch.full((2 * max(n, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    res = ctx.price_heston(option(K), sim, hs, y, state)
    torch.cuda.synchronize()
    if not outputs:
        return res, None, None, None
    st = state.cpu().numpy().astype(np.float64)
    return res, y[:n].cpu().numpy().astype(np.float64), st[:n], st[n:2 * n]


def shard(prec, n_steps, where, n=N_LOCAL):
    seed, first, n_job = where
    return capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=n)


def full_work(n, n_steps):
    return 64 * -(-n // 64) * n_steps


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- 1. against the restatement ----------------------------------------------------------------------------------------

PARITY = [pytest.param(prec, name, shape, id=f"{prec}-{name}-{shape[0]}" + ("-deep" if shape[1] == DEEP else ""))
          for shape in SHAPES for name, precs in (("F", PRECS), ("N", PRECS), ("H", (capi.F64,))) for prec in precs]


@pytest.mark.parametrize("prec,name,shape", PARITY)
def test_samples_state_and_counters_against_the_restatement(ctx, prec, name, shape):
    n_steps, where = shape
    tol = hc.tolerance(prec, name)
    for K, payoff in hr.STRIKES:
        want = hc.restate(prec, name, n_steps, where, N_LOCAL, (K, payoff), np.float64)
        res, y, S_T, v_n = run(ctx, shard(prec, n_steps, where), K, model(name, payoff))
        assert np.isfinite(y).all() and np.isfinite(S_T).all() and np.isfinite(v_n).all()
        assert (res.n, res.block, res.grid) == (N_LOCAL, 256, 1) and res.work_steps == full_work(N_LOCAL, n_steps)
        err = {"y": np.abs(y - f64(want["y"])).max(), "S_T": np.abs(S_T - f64(want["S_T"])).max(),
               "v_n": np.abs(v_n - f64(want["v_n"])).max(),
               "rv": abs(res.mean_variance - float(f64(want["rv"]).mean()))}
        near = int((want["min_abs_v"] < hc.NEAR_ZERO).sum())
        print(f"{name} fp{prec} {n_steps} steps K {K}: deviations " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()) +
              f"; tolerances " + ", ".join(f"{k} {tol[k]:.1e}" for k in err) +
              f"; truncated {res.truncated_steps:.0f} (restated {int(want['trunc'].sum())}, paths near zero {near})")
        for k in err:
            assert err[k] <= tol[k], (k, err[k], tol[k])
        if prec == capi.F64:
            assert res.truncated_steps == float(want["trunc"].sum())
        else:
            assert near <= hc.NEAR_CAP * N_LOCAL and abs(res.truncated_steps - float(want["trunc"].sum())) <= near
        if n_steps == 1:
            assert res.truncated_steps == 0 and abs(res.mean_variance - hr.MODELS[name][0]) <= tol["rv"]
        # the sums are those of the samples: in fp32 the kernel sums the fp32 payoff widened, which is what it stored
        assert abs(res.sum - y.sum()) <= 1e-12 * max(abs(y).sum(), 1.0)
        assert abs(res.sumsq - (y * y).sum()) <= 1e-12 * max((y * y).sum(), 1.0)
        fin = capi.finalize(res.sum, res.sumsq, res.n, R, T_)
        assert (res.price, res.std_err, res.ci_lo, res.ci_hi) == (fin.price, fin.std_err, fin.ci_lo, fin.ci_hi)


@pytest.mark.parametrize("n_steps,where", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_heavy_truncation_in_fp32_stays_finite_and_counts_like_fp64(ctx, n_steps, where):
    K, payoff = hr.STRIKES[1]
    wide, *_ = run(ctx, shard(capi.F64, n_steps, where), K, model("H", payoff))
    narrow, y, S_T, v_n = run(ctx, shard(capi.F32, n_steps, where), K, model("H", payoff))
    assert np.isfinite(y).all() and np.isfinite(S_T).all() and np.isfinite(v_n).all() and (S_T > 0).all()
    print(f"H {n_steps} steps: truncated {narrow.truncated_steps:.0f} (fp32) {wide.truncated_steps:.0f} (fp64) of "
          f"{N_LOCAL * n_steps}; mean variance {narrow.mean_variance:.5f} and {wide.mean_variance:.5f}")
    assert abs(narrow.truncated_steps - wide.truncated_steps) <= 0.25 * wide.truncated_steps
    if n_steps >= 50:
        assert wide.truncated_steps > 0.5 * N_LOCAL * n_steps


# ---- 2. the constant-variance path is mcamd_price_localvol's --------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n_steps,where", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_constant_variance_against_the_localvol_samples(ctx, prec, n_steps, where):
    v0 = hr.MODELS["F"][0]
    tol = hc.tolerance(prec, "F")
    sim = shard(prec, n_steps, where)
    with ctx.localvol_surface((1, 2, -1.0, 1.0), [[np.sqrt(v0), np.sqrt(v0)]]) as flat:
        def localvol(K, payoff):
            s = torch.full((N_LOCAL,), float("nan"), dtype=TORCH_T[prec], device="cuda")
            ctx.price_localvol(option(K), sim, capi.make_localvol(payoff, q=Q), flat, s)
            torch.cuda.synchronize()
            return s.cpu().numpy().astype(np.float64)
        for K, payoff in hr.STRIKES:
            res, y, S_T, v_n = run(ctx, sim, K, model("F", payoff, xi=0.0, kappa=0.0, theta=0.3))
            want = localvol(K, payoff)
            # a call struck at 1 is in the money on every path: its sample plus 1 is S_T
            spot = localvol(1.0, hr.CALL) + 1.0
            assert (spot > 2.0).all()
            err_y, err_s = np.abs(y - want).max(), np.abs(S_T - spot).max()
            print(f"fp{prec} {n_steps} steps K {K}: worst deviation from mcamd_price_localvol y {err_y:.3e} S_T {err_s:.3e} "
                  f"(tolerance {tol['y']:.1e})")
            assert err_y <= tol["y"] and err_s <= tol["S_T"]
            assert (v_n == NP_OF[prec](v0)).all() and res.truncated_steps == 0
            assert abs(res.mean_variance - v0) <= tol["rv"]


NP_OF = {capi.F64: np.float64, capi.F32: np.float32}


# ---- 3. the two streams ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_variance_stream_moves_the_variance_alone_at_zero_correlation(ctx, prec):
    K, payoff = hr.STRIKES[1]
    for n_steps in (1, 6):
        sim = shard(prec, n_steps, SHALLOW)
        _, _, S_a, v_a = run(ctx, sim, K, model("F", payoff, rho=0.0, xi=0.3))
        _, _, S_b, v_b = run(ctx, sim, K, model("F", payoff, rho=0.0, xi=0.6))
        assert (v_a != v_b).all()
        # v_0 + xi sqrt(v0 dt) z' - theta-terms that cancel: the first step's variance moves in proportion to xi
        if n_steps == 1:
            v0 = hr.MODELS["F"][0]
            assert np.array_equal(S_a, S_b)          # the first step reads v0 alone
            assert np.abs((v_b - v0) - 2.0 * (v_a - v0)).max() <= hc.tolerance(prec, "F")["v_n"]
        else:
            assert (S_a != S_b).mean() > 0.99        # later steps read the variance, and so the other stream


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rho", [1.0, -1.0])
def test_variance_stream_is_not_read_at_full_correlation(ctx, prec, rho):
    n_steps = 6
    K, payoff = hr.STRIKES[1]
    z, zv = hr.draws(prec, SHALLOW[0], SHALLOW[1], N_LOCAL, n_steps)
    garbage = 1e3 * np.cos(np.arange(zv.size, dtype=np.float64)).reshape(zv.shape)
    p = hr.params("N", rho=rho)
    want = hr.samples(z, garbage, S0, K, T_, R, p, payoff, np.float64)
    same = hr.samples(z, zv, S0, K, T_, R, p, payoff, np.float64)
    assert np.array_equal(want["S_T"], same["S_T"]) and np.array_equal(want["v_n"], same["v_n"])
    res, y, S_T, v_n = run(ctx, shard(prec, n_steps, SHALLOW), K, model("N", payoff, rho=rho))
    tol = hc.tolerance(prec, "N")
    assert np.abs(S_T - want["S_T"]).max() <= tol["S_T"] and np.abs(v_n - want["v_n"]).max() <= tol["v_n"]
    assert np.abs(y - f64(want["y"])).max() <= tol["y"]


# ---- 4. plumbing ---------------------------------------------------------------------------------------------------------

def counted(r):
    return (r.sum, r.sumsq, r.truncated_steps, r.mean_variance, r.work_steps, r.n)


@pytest.mark.parametrize("prec", PRECS)
def test_three_shards_add_up_to_the_whole_job(ctx, prec):
    n, n_steps = 513, 12
    K, payoff = hr.STRIKES[1]
    hs = model("N", payoff)
    whole, y, S_T, v_n = run(ctx, capi.make_sim(n, n_steps, prec, seed=3), K, hs)
    assert whole.grid == 3 and whole.truncated_steps > 0
    parts = []
    for lo, hi in ((0, 100), (100, 101), (101, 513)):
        sim = capi.make_sim(n, n_steps, prec, seed=3, path_offset=lo, n_paths_local=hi - lo)
        part, y_p, S_p, v_p = run(ctx, sim, K, hs)
        assert np.array_equal(y_p, y[lo:hi]) and np.array_equal(S_p, S_T[lo:hi]) and np.array_equal(v_p, v_n[lo:hi])
        parts.append(part)
    assert abs(sum(p.sum for p in parts) - whole.sum) <= SUM_RTOL * abs(whole.sum)
    assert abs(sum(p.sumsq for p in parts) - whole.sumsq) <= SUM_RTOL * whole.sumsq
    assert sum(p.truncated_steps for p in parts) == whole.truncated_steps
    assert abs(sum(p.mean_variance * p.n for p in parts) - whole.mean_variance * n) <= SUM_RTOL * whole.mean_variance * n
    assert sum(p.n for p in parts) == whole.n == n


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [3000, 3_000_000])   # one wave of workgroups; beyond the 8192-workgroup cap (grid-stride)
def test_same_bits_twice_and_from_the_enqueue_form(ctx, prec, n):
    n_steps = 13
    K, payoff = hr.STRIKES[0]
    hs = model("N", payoff)
    sim = capi.make_sim(n + 9, n_steps, prec, seed=4, path_offset=9, n_paths_local=n)
    a, y_a, S_a, v_a = run(ctx, sim, K, hs)
    b, y_b, S_b, v_b = run(ctx, sim, K, hs)
    assert np.array_equal(y_a, y_b) and np.array_equal(S_a, S_b) and np.array_equal(v_a, v_b) and counted(a) == counted(b)
    assert a.grid == min(-(-n // 256), 8192) and a.sum > 0 and a.work_steps == full_work(n, n_steps)
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    y = torch.full((n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    state = torch.full((2 * n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    ctx.price_heston_enqueue(option(K), sim, hs, stats, y, state)
    ms = ctx.enqueued_kernel_ms(1)
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    assert rec[:3].tolist() == [a.sum, a.sumsq, a.truncated_steps] and rec[4:].tolist() == [0.0, float(n)]
    assert rec[3] / n == a.mean_variance
    assert np.array_equal(y.cpu().numpy().astype(np.float64), y_a)
    assert np.array_equal(state.cpu().numpy().astype(np.float64), np.concatenate([S_a, v_a]))
    fin = capi.finalize_stats(rec, R, T_)
    assert (fin.price, fin.std_err, fin.n) == (a.price, a.std_err, n)
    assert 0.0 < ms[0] < 1e4


def test_eight_calls_enqueued_back_to_back(ctx):
    n, n_steps = 5000, 9
    jobs = [(prec, name, strike, seed) for seed, (prec, name, strike) in enumerate(
        [(capi.F64, "F", 0), (capi.F32, "N", 1), (capi.F64, "H", 0), (capi.F32, "F", 2), (capi.F64, "N", 0),
         (capi.F32, "H", 1), (capi.F64, "F", 1), (capi.F32, "N", 2)])]
    stats = torch.full((len(jobs), 6), float("nan"), dtype=torch.float64, device="cuda")
    sims = [capi.make_sim(n, n_steps, prec, seed=40 + seed) for prec, _, _, seed in jobs]
    for row, (sim, (prec, name, strike, _)) in enumerate(zip(sims, jobs)):
        ctx.price_heston_enqueue(option(hr.STRIKES[strike][0]), sim, model(name, hr.STRIKES[strike][1]), stats[row])
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    for row, (sim, (prec, name, strike, _)) in enumerate(zip(sims, jobs)):
        res, *_ = run(ctx, sim, hr.STRIKES[strike][0], model(name, hr.STRIKES[strike][1]), False)
        assert rec[row].tolist() == [res.sum, res.sumsq, res.truncated_steps, rec[row][3], 0.0, float(n)]
        assert rec[row][3] / n == res.mean_variance and res.sum > 0
    assert len({tuple(r) for r in rec}) == len(jobs)


def test_an_empty_shard_launches_nothing(ctx):
    sim = capi.make_sim(1000, 12, path_offset=10, n_paths_local=0)
    res, *_ = run(ctx, sim, 100.0, model("F", hr.CALL), False)
    assert all(v == 0 for v in res.as_dict().values())
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    ctx.price_heston_enqueue(option(100.0), sim, model("F", hr.CALL), stats)
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()


# ---- 5. one statistical run ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_two_million_paths_within_4_se_of_the_closed_form(ctx, prec):
    q, v0, kappa, theta, xi, rho = hr.params("F")
    for k, (K, payoff) in enumerate(hr.STRIKES):
        res, *_ = run(ctx, capi.make_sim(2_000_000, 128, prec, seed=2050 + k), K, model("F", payoff), False)
        want = capi.heston_price(S0, K, T_, R, q, v0, kappa, theta, xi, rho, payoff)
        print(f"F fp{prec} K {K}: closed {want:.5f} price {res.price:.5f} SE {res.std_err:.5f} "
              f"({(res.price - want) / res.std_err:+.2f} SE), truncated {res.truncated_steps / (2e6 * 128):.5f} of the "
              f"steps, mean variance {res.mean_variance:.5f}, kernel {res.kernel_ms:.3f} ms")
        assert res.std_err > 0 and abs(res.price - want) <= 4.0 * res.std_err
        assert res.grid == 2_000_000 // 256 + 1 and res.work_steps == full_work(2_000_000, 128)
        assert abs(res.mean_variance - theta) <= 1e-3   # v0 = theta: the variance's mean stays there but for truncation


# ---- 6. refusals with a live context ----------------------------------------------------------------------------------------

def test_refusals_reach_no_device_and_leave_the_context_usable(ctx):
    from test_heston_cpu import refusals
    L, h = ctx._L, ctx._h
    ref = lambda x: None if x is None else C.byref(x)
    K, payoff = hr.STRIKES[1]
    before, y_before, *_ = run(ctx, shard(capi.F64, 5, SHALLOW), K, model("F", payoff))
    stats = torch.zeros(6, dtype=torch.float64, device="cuda")
    n_cases = 0
    for name, (opt, sim, hs), kw, words in refusals():
        if name == "no context":
            continue
        out = capi.HestonResult()
        rc = L.mcamd_price_heston(h, ref(opt), ref(sim), ref(hs), None, None, C.byref(out) if kw.get("res", True) else None)
        assert rc == capi.ERR_INVALID and words in L.mcamd_last_error().decode(), name
        assert all(v == 0 for v in out.as_dict().values())
        if kw.get("res", True):
            rc = L.mcamd_price_heston_enqueue(h, ref(opt), ref(sim), ref(hs), None, None, C.c_void_p(stats.data_ptr()))
            assert rc == capi.ERR_INVALID and words in L.mcamd_last_error().decode(), name
        n_cases += 1
    assert n_cases > 60
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()
    after, y_after, *_ = run(ctx, shard(capi.F64, 5, SHALLOW), K, model("F", payoff))
    assert counted(after) == counted(before) and np.array_equal(y_after, y_before)
