"""GPU tests of the Heston barrier pricer (mcamd_price_heston_barrier).  Run with -m gpu on an MI355X.  Everything
elementwise goes through d_samples (y) and d_state (S_T, the raw v_n, w).

  1. y, S_T, v_n and w elementwise, live_steps, truncated_steps and mean_variance against the numpy restatement
     (tests/heston_barrier_restate.py) on the two normal streams drawn from the oracle's rocRAND-exact generator: 1024
     paths at global ids 5003.. under seed 77 with 50, 3, 5 and 1 steps, and 7 steps on the deep inputs of
     tests/deep_inputs.py; inputs F and N in both precisions and H in fp64; 4 kinds x 2 monitorings x call / put each.
     A knock-out path that was hit: NaN, NaN and 0 in d_state and 0 in d_samples;
  2. against kernels already trusted: with a barrier nobody reaches d_samples, S_T and v_n are mcamd_price_heston's bit
     for bit; with xi = 0, kappa = 0 the samples are those of mcamd_price_localvol's own barrier on a flat 1 x 2
     surface, in all 16 cases, at the tolerance tests/test_gpu_heston.py uses for its flat-surface comparison;
  3. early exit: an up-and-out at B = 1.0001 S0 runs fewer wave-steps than the full count, and three of its paths — hit
     at step 1, hit late, never hit — priced as shards of one path each give the same bits;
  4. shards, repeats, the enqueue form, eight calls enqueued back to back, an empty shard, every refusal with a live
     context;
  5. the exact check of tests/test_heston_barrier_cpu.py on the device: rho = 0, r = q, 2^18 paths x 16 steps, the
     down-and-out call and the up-and-in put in both precisions, |mean(y_j - c_j)| <= 4 SE(y_j - c_j) with c_j from the
     numpy-restated variance paths of the same ids.

Tolerances and the left-out rule of 1 and 2: tests/heston_barrier_cases.py, from the restatement alone, computed on the
CPU (tests/test_heston_barrier_cpu.py prints the spreads).  The counters are exact where no path is left out; otherwise
they may differ by n_steps per left-out path, and an fp32 truncation count by the paths whose restated |v| comes within
heston_cases.NEAR_ZERO of 0 as well.
The kernels themselves, on an MI355X, over all cases of test 1: y within 6.6e-13 (F), 3.6e-12 (N) and 4.3e-10 (H) of the
restatement in fp64 and 6.0e-5 (F), 2.2e-4 (N) in fp32, against 1e-9 and 2e-3; w within 2.4e-14, 4.5e-13, 5.4e-12 and
5.1e-6, 1.4e-5, against 1e-11 (H: 1.5e-11) and 2e-5 (N: 8.5e-5); in test 2 at most 2.8e-14 / 1.5e-5 from
mcamd_price_localvol's barrier samples; in test 5 between -1.03 and +0.13 SE.  In test 3 some 7.5 % of the paths
survive all 50 steps, so few wavefronts of 64 lose every lane early: the seeds are ones where the restatement has some."""
import ctypes as C
import importlib

import numpy as np
import pytest

import barrier_restate as br
import heston_barrier_cases as hbc
import heston_barrier_restate as hbr
import heston_cases as hc
import heston_restate as hr
from deep_inputs import DEEP, SHALLOW

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

S0, T_, R, Q = hr.S0, hr.T_, hr.R, hr.Q_DIV
K = hbc.STRIKE
N = hbc.N_PATHS
PRECS = (capi.F64, capi.F32)
SUM_RTOL = 1e-13

torch = pytest.importorskip("torch")
TORCH_T = {capi.F64: torch.float64, capi.F32: torch.float32}
NP_OF = {capi.F64: np.float64, capi.F32: np.float32}


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


def option(B, r=R):
    # v is ignored by the call: leave something in it that any use would show
    return capi.make_option(S0=S0, K=K, r=r, T=T_, v=float("nan"), B=B)


def model(name, payoff, **changes):
    q, v0, kappa, theta, xi, rho = hr.params(name, **changes)
    return capi.make_heston(payoff, q, v0, kappa, theta, xi, rho)


def run(ctx, sim, case, hs, B=None, outputs=True, r=R):
    """(result, y, S_T, v_n, w as float64 numpy, or None).  case: (kind, monitoring, payoff)"""
    kind, mon, payoff = case
    n = sim.n_paths_local
    y = state = None
    if outputs:
        y = torch.full((max(n, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
        state = torch.full((3 * max(n, 1),), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    res = ctx.price_heston_barrier(option(hbc.LEVEL[kind] if B is None else B, r), sim, hs,
                                   capi.make_barrier(kind, payoff, mon), y, state)
    torch.cuda.synchronize()
    if not outputs:
        return res, None, None, None, None
    st = state.cpu().numpy().astype(np.float64)
    return res, y[:n].cpu().numpy().astype(np.float64), st[:n], st[n:2 * n], st[2 * n:3 * n]


def shard(prec, n_steps, where, n=N):
    seed, first, n_job = where
    return capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=n)


def full_work(n, n_steps):
    return 64 * -(-n // 64) * n_steps


def f64(a):
    return np.asarray(a, dtype=np.float64)


def counted_steps(res, case, n_steps):
    return res.live_steps if br.is_out(case[0]) else float(res.n) * n_steps


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- 1. against the restatement ----------------------------------------------------------------------------------------

PARITY = [pytest.param(prec, name, shape, id=f"{prec}-{name}-{shape[0]}" + ("-deep" if shape[1] == DEEP else ""))
          for shape in hbc.SHAPES for name, precs in hbc.ELEMENTWISE for prec in precs]


@pytest.mark.parametrize("prec,name,shape", PARITY)
def test_samples_state_and_counters_against_the_restatement(ctx, prec, name, shape):
    n_steps, where = shape
    tol = hbc.tolerance(prec, name)
    worst = dict.fromkeys(("y", "S_T", "v_n", "w", "mv"), 0.0)
    for case in hbc.CASES:
        kind, mon, payoff = case
        out = br.is_out(kind)
        want = hbc.restate(prec, name, n_steps, where, N, case, np.float64)
        keep = hbc.kept(prec, name, n_steps, where, N, case)
        left = N - int(keep.sum())
        assert left <= hbc.LEFT_CAP * N
        res, y, S_T, v_n, w = run(ctx, shard(prec, n_steps, where), case, model(name, payoff))
        assert (res.n, res.block, res.grid) == (N, 256, 4)
        assert np.isfinite(y).all() and ((w >= 0) & (w <= 1)).all()
        # the convention for a knocked path of a knock-out, on every path: hit ones have no state, the others have one
        knocked = np.isnan(S_T)
        assert np.array_equal(knocked, np.isnan(v_n))
        if out:
            assert (w[knocked] == 0).all() and (y[knocked] == 0).all() and (w[~knocked] > 0).all()
            assert np.array_equal(knocked[keep], ~want["alive"][keep])
            assert res.work_steps <= full_work(N, n_steps)
        else:
            assert not knocked.any() and res.work_steps == full_work(N, n_steps)
        if mon == br.DISCRETE:
            assert set(np.unique(w)) <= {0.0, 1.0}
        defined = keep & ~knocked
        assert defined.any()
        err = {"y": np.abs(y - f64(want["y"]))[keep].max(), "w": np.abs(w - f64(want["w"]))[keep].max(),
               "S_T": np.abs(S_T - f64(want["S_T"]))[defined].max(), "v_n": np.abs(v_n - f64(want["v_n"]))[defined].max()}
        # the counters: exact but for left-out paths (and, in fp32, paths whose variance grazes zero)
        assert abs(res.live_steps - float(want["live"].sum())) <= left * n_steps
        near = int((want["min_abs_v"] < hc.NEAR_ZERO).sum()) if prec == capi.F32 else 0
        assert near <= hc.NEAR_CAP * N
        assert abs(res.truncated_steps - float(want["trunc"].sum())) <= left * n_steps + near
        counted = counted_steps(res, case, n_steps)
        assert counted >= N
        vs_sum = float(f64(want["vs"]).sum())
        slack = left * n_steps * float(want["max_vp"].max())
        err["mv"] = max(abs(res.mean_variance * counted - vs_sum) - slack, 0.0) / counted
        for k in err:
            worst[k] = max(worst[k], float(err[k]))
            assert err[k] <= tol[k], (case, k, err[k], tol[k])
        # the sums are those of the samples: the kernel sums y as it forms it, in fp64, and stores it in the path
        # precision, so in fp32 a stored sample is y rounded to 24 bits (half an ulp: 2^-24 of it at the most)
        rounding = 1e-12 if prec == capi.F64 else 2.0 ** -24
        assert abs(res.sum - y.sum()) <= rounding * max(abs(y).sum(), 1.0)
        assert abs(res.sumsq - (y * y).sum()) <= 2.5 * rounding * max((y * y).sum(), 1.0)
        fin = capi.finalize(res.sum, res.sumsq, res.n, R, T_)
        assert (res.price, res.std_err, res.ci_lo, res.ci_hi) == (fin.price, fin.std_err, fin.ci_lo, fin.ci_hi)
    print(f"{name} fp{prec} {n_steps} steps: worst deviations " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()) +
          "; tolerances " + ", ".join(f"{k} {tol[k]:.1e}" for k in worst))


# ---- 2. against kernels already trusted -----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["N", "H"])
def test_unreachable_barrier_is_mcamd_price_heston(ctx, prec, name):
    n, n_steps = 1000, 13
    sim = capi.make_sim(n + 7, n_steps, prec, seed=11, path_offset=7, n_paths_local=n)
    for payoff in (br.CALL, br.PUT):
        hs = model(name, payoff)
        y_e = torch.full((n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
        st_e = torch.full((2 * n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
        european = ctx.price_heston(option(float("nan")), sim, hs, y_e, st_e)
        torch.cuda.synchronize()
        y_e, st_e = y_e.cpu().numpy().astype(np.float64), st_e.cpu().numpy().astype(np.float64)
        assert european.truncated_steps > 0
        for kind in br.KINDS:
            B = 1e30 if br.is_up(kind) else 1e-30
            for mon in (br.DISCRETE, br.CONTINUOUS):
                res, y, S_T, v_n, w = run(ctx, sim, (kind, mon, payoff), hs, B=B)
                assert np.array_equal(S_T, st_e[:n]) and np.array_equal(v_n, st_e[n:]) and (w == 1).all()
                assert res.truncated_steps == european.truncated_steps and res.live_steps == n * n_steps
                assert res.work_steps == full_work(n, n_steps) == european.work_steps
                assert abs(res.mean_variance - european.mean_variance) <= 1e-12 * european.mean_variance
                if br.is_out(kind):
                    assert np.array_equal(y, y_e) and (res.sum, res.sumsq) == (european.sum, european.sumsq)
                else:
                    assert not y.any() and res.sum == 0


FLAT_SHAPES = ((50, SHALLOW), (5, SHALLOW), (7, DEEP), (1, SHALLOW))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n_steps,where", FLAT_SHAPES, ids=[str(s[0]) for s in FLAT_SHAPES])
def test_constant_variance_against_the_localvol_barrier_samples(ctx, prec, n_steps, where):
    v0 = hr.MODELS["F"][0]
    flat_model = dict(xi=0.0, kappa=0.0, theta=0.3)
    tol = hc.tolerance(prec, "F")   # what tests/test_gpu_heston.py allows between the two kernels on a flat surface
    sim = shard(prec, n_steps, where)
    worst = 0.0
    with ctx.localvol_surface((1, 2, -1.0, 1.0), [[np.sqrt(v0), np.sqrt(v0)]]) as flat:
        for case in hbc.CASES:
            kind, mon, payoff = case
            s = torch.full((N,), float("nan"), dtype=TORCH_T[prec], device="cuda")
            lv = ctx.price_localvol(option(hbc.LEVEL[kind]), sim, capi.make_localvol(payoff, kind, mon, q=Q), flat, s)
            torch.cuda.synchronize()
            want = s.cpu().numpy().astype(np.float64)
            res, y, S_T, v_n, w = run(ctx, sim, case, model("F", payoff, **flat_model))
            # s s against v+: the two walks differ by a rounding, which the strict hit test may turn into a payoff
            keep = hbc.kept(prec, "F", n_steps, where, N, case, **flat_model)
            left = N - int(keep.sum())
            assert left <= hbc.LEFT_CAP * N
            err = np.abs(y - want)[keep].max()
            worst = max(worst, float(err))
            assert err <= tol["y"], (case, err)
            assert abs(res.live_steps - lv.live_steps) <= left * n_steps and res.truncated_steps == 0
            assert (v_n[~np.isnan(v_n)] == NP_OF[prec](v0)).all()
            assert abs(res.mean_variance - v0) <= hbc.tolerance(prec, "F")["mv"]
    print(f"fp{prec} {n_steps} steps: worst deviation from mcamd_price_localvol's barrier samples {worst:.3e} "
          f"(tolerance {tol['y']:.1e})")


# ---- 3. early exit ----------------------------------------------------------------------------------------------------------

# At this level some 7.5 % of the paths survive all 50 steps, so a wavefront of 64 seldom loses every lane before its last
# Philox block.  The seeds are ones under which the restatement (numpy's Philox normals, on the CPU) has such
# wavefronts: two of the 64 in fp64 under seed 40, one in fp32 under seed 32.
EARLY_SEED = {capi.F64: 40, capi.F32: 32}


def wave_steps(live, alive, n_steps, per_block):
    """the steps each wavefront of 64 consecutive paths runs: up to the end of the first whole Philox block at which
    every lane has been hit (a path hit at step s entered s steps live), else all of them"""
    last_hit = np.where(alive, np.inf, live).reshape(-1, 64).max(axis=1)
    blocks = np.ceil(last_hit / per_block)
    return np.where(blocks <= n_steps // per_block, blocks * per_block, n_steps)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mon", [br.DISCRETE, br.CONTINUOUS])
def test_a_knock_out_wavefront_leaves_early_and_one_path_shards_give_the_same_bits(ctx, prec, mon):
    n, n_steps, seed = 4096, 50, EARLY_SEED[prec]
    per_block = 2 if prec == capi.F64 else 4
    B = S0 * 1.0001
    case = (br.UP_OUT, mon, br.PUT)
    hs = model("F", br.PUT)
    res, y, S_T, v_n, w = run(ctx, capi.make_sim(n, n_steps, prec, seed=seed), case, hs, B=B)
    print(f"fp{prec} monitoring {mon}: work_steps {res.work_steps:.0f} of {full_work(n, n_steps)}, live_steps "
          f"{res.live_steps:.0f}, lane efficiency {res.live_steps / res.work_steps:.3f}")
    assert res.work_steps < 64 * (n // 64) * n_steps and res.work_steps >= res.live_steps >= n
    # which paths: by the restatement on numpy's own Philox normals (to a rounding of the kernel's), away from the level
    normals = hr.philox_normals_f64 if prec == capi.F64 else hbr.philox_normals_f32
    z, zv = normals(seed, 0, n, n_steps), normals(seed, 0, n, n_steps, hr.VARIANCE_BLOCKS)
    want = hbr.samples(z, zv, S0, K, B, T_, R, hr.params("F"), br.UP_OUT, br.PUT, mon)
    hit = ~want["alive"]
    # the wave-steps are the restated ones, but for wavefronts that hold a path too close to the level to call
    steps = wave_steps(want["live"], want["alive"], n_steps, per_block)
    unsure = (want["min_abs_d"] < hbc.MARGIN).reshape(-1, 64).any(axis=1)
    assert (steps < n_steps).any() and not unsure[steps < n_steps].any()
    assert abs(res.work_steps - 64 * steps.sum()) <= 64 * n_steps * unsure.sum()
    assert abs(res.live_steps - want["live"].sum()) <= n_steps * (want["min_abs_d"] < hbc.MARGIN).sum()
    clear = want["min_abs_d"] >= 1e-4
    first = np.flatnonzero(clear & hit & (want["live"] == 1))
    late = np.flatnonzero(clear & hit & (want["live"] >= 20))
    alive = np.flatnonzero(clear & ~hit)
    assert len(first) and len(late) and len(alive)
    for p in (int(first[0]), int(late[-1]), int(alive[len(alive) // 2])):
        assert (w[p] == 0) == bool(hit[p]) and np.isnan(S_T[p]) == bool(hit[p])
        one = capi.make_sim(n, n_steps, prec, seed=seed, path_offset=p, n_paths_local=1)
        r1, y1, S1, v1, w1 = run(ctx, one, case, hs, B=B)
        assert same(y1, y[p:p + 1]) and same(S1, S_T[p:p + 1]) and same(v1, v_n[p:p + 1]) and same(w1, w[p:p + 1])
        # alone in its wavefront, the path leaves at the end of the block it was hit in
        alone = wave_steps(np.full(64, want["live"][p]), np.full(64, not hit[p]), n_steps, per_block)[0]
        assert r1.live_steps == want["live"][p] and r1.work_steps == 64 * alone
        if not hit[p]:
            assert alone == n_steps and y1[0] > 0


# ---- 4. plumbing ---------------------------------------------------------------------------------------------------------

def counted(r):
    return (r.sum, r.sumsq, r.live_steps, r.truncated_steps, r.mean_variance, r.work_steps, r.n)


PLUMBING = ((br.DOWN_OUT, br.CONTINUOUS, br.PUT), (br.UP_IN, br.CONTINUOUS, br.CALL), (br.UP_OUT, br.DISCRETE, br.CALL))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", PLUMBING, ids=lambda c: "-".join(map(str, c)))
def test_three_shards_add_up_to_the_whole_job(ctx, prec, case):
    n, n_steps = 513, 12
    hs = model("N", case[2])
    whole, y, S_T, v_n, w = run(ctx, capi.make_sim(n, n_steps, prec, seed=3), case, hs)
    assert whole.grid == 3 and whole.truncated_steps > 0 and 0 < (w == 0).sum() < n
    parts = []
    for lo, hi in ((0, 100), (100, 101), (101, 513)):
        sim = capi.make_sim(n, n_steps, prec, seed=3, path_offset=lo, n_paths_local=hi - lo)
        part, y_p, S_p, v_p, w_p = run(ctx, sim, case, hs)
        assert same(y_p, y[lo:hi]) and same(S_p, S_T[lo:hi]) and same(v_p, v_n[lo:hi]) and same(w_p, w[lo:hi])
        parts.append(part)
    assert abs(sum(p.sum for p in parts) - whole.sum) <= SUM_RTOL * abs(whole.sum)
    assert abs(sum(p.sumsq for p in parts) - whole.sumsq) <= SUM_RTOL * whole.sumsq
    assert sum(p.live_steps for p in parts) == whole.live_steps
    assert sum(p.truncated_steps for p in parts) == whole.truncated_steps
    vs = lambda r: r.mean_variance * counted_steps(r, case, n_steps)
    assert abs(sum(vs(p) for p in parts) - vs(whole)) <= SUM_RTOL * vs(whole)
    assert sum(p.n for p in parts) == whole.n == n


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [3000, 3_000_000])   # one wave of workgroups; beyond the 8192-workgroup cap (grid-stride)
def test_same_bits_twice_and_from_the_enqueue_form(ctx, prec, n):
    n_steps = 13
    case = PLUMBING[0] if prec == capi.F64 else PLUMBING[1]
    hs = model("N", case[2])
    bar = capi.make_barrier(*[case[0], case[2], case[1]])
    sim = capi.make_sim(n + 9, n_steps, prec, seed=4, path_offset=9, n_paths_local=n)
    a, y_a, S_a, v_a, w_a = run(ctx, sim, case, hs)
    b, y_b, S_b, v_b, w_b = run(ctx, sim, case, hs)
    assert same(y_a, y_b) and same(S_a, S_b) and same(v_a, v_b) and same(w_a, w_b) and counted(a) == counted(b)
    assert a.grid == min(-(-n // 256), 8192) and a.sum > 0 and n <= a.live_steps <= a.work_steps <= full_work(n, n_steps)
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    y = torch.full((n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    state = torch.full((3 * n,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    ctx.price_heston_barrier_enqueue(option(hbc.LEVEL[case[0]]), sim, hs, bar, stats, y, state)
    ms = ctx.enqueued_kernel_ms(1)
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    assert rec[:4].tolist() == [a.sum, a.sumsq, a.live_steps, a.truncated_steps] and rec[5] == float(n)
    assert rec[4] / counted_steps(a, case, n_steps) == a.mean_variance
    assert same(y.cpu().numpy().astype(np.float64), y_a)
    assert same(state.cpu().numpy().astype(np.float64), np.concatenate([S_a, v_a, w_a]))
    fin = capi.finalize_stats(rec, R, T_)
    assert (fin.price, fin.std_err, fin.n) == (a.price, a.std_err, n)
    assert 0.0 < ms[0] < 1e4


def test_eight_calls_enqueued_back_to_back(ctx):
    n, n_steps = 5000, 9
    jobs = [(prec, name, hbc.CASES[(5 * k) % 16]) for k, (prec, name) in enumerate(
        [(capi.F64, "F"), (capi.F32, "N"), (capi.F64, "H"), (capi.F32, "F"), (capi.F64, "N"), (capi.F32, "H"),
         (capi.F64, "F"), (capi.F32, "N")])]
    stats = torch.full((len(jobs), 6), float("nan"), dtype=torch.float64, device="cuda")
    sims = [capi.make_sim(n, n_steps, prec, seed=40 + k) for k, (prec, _, _) in enumerate(jobs)]
    for row, (sim, (prec, name, (kind, mon, payoff))) in enumerate(zip(sims, jobs)):
        ctx.price_heston_barrier_enqueue(option(hbc.LEVEL[kind]), sim, model(name, payoff),
                                         capi.make_barrier(kind, payoff, mon), stats[row])
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    for row, (sim, (prec, name, case)) in enumerate(zip(sims, jobs)):
        res, *_ = run(ctx, sim, case, model(name, case[2]), outputs=False)
        assert rec[row].tolist() == [res.sum, res.sumsq, res.live_steps, res.truncated_steps, rec[row][4], float(n)]
        assert rec[row][4] / counted_steps(res, case, n_steps) == res.mean_variance and res.sum > 0
    assert len({tuple(r) for r in rec}) == len(jobs)


def test_an_empty_shard_launches_nothing(ctx):
    sim = capi.make_sim(1000, 12, path_offset=10, n_paths_local=0)
    case = PLUMBING[0]
    res, *_ = run(ctx, sim, case, model("F", case[2]), outputs=False)
    assert all(v == 0 for v in res.as_dict().values())
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    ctx.price_heston_barrier_enqueue(option(hbc.LEVEL[case[0]]), sim, model("F", case[2]),
                                     capi.make_barrier(case[0], case[2], case[1]), stats)
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()


def test_refusals_reach_no_device_and_leave_the_context_usable(ctx):
    from test_heston_barrier_cpu import price, refusals
    L, h = ctx._L, ctx._h
    case = PLUMBING[0]
    before, y_before, *_ = run(ctx, shard(capi.F64, 5, SHALLOW), case, model("F", case[2]))
    stats = torch.zeros(6, dtype=torch.float64, device="cuda")
    n_cases = 0
    for name, args, kw, words in refusals():
        if name == "no context":
            continue
        rc, msg = price(L, *args, ctx=h, **kw)
        assert rc == capi.ERR_INVALID and words in msg, name
        if kw.get("res", True):
            rc, msg = price(L, *args, enqueue=True, ctx=h, stats=C.c_void_p(stats.data_ptr()), **kw)
            assert rc == capi.ERR_INVALID and words in msg, name
        n_cases += 1
    assert n_cases > 80
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()
    after, y_after, *_ = run(ctx, shard(capi.F64, 5, SHALLOW), case, model("F", case[2]))
    assert counted(after) == counted(before) and np.array_equal(y_after, y_before)


# ---- 5. the exact check on the device -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["F", "N"])
def test_quarter_million_paths_have_the_exact_conditional_expectation(ctx, prec, name):
    n, n_steps, seed = 2 ** 18, 16, 7100 + prec
    r, p = hbc.exact_inputs(name)
    normals = hr.philox_normals_f64 if prec == capi.F64 else hbr.philox_normals_f32
    clock = hbr.variance_clock(normals(seed, 0, n, n_steps, hr.VARIANCE_BLOCKS), T_, p)
    for kind, payoff in ((br.DOWN_OUT, br.CALL), (br.UP_IN, br.PUT)):
        case = (kind, br.CONTINUOUS, payoff)
        res, y, S_T, v_n, w = run(ctx, capi.make_sim(n, n_steps, prec, seed=seed), case,
                                  model(name, payoff, q=r, rho=0.0), r=r)
        # the restated clock is the kernel's: a knock-in counts every step
        if not br.is_out(kind):
            assert abs(res.mean_variance * T_ - clock.mean()) <= (1e-11 if prec == capi.F64 else 2e-5)
        c = hbc.conditional_expectation(capi, clock, kind, payoff)
        mean, se = hbc.mean_in_standard_errors(y, c)
        print(f"{name} fp{prec} kind {kind} payoff {payoff}: mean y {y.mean():.5f}, mean c {c.mean():.5f}, mean(y - c) "
              f"{mean:+.2e} = {mean / se:+.2f} SE (SE {se:.2e}), kernel {res.kernel_ms:.3f} ms")
        assert se > 0 and abs(mean) <= 4.0 * se
