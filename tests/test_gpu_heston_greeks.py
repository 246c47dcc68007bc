"""GPU tests of the Heston Greeks (mcamd_price_heston_greeks, include/mcamd_heston_greeks.h).  Run with -m gpu on an
MI355X.  Everything elementwise goes through d_samples, the (3 + 2 P) x n rows of the path precision.

  1. the rows bit for bit, tolerance ZERO: 256 paths at global ids 5003.. under seed 77 with 50, 3, 5 and 1 steps, and 7
     steps on the deep inputs of tests/deep_inputs.py, in both precisions; inputs F and N, H in fp64 only; the three
     strikes, all five bumps and gamma_eta = 0.01.  Row 0 and every h+ / h- row equal the d_samples of a
     mcamd_price_heston call at the base or bumped model with the same seed and ids; rows 1 and 2 equal what numpy forms
     from that call's d_state S_T by the header's definitions; truncated_steps and mean_variance equal that call's.
     Every bump must move a sample (after ONE step only v0 can: X_1 reads v_0 alone, and there the other four rows must
     equal row 0 instead);
  2. subsets: with P = 0 (gamma only), 1, 2, 3 and 4 of the parameters requested, the rows and values present equal those
     of the full request bit for bit, and what was not requested is 0: every P instantiation runs;
  3. sums: value and std_err against the numpy finalize of the returned rows to 1e-13 relative; three shards add up to
     the whole job; two runs and the enqueue form give the same bits at 3000 and at 3 000 000 paths; eight calls
     enqueued back to back; an empty shard;
  4. one statistical run per precision, 2^20 paths x 128 steps on F, K = 100 call and K = 80 put, P = 5 with gamma:
     every value within 4 std_err + 2 b_k of mcamd_heston_greeks_f64, b_k the scheme bias measured on the CPU
     (tests/heston_greeks_cases.py);
  5. every refusal with a live context: MCAMD_ERR_INVALID, and the context still prices afterwards."""
import ctypes as C
import importlib

import numpy as np
import pytest

import heston_greeks_cases as gc
import heston_restate as hr
from deep_inputs import DEEP, SHALLOW

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
hg = importlib.import_module("monte-carlo-project-cuda_amd.heston_greeks")

S0, T_, R, Q = hr.S0, hr.T_, hr.R, hr.Q_DIV
N_LOCAL = 256
PRECS = (capi.F64, capi.F32)
NP_OF = {capi.F64: np.float64, capi.F32: np.float32}
SUM_RTOL = 1e-13
SHAPES = ((50, SHALLOW), (3, SHALLOW), (5, SHALLOW), (7, DEEP), (1, SHALLOW))
FULL = hg.make_job(gc.ETA, **gc.BUMPS)

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
    return capi.make_option(S0=S0, K=K, r=R, T=T_, v=float("nan"), B=float("nan"))


def heston_of(params, payoff):
    q, v0, kappa, theta, xi, rho = params
    return capi.make_heston(payoff, q, v0, kappa, theta, xi, rho)


def model(name, payoff):
    return heston_of(hr.params(name), payoff)


def shard(prec, n_steps, where, n=N_LOCAL):
    seed, first, n_job = where
    return capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=n)


def greeks(ctx, sim, K, hs, job, outputs=True):
    """(out, the rows in the path precision as a numpy array (3 + 2 P, n), or None)"""
    n = sim.n_paths_local
    rows = None
    if outputs:
        rows = torch.full((job.n_rows, max(n, 1)), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    out = ctx.price_heston_greeks(option(K), sim, hs, job, rows)
    torch.cuda.synchronize()
    return out, (rows[:, :n].cpu().numpy() if outputs else None)


def heston(ctx, sim, K, hs):
    """(result, y, S_T in the path precision) of mcamd_price_heston"""
    n = sim.n_paths_local
    y = torch.full((n,), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    state = torch.full((2 * n,), float("nan"), dtype=TORCH_T[sim.precision], device="cuda")
    res = ctx.price_heston(option(K), sim, hs, y, state)
    torch.cuda.synchronize()
    return res, y.cpu().numpy(), state[:n].cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def values(out):
    return list(out.value), list(out.std_err)


# ---- 1. the rows, bit for bit ----------------------------------------------------------------------------------------------

PARITY = [pytest.param(prec, name, shape, id=f"{prec}-{name}-{shape[0]}" + ("-deep" if shape[1] == DEEP else ""))
          for shape in SHAPES for name, precs in (("F", PRECS), ("N", PRECS), ("H", (capi.F64,))) for prec in precs]


@pytest.mark.parametrize("prec,name,shape", PARITY)
def test_rows_equal_the_heston_calls_bit_for_bit(ctx, prec, name, shape):
    n_steps, where = shape
    sim = shard(prec, n_steps, where)
    walks = gc.walks(name, gc.BUMPS)
    assert len(walks) == 11
    moved = dict.fromkeys(gc.PARAMS, False)
    for K, payoff in hr.STRIKES:
        out, rows = greeks(ctx, sim, K, model(name, payoff), FULL)
        assert rows.shape == (13, N_LOCAL) and rows.dtype == NP_OF[prec] and np.isfinite(rows).all()
        assert (out.n, out.block, out.grid) == (N_LOCAL, 256, 1)
        assert out.work_steps == 64 * -(-N_LOCAL // 64) * n_steps
        base, y, S_T = heston(ctx, sim, K, heston_of(walks[0][1], payoff))
        assert same_bits(rows[0], y)
        want = gc.rows_from_state(S_T, [], K, payoff, gc.ETA)
        assert same_bits(rows[1], want[1]) and same_bits(rows[2], want[2])
        assert ((rows[2] == 0) | (rows[2] == S_T)).all() and (rows[2] >= 0).all()   # S_T or 0, never negative
        assert (out.truncated_steps, out.mean_variance) == (base.truncated_steps, base.mean_variance)
        assert out.value[0] == base.price and out.std_err[0] == base.std_err
        for j, (label, params) in enumerate(walks[1:]):
            _, y_b, _ = heston(ctx, sim, K, heston_of(params, payoff))
            assert same_bits(rows[3 + j], y_b), (label, K)
        for j, p in enumerate(gc.PARAMS):
            moved[p] |= bool((rows[3 + 2 * j] != rows[4 + 2 * j]).any())
            if n_steps == 1 and p != "v0":   # X_1 reads v_0 alone
                assert same_bits(rows[3 + 2 * j], rows[0]) and same_bits(rows[4 + 2 * j], rows[0])
        print(f"{name} fp{prec} {n_steps} steps K {K}: in the money {int((rows[0] > 0).sum())}, gamma band "
              f"{int((rows[2] > 0).sum())}, rows that differ between + and - " +
              ", ".join(f"{p} {int((rows[3 + 2 * j] != rows[4 + 2 * j]).sum())}" for j, p in enumerate(gc.PARAMS)))
    assert moved["v0"], moved
    if n_steps > 1:
        assert all(moved.values()), moved   # the comparison above is not vacuous: every bump moves a sample


# ---- 2. subsets ------------------------------------------------------------------------------------------------------------

SUBSETS = [(), ("xi",), ("v0", "rho"), ("kappa", "theta", "xi"), ("v0", "kappa", "theta", "rho")]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("subset", SUBSETS, ids=[str(len(s)) for s in SUBSETS])
def test_a_subset_of_the_parameters_gives_the_full_requests_bits(ctx, prec, subset):
    sim = shard(prec, 5, SHALLOW)
    K, payoff = hr.STRIKES[1]
    hs = model("N", payoff)
    full, full_rows = greeks(ctx, sim, K, hs, FULL)
    job = hg.make_job(gc.ETA, **{p: gc.BUMPS[p] for p in subset})
    assert job.n_params == len(subset)
    out, rows = greeks(ctx, sim, K, hs, job)
    assert rows.shape == (3 + 2 * len(subset), N_LOCAL)
    assert same_bits(rows[:3], full_rows[:3])
    for j, p in enumerate(subset):
        k = gc.PARAMS.index(p)
        assert same_bits(rows[3 + 2 * j: 5 + 2 * j], full_rows[3 + 2 * k: 5 + 2 * k]), p
        assert (out.value[5 + k], out.std_err[5 + k]) == (full.value[5 + k], full.std_err[5 + k]) and out.std_err[5 + k] > 0
    for k, p in enumerate(gc.PARAMS):
        if p not in subset:
            assert (out.value[5 + k], out.std_err[5 + k]) == (0.0, 0.0)
    assert values(out)[0][:5] == values(full)[0][:5] and values(out)[1][:5] == values(full)[1][:5]
    assert (out.truncated_steps, out.mean_variance) == (full.truncated_steps, full.mean_variance)
    assert full.value[hg.GREEK_GAMMA] > 0 and full.std_err[hg.GREEK_GAMMA] > 0
    # without gamma: row 2 is all zeros, gamma is 0, the rest stays
    job0 = hg.make_job(0.0, **{p: gc.BUMPS[p] for p in subset})
    out0, rows0 = greeks(ctx, sim, K, hs, job0)
    assert not rows0[2].any() and same_bits(rows0[:2], rows[:2]) and same_bits(rows0[3:], rows[3:])
    assert (out0.value[hg.GREEK_GAMMA], out0.std_err[hg.GREEK_GAMMA]) == (0.0, 0.0)
    for k in range(hg.GREEKS):
        if k != hg.GREEK_GAMMA:
            assert (out0.value[k], out0.std_err[k]) == (out.value[k], out.std_err[k])


# ---- 3. sums and plumbing --------------------------------------------------------------------------------------------------

def exact_record(rows, trunc, rv_sum):
    """gc.record with exactly rounded sums (math.fsum): the reference carries no summation error of its own"""
    import math
    rows = np.asarray(rows, dtype=np.float64)
    P = (rows.shape[0] - 3) // 2
    y, d, g = rows[0], rows[1], rows[2]
    e = d - y
    cols = [y, y * y, d, d * d, e * e, g, g * g]
    for j in range(P):
        c = rows[3 + 2 * j] - rows[4 + 2 * j]
        cols += [c, c * c]
    rec = [math.fsum(c) for c in cols] + [float(trunc), float(rv_sum), float(rows.shape[1])]
    return np.array(rec + [0.0] * (gc.STATS - len(rec)))


def enqueue(ctx, sim, K, hs, job, rows=None):
    stats = torch.full((hg.STATS,), float("nan"), dtype=torch.float64, device="cuda")
    ctx.price_heston_greeks_enqueue(option(K), sim, hs, job, stats, rows)
    torch.cuda.synchronize()
    return stats.cpu().numpy()


@pytest.mark.parametrize("prec", PRECS)
def test_values_are_the_finalize_of_the_rows(ctx, prec):
    n, n_steps = 3000, 12
    for name, (K, payoff) in (("F", hr.STRIKES[1]), ("N", hr.STRIKES[0])):
        sim = capi.make_sim(n, n_steps, prec, seed=5)
        out, rows = greeks(ctx, sim, K, model(name, payoff), FULL)
        assert out.grid == 12
        rec = exact_record(rows, out.truncated_steps, out.mean_variance * n)
        value, se, _, _ = gc.finalize(rec, S0, R, T_, gc.ETA, gc.bump_list(gc.BUMPS))
        for k, what in enumerate(gc.NAMES):
            print(f"{name} fp{prec} {what}: value {out.value[k]:+.12g} (numpy {value[k]:+.12g}) std_err {out.std_err[k]:.6g} "
                  f"(numpy {se[k]:.6g})")
            assert se[k] > 0 and out.value[k] != 0
            assert abs(out.value[k] - value[k]) <= SUM_RTOL * abs(value[k]), what
            assert abs(out.std_err[k] - se[k]) <= SUM_RTOL * se[k], what


@pytest.mark.parametrize("prec", PRECS)
def test_three_shards_add_up_to_the_whole_job(ctx, prec):
    n, n_steps = 513, 12
    K, payoff = hr.STRIKES[1]
    hs = model("N", payoff)
    P = FULL.n_params
    whole_rows = torch.full((FULL.n_rows, n), float("nan"), dtype=TORCH_T[prec], device="cuda")
    whole = enqueue(ctx, capi.make_sim(n, n_steps, prec, seed=3), K, hs, FULL, whole_rows)
    whole_rows = whole_rows.cpu().numpy()
    assert whole[9 + 2 * P] == n and whole[7 + 2 * P] > 0 and not whole[10 + 2 * P:].any()
    total = np.zeros(hg.STATS)
    for lo, hi in ((0, 100), (100, 101), (101, 513)):
        sim = capi.make_sim(n, n_steps, prec, seed=3, path_offset=lo, n_paths_local=hi - lo)
        rows = torch.full((FULL.n_rows, hi - lo), float("nan"), dtype=TORCH_T[prec], device="cuda")
        total += enqueue(ctx, sim, K, hs, FULL, rows)
        assert same_bits(rows.cpu().numpy(), whole_rows[:, lo:hi])
    assert total[9 + 2 * P] == n and total[7 + 2 * P] == whole[7 + 2 * P]
    for k in range(9 + 2 * P):
        # sum c_p has both signs: its scale is sum |c_p| <= sqrt(n sum c_p^2), the slot behind it
        signed = 7 <= k < 7 + 2 * P and (k - 7) % 2 == 0
        scale = np.sqrt(n * whole[k + 1]) if signed else abs(whole[k])
        assert abs(total[k] - whole[k]) <= SUM_RTOL * scale, k
    a = hg.finalize_stats(total, option(K), FULL)
    b = hg.finalize_stats(whole, option(K), FULL)
    for k in range(hg.GREEKS):   # a mean moves by its summation error; a standard error through the variance's difference
        assert abs(a.value[k] - b.value[k]) <= 1e-10 * (abs(b.value[k]) + b.std_err[k] * np.sqrt(n)), k
        assert abs(a.std_err[k] - b.std_err[k]) <= 1e-10 * b.std_err[k], k


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [3000, 3_000_000])   # one wave of workgroups; beyond the 8192-workgroup cap (grid-stride)
def test_same_bits_twice_and_from_the_enqueue_form(ctx, prec, n):
    n_steps = 13
    K, payoff = hr.STRIKES[0]
    hs = model("N", payoff)
    sim = capi.make_sim(n + 9, n_steps, prec, seed=4, path_offset=9, n_paths_local=n)
    small = n <= 3000
    a, rows_a = greeks(ctx, sim, K, hs, FULL, small)
    b, rows_b = greeks(ctx, sim, K, hs, FULL, small)
    assert values(a) == values(b) and (a.truncated_steps, a.mean_variance, a.n) == (b.truncated_steps, b.mean_variance, n)
    assert a.grid == min(-(-n // 256), 8192) and a.value[0] > 0 and a.work_steps == 64 * -(-n // 64) * n_steps
    rows = torch.full((FULL.n_rows, n), float("nan"), dtype=TORCH_T[prec], device="cuda") if small else None
    rec = enqueue(ctx, sim, K, hs, FULL, rows)
    ms = ctx.enqueued_kernel_ms(1)
    if small:
        assert same_bits(rows_a, rows_b) and same_bits(rows.cpu().numpy(), rows_a)
    P = FULL.n_params
    assert rec[9 + 2 * P] == n and not rec[10 + 2 * P:].any()
    fin = hg.finalize_stats(rec, option(K), FULL)
    assert values(fin) == values(a)
    assert (fin.truncated_steps, fin.mean_variance, fin.n) == (a.truncated_steps, a.mean_variance, n)
    assert 0.0 < ms[0] < 1e4


def test_eight_calls_enqueued_back_to_back(ctx):
    n, n_steps = 5000, 9
    jobs = [(prec, name, strike, subset, 40 + seed) for seed, (prec, name, strike, subset) in enumerate(
        [(capi.F64, "F", 0, gc.PARAMS), (capi.F32, "N", 1, ()), (capi.F64, "H", 0, ("xi",)), (capi.F32, "F", 2, gc.PARAMS),
         (capi.F64, "N", 0, ("v0", "rho")), (capi.F32, "N", 1, ("kappa", "theta", "xi")), (capi.F64, "F", 1, ()),
         (capi.F32, "N", 2, ("v0", "kappa", "theta", "rho"))])]
    stats = torch.full((len(jobs), hg.STATS), float("nan"), dtype=torch.float64, device="cuda")
    made = []
    for row, (prec, name, strike, subset, seed) in enumerate(jobs):
        K, payoff = hr.STRIKES[strike]
        job = hg.make_job(gc.ETA, **{p: gc.BUMPS[p] for p in subset})
        sim, hs = capi.make_sim(n, n_steps, prec, seed=seed), model(name, payoff)
        made.append((sim, K, hs, job))
        ctx.price_heston_greeks_enqueue(option(K), sim, hs, job, stats[row])
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    for row, (sim, K, hs, job) in enumerate(made):
        out, _ = greeks(ctx, sim, K, hs, job, False)
        fin = hg.finalize_stats(rec[row], option(K), job)
        assert values(fin) == values(out) and fin.n == n and out.value[0] > 0
        assert (fin.truncated_steps, fin.mean_variance) == (out.truncated_steps, out.mean_variance)
        assert rec[row][9 + 2 * job.n_params] == n and not rec[row][10 + 2 * job.n_params:].any()
    assert len({tuple(r) for r in rec}) == len(jobs)


def test_an_empty_shard_launches_nothing(ctx):
    sim = capi.make_sim(1000, 12, path_offset=10, n_paths_local=0)
    out, _ = greeks(ctx, sim, 100.0, model("F", hr.CALL), FULL, False)
    assert not any(out.value) and not any(out.std_err)
    assert (out.n, out.truncated_steps, out.mean_variance, out.work_steps, out.kernel_ms, out.grid) == (0, 0, 0, 0, 0, 0)
    assert not enqueue(ctx, sim, 100.0, model("F", hr.CALL), FULL).any()


# ---- 4. one statistical run per precision ----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_a_million_paths_within_4_se_and_the_scheme_bias_of_the_closed_form(ctx, prec):
    q, v0, kappa, theta, xi, rho = hr.params("F")
    n = 2 ** 20
    for k, (K, payoff) in enumerate(gc.STAT_STRIKES):
        out, _ = greeks(ctx, capi.make_sim(n, gc.STAT_STEPS, prec, seed=3050 + k), K, model("F", payoff), FULL, False)
        want = hg.greeks_closed_form(S0, K, T_, R, q, v0, kappa, theta, xi, rho, payoff, gc.ETA, gc.bump_list(gc.BUMPS))
        bias = gc.BIAS[(K, payoff)]
        bad = []
        for i, what in enumerate(gc.NAMES):
            dev = out.value[i] - want[i]
            print(f"F fp{prec} K {K} {what:6s}: closed {want[i]:+.6f} estimate {out.value[i]:+.6f} SE {out.std_err[i]:.6f} "
                  f"({dev / out.std_err[i]:+.2f} SE; allowed 4 SE + 2 x {bias[i]:.2e})")
            if not (out.std_err[i] > 0 and abs(dev) <= 4.0 * out.std_err[i] + 2.0 * bias[i]):
                bad.append(what)
        print(f"kernel {out.kernel_ms:.3f} ms, truncated {out.truncated_steps / (n * gc.STAT_STEPS):.5f} of the steps")
        assert not bad, bad
        assert out.grid == n // 256 and out.n == n


# ---- 5. refusals with a live context ---------------------------------------------------------------------------------------

def test_refusals_reach_no_device_and_leave_the_context_usable(ctx):
    from test_heston_greeks_cpu import refusals
    L, h = hg.load(), ctx._h
    ref = lambda x: None if x is None else C.byref(x)
    K, payoff = hr.STRIKES[1]
    before, rows_before = greeks(ctx, shard(capi.F64, 5, SHALLOW), K, model("F", payoff), FULL)
    stats = torch.zeros(hg.STATS, dtype=torch.float64, device="cuda")
    n_cases = 0
    for name, (opt, sim, hs, job), kw, words in refusals():
        if name == "no context":
            continue
        out = hg.HestonGreeks()
        rc = L.mcamd_price_heston_greeks(h, ref(opt), ref(sim), ref(hs), ref(job), None,
                                         C.byref(out) if kw.get("res", True) else None)
        assert rc == capi.ERR_INVALID and words in L.mcamd_last_error().decode(), name
        assert not any(out.value) and not any(out.std_err) and out.n == 0
        if kw.get("res", True):
            rc = L.mcamd_price_heston_greeks_enqueue(h, ref(opt), ref(sim), ref(hs), ref(job), None,
                                                     C.c_void_p(stats.data_ptr()))
            assert rc == capi.ERR_INVALID and words in L.mcamd_last_error().decode(), name
        n_cases += 1
    assert n_cases > 80
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()
    after, rows_after = greeks(ctx, shard(capi.F64, 5, SHALLOW), K, model("F", payoff), FULL)
    assert values(after) == values(before) and same_bits(rows_after, rows_before)
