"""GPU tests of the local-volatility Greeks (mcamd_price_localvol_greeks).  Run with -m gpu on an MI355X.

  1. every sample of every path, through d_samples, against the numpy restatement (tests/localvol_greeks_restate.py) on
     the inputs and under the tolerance of tests/localvol_greeks_cases.py (1024 paths per case; the tolerance comes from
     the restatement alone); in every case sample row 0 is mcamd_price_localvol's d_samples, widened, bit for bit, and
     the record's sums are the sums of d_samples;
  2. shards of 1..5, 63..65, 255..257 and 513 paths against the sums of exactly their restated paths, and one job of
     8192 * 256 + 513 paths (a second grid-stride trip) against its two shards;
  3. within 4 SE: a flat surface against the closed-form Black-Scholes Greeks (q = 0) and against double-precision
     central differences of mcamd_bs_price_f64 (q = 0.03), a time-only surface against Black-Scholes at the rms
     volatility, displaced diffusion against its exact delta;
  4. state: the same bits twice and from the enqueue form, the buckets against vega on the summed record, no gamma
     without a bump, two surfaces alive in one context, a foreign surface, the refusals that need a context, and an
     existing Greeks call and smile call before and after (the pinned record grew from 16 to 32 doubles).

tests/test_localvol_greeks_cpu.py asserts, without a kernel, that the restatement's two precisions differ by at most
half the tolerance on every input of test 1 and leave out at most 1 % of a case."""
import importlib
import math

import numpy as np
import pytest

import localvol_greeks_cases as cases
import localvol_greeks_restate as gr
import localvol_restate as lv
from deep_inputs import DEEP, SHALLOW, check_deep_draws_differ

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

BASE, Q_DIV, N_LOCAL, ETA = cases.BASE, cases.Q_DIV, cases.N_LOCAL, cases.ETA
SUM_RTOL = {capi.F64: 1e-11, capi.F32: 2e-5}
N_EST = gr.N_EST


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_deep_normals_are_those_of_neither_shallow_word(prec):
    """no kernel runs: the deep normals share nothing with the streams a dropped high word lands on"""
    check_deep_draws_differ(lambda seed, first: cases.normals(prec, seed, first, 64, 7))


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


FLAT = ((1, 2, -1.0, 1.0), np.array([[0.2, 0.2]]))


@pytest.fixture(scope="module")
def surfaces(ctx):
    made = {name: ctx.localvol_surface(grid, sigma) for name, (grid, sigma) in cases.SURFACES.items()}
    made["flat"] = ctx.localvol_surface(*FLAT)
    yield made
    for s in made.values():
        s.close()


def option(**kw):
    # v is ignored by the call: leave something in it that any use would show
    return capi.make_option(**dict(BASE, v=float("nan"), **kw))


def run(ctx, opt, sim, job, surface, want_samples=True):
    """(result, samples as a [6 + B, n_paths_local] float64 numpy array or None)"""
    rows, n = N_EST + job.n_vega_buckets, sim.n_paths_local
    s = torch.full((rows * max(n, 1),), float("nan"), dtype=torch.float64, device="cuda") if want_samples else None
    res = ctx.price_localvol_greeks(opt, sim, job, surface, s)
    torch.cuda.synchronize()
    return res, (s[:rows * n].cpu().numpy().reshape(rows, n) if want_samples else None)


def record_of(res):
    """(sums, sumsqs) of the 6 + 8 rows of a result"""
    return (np.array(list(res.sum) + list(res.bucket_sum)), np.array(list(res.sumsq) + list(res.bucket_sumsq)))


def check_sums(res, ref, prec):
    """the record against the sums of the samples `ref` ([rows, n]); every |sum| is bounded by sqrt(n sum q^2)"""
    sums, sumsqs = record_of(res)
    rows, n = ref.shape
    for e in range(rows):
        sq = float((ref[e] * ref[e]).sum())
        scale = math.sqrt(n * sq)
        assert abs(sums[e] - ref[e].sum()) <= SUM_RTOL[prec] * scale, (e, sums[e], ref[e].sum())
        assert abs(sumsqs[e] - sq) <= SUM_RTOL[prec] * sq, (e, sumsqs[e], sq)
    assert not sums[rows:].any() and not sumsqs[rows:].any()   # unused buckets are exact zeros


# ---- 1. samples against the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", cases.ALL_CASES, ids=cases.case_id)
def test_samples_against_the_restatement(ctx, surfaces, case):
    surface, n_steps, where, prec, payoff, eta, B = case
    seed, first, n_job = where
    own, other, keep, keep3 = cases.compare(case)
    want = cases.want_of(case)[:N_EST + B]
    tol = cases.tolerance(case, want)
    sim = capi.make_sim(n_job, n_steps, prec, seed=seed, path_offset=first, n_paths_local=N_LOCAL)
    res, got = run(ctx, option(), sim, capi.make_localvol_greeks_job(payoff, B, Q_DIV, eta), surfaces[surface])
    assert np.isfinite(got).all() and res.n == N_LOCAL and res.block == 256 and res.grid == N_LOCAL // 256
    excluded = 1.0 - (keep3 if eta > 0.0 else keep).mean()
    assert excluded <= cases.CAP, excluded
    report = []
    for e in cases.rows_of(eta, B):
        k = keep3 if e == gr.GAMMA else keep
        err = np.abs(got[e] - want[e])
        mean = np.abs(want[e]).mean()
        report.append(f"{err[k].max() / mean if mean else 0.0:.1e}")
        worst = int(np.argmax(np.where(k, err - tol[e], -np.inf)))
        assert (err[k] <= tol[e][k]).all(), (e, worst, got[e][worst], want[e][worst], tol[e][worst])
    if eta == 0.0:
        assert not got[gr.GAMMA].any()
    print(f"{cases.case_id(case)}: excluded {excluded:.4f}, worst kept deviation over mean |q| per row " + " ".join(report))
    assert 0.02 < (want[gr.PRICE] != 0).mean()
    # the same walk: row 0 is mcamd_price_localvol's sample, widened
    y = torch.full((N_LOCAL,), float("nan"), dtype=TORCH_T[prec], device="cuda")
    plain = ctx.price_localvol(option(), sim, capi.make_localvol(payoff, q=Q_DIV), surfaces[surface], y)
    torch.cuda.synchronize()
    assert np.array_equal(got[gr.PRICE], y.cpu().numpy().astype(np.float64))
    assert abs(res.sum[0] - plain.sum) <= 1e-12 * plain.sum and abs(res.sumsq[0] - plain.sumsq) <= 1e-12 * plain.sumsq
    # the record: the sums of d_samples, and what the finalize call makes of them
    check_sums(res, got, prec)
    fin = capi.finalize(res.sum[1], res.sumsq[1], res.n, BASE["r"], BASE["T"])
    assert (res.value[1], res.std_err[1]) == (fin.price, fin.std_err)
    if eta == 0.0:
        assert math.isnan(res.value[gr.GAMMA]) and math.isnan(res.std_err[gr.GAMMA])
        assert res.sum[gr.GAMMA] == res.sumsq[gr.GAMMA] == 0.0


# ---- 2. shards and the grid-stride trip ------------------------------------------------------------------------------------

SHARDS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513)


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_shards_against_the_sums_of_their_restated_paths(ctx, surfaces, prec):
    case = ("skew", 50, SHALLOW, prec, gr.CALL, ETA, 3)
    seed, first, n_job = SHALLOW
    own, other, keep, keep3 = cases.compare(case)
    want = cases.want_of(case)
    tol = cases.tolerance(case, want)
    job = capi.make_localvol_greeks_job(gr.CALL, 3, Q_DIV, ETA)
    for j, n in enumerate(SHARDS):
        lo = 37 * j   # 37 * 11 + 513 <= 1024
        sim = capi.make_sim(n_job, 50, prec, seed=seed, path_offset=first + lo, n_paths_local=n)
        res, got = run(ctx, option(), sim, job, surfaces["skew"])
        assert res.n == n and res.grid == -(-n // 256)
        sums, sumsqs = record_of(res)
        for e in range(N_EST + 3):
            k = (keep3 if e == gr.GAMMA else keep)[lo:lo + n]
            w, t = want[e][lo:lo + n], tol[e][lo:lo + n]
            assert (np.abs(got[e] - w)[k] <= t[k]).all(), (n, e)
            ref = np.where(k, w, got[e])   # a path beside the strike contributes whatever the kernel made of it
            slack = t[k].sum() + SUM_RTOL[prec] * np.abs(ref).sum()
            assert abs(sums[e] - ref.sum()) <= slack, (n, e, sums[e], ref.sum())
            assert abs(sumsqs[e] - (ref * ref).sum()) <= 2.0 * (np.abs(ref) * np.where(k, t, 0.0)).sum() + \
                (t[k] ** 2).sum() + SUM_RTOL[prec] * (ref * ref).sum(), (n, e)


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_a_second_grid_stride_trip_equals_its_two_shards(ctx, surfaces, prec):
    cut, n, n_steps = 8192 * 256, 8192 * 256 + 513, 3
    job = capi.make_localvol_greeks_job(gr.PUT, 8, Q_DIV, ETA)
    whole, _ = run(ctx, option(), capi.make_sim(n, n_steps, prec, seed=11), job, surfaces["skew"], False)
    a, _ = run(ctx, option(), capi.make_sim(n, n_steps, prec, seed=11, n_paths_local=cut), job, surfaces["skew"], False)
    b, tail = run(ctx, option(), capi.make_sim(n, n_steps, prec, seed=11, path_offset=cut, n_paths_local=513), job,
                  surfaces["skew"])
    assert (whole.grid, a.grid, b.grid) == (8192, 8192, 3) and whole.n == n == a.n + b.n
    (ws, wq), (as_, aq), (bs, bq) = record_of(whole), record_of(a), record_of(b)
    for e in range(N_EST + 8):
        scale = math.sqrt(n * wq[e])
        assert abs(ws[e] - (as_[e] + bs[e])) <= 1e-11 * scale and abs(wq[e] - (aq[e] + bq[e])) <= 1e-11 * wq[e], e
    assert wq[:N_EST].all()
    assert [bool(v) for v in wq[N_EST:]] == [k in (0, 2, 5) for k in range(8)]   # what 3 steps reach of 8 buckets
    check_sums(b, tail, prec)


# ---- 3. closed forms -------------------------------------------------------------------------------------------------------

def within_4_se(tag, value, se, want):
    print(f"{tag}: closed {want:.6f} got {value:.6f} SE {se:.6f} ({(value - want) / se:+.2f} SE)")
    assert se > 0 and abs(value - want) <= 4.0 * se, (tag, value, want, se)


def ncdf(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("n_steps", [1, 12, 50])
def test_flat_surface_against_the_closed_form_greeks(ctx, surfaces, prec, n_steps):
    S0, K, T, r, v = BASE["S0"], BASE["K"], BASE["T"], BASE["r"], 0.2
    sim = capi.make_sim(1 << 20, n_steps, prec, seed=3100 + n_steps)
    res, _ = run(ctx, option(), sim, capi.make_localvol_greeks_job(gr.CALL, 4, 0.0, ETA), surfaces["flat"], False)
    bs = capi.bs_greeks_f64(S0, K, T, r, v)
    tag = f"FLAT prec {prec} n_steps {n_steps}"
    for e, name in ((0, "price"), (1, "delta"), (3, "vega"), (4, "rho")):
        within_4_se(f"{tag} {name}", res.value[e], res.std_err[e], bs[e])
    S_up, S_dn = S0 * math.exp(ETA), S0 * math.exp(-ETA)
    gamma = (capi.bs_greeks_f64(S_up, K, T, r, v)[1] - capi.bs_greeks_f64(S_dn, K, T, r, v)[1]) / (S_up - S_dn)
    within_4_se(f"{tag} gamma", res.value[2], res.std_err[2], gamma)
    # a flat surface's buckets are vega's equal shares (statistically) and its exact parts (on the record)
    assert abs(sum(res.bucket_sum) - res.sum[3]) <= SUM_RTOL[prec] * math.sqrt(res.n * res.sumsq[3])
    print(f"{tag}: kernel {res.kernel_ms:.3f} ms")


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("payoff", [gr.CALL, gr.PUT])
def test_flat_surface_with_dividends_against_differences_of_the_closed_form(ctx, surfaces, prec, payoff):
    S0, K, T, r, v, q = BASE["S0"], BASE["K"], BASE["T"], BASE["r"], 0.2, Q_DIV
    res, _ = run(ctx, option(), capi.make_sim(1 << 20, 12, prec, seed=3200 + payoff),
                 capi.make_localvol_greeks_job(payoff, 0, q, ETA), surfaces["flat"], False)
    p = lambda S=S0, r_=r, q_=q, v_=v: capi.bs_price_f64(S, K, T, r_, q_, v_, payoff)
    delta = lambda S, h=1e-3: (p(S + h) - p(S - h)) / (2 * h)
    S_up, S_dn = S0 * math.exp(ETA), S0 * math.exp(-ETA)
    h = 1e-5
    want = {0: p(), 1: delta(S0), 2: (delta(S_up) - delta(S_dn)) / (S_up - S_dn), 3: (p(v_=v + h) - p(v_=v - h)) / (2 * h),
            4: (p(r_=r + h) - p(r_=r - h)) / (2 * h), 5: (p(q_=q + h) - p(q_=q - h)) / (2 * h)}
    for e, name in enumerate(gr.NAMES):
        within_4_se(f"FLAT q prec {prec} payoff {payoff} {name}", res.value[e], res.std_err[e], want[e])


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_time_only_surface_against_black_scholes_at_the_rms_volatility(ctx, prec):
    """as tests/test_localvol_greeks_cpu.py: vega = BSvega(vbar) mean(s) / vbar, bucket b its steps' share"""
    vols, n_steps, B = (0.15, 0.30, 0.20, 0.25), 12, 3
    S0, K, T, r, q = BASE["S0"], BASE["K"], BASE["T"], BASE["r"], Q_DIV
    with ctx.localvol_surface((4, 2, -1.0, 1.0), [[v, v] for v in vols]) as surface:
        res, _ = run(ctx, option(), capi.make_sim(1 << 20, n_steps, prec, seed=2031),
                     capi.make_localvol_greeks_job(gr.CALL, B, q, 0.0), surface, False)
    s = np.array([vols[lv.row_of(i, 4, n_steps)] for i in range(n_steps)])
    vbar = math.sqrt((s * s).mean())
    d1 = (math.log(S0 / K) + (r - q + 0.5 * vbar * vbar) * T) / (vbar * math.sqrt(T))
    bs_vega = S0 * math.exp(-q * T) * math.exp(-0.5 * d1 * d1) / math.sqrt(2 * math.pi) * math.sqrt(T)
    tag = f"TIME-ONLY prec {prec}"
    within_4_se(f"{tag} price", res.value[0], res.std_err[0], capi.bs_price_f64(S0, K, T, r, q, vbar))
    within_4_se(f"{tag} delta", res.value[1], res.std_err[1], math.exp(-q * T) * ncdf(d1))
    within_4_se(f"{tag} vega", res.value[3], res.std_err[3], bs_vega * s.mean() / vbar)
    for b in range(B):
        share = sum(s[i] for i in range(n_steps) if gr.bucket_of(i, B, n_steps) == b) / n_steps
        within_4_se(f"{tag} bucket {b}", res.bucket_value[b], res.bucket_std_err[b], bs_vega * share / vbar)


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_displaced_diffusion_delta_against_its_exact_value(ctx, prec):
    """r = q = 0, sigma(x) = sigma_d (1 + a / (S0 e^x)) on 65 nodes: delta = N(d1) at (S0 + a, K + a)"""
    S0, a, sigma_d = 100.0, 50.0, 0.2 * 100.0 / 150.0
    x = np.linspace(-1.5, 1.5, 65)
    sim = capi.make_sim(1 << 19, 64, prec, seed=909)
    S_up, S_dn = S0 * math.exp(ETA), S0 * math.exp(-ETA)
    with ctx.localvol_surface((1, 65, -1.5, 1.5), [sigma_d * (1.0 + a / (S0 * np.exp(x)))]) as surface:
        for K in (80.0, 100.0, 125.0):
            opt = capi.make_option(S0=S0, K=K, r=0.0, T=1.0, v=0.0)
            res, _ = run(ctx, opt, sim, capi.make_localvol_greeks_job(gr.CALL, 0, 0.0, ETA), surface, False)
            delta = lambda S: ncdf((math.log((S + a) / (K + a)) + 0.5 * sigma_d ** 2) / sigma_d)
            within_4_se(f"DISPLACED prec {prec} K {K} delta", res.value[1], res.std_err[1], delta(S0))
            within_4_se(f"DISPLACED prec {prec} K {K} gamma", res.value[2], res.std_err[2],
                        (delta(S_up) - delta(S_dn)) / (S_up - S_dn))


# ---- 4. state and ordering -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
@pytest.mark.parametrize("n", [3000, 8192 * 256 + 700])   # one wave of workgroups; beyond the 8192-workgroup cap
def test_same_bits_twice_and_from_the_enqueue_form(ctx, surfaces, prec, n):
    n_steps, B = 13, 5
    opt, job = option(), capi.make_localvol_greeks_job(gr.PUT, B, Q_DIV, ETA)
    sim = capi.make_sim(n + 9, n_steps, prec, seed=4, path_offset=9, n_paths_local=n)
    want_samples = n < 10_000
    a, y_a = run(ctx, opt, sim, job, surfaces["skew"], want_samples)
    b, y_b = run(ctx, opt, sim, job, surfaces["skew"], want_samples)
    (sa, qa), (sb, qb) = record_of(a), record_of(b)
    assert np.array_equal(sa, sb) and np.array_equal(qa, qb) and qa[:N_EST + B].all() and not qa[N_EST + B:].any()
    assert list(a.value) == list(b.value) and list(a.bucket_std_err) == list(b.bucket_std_err)
    assert a.grid == min(-(-n // 256), 8192) and a.block == 256 and a.n == n
    if want_samples:
        assert np.array_equal(y_a, y_b)
    stats = torch.full((32,), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.full(((N_EST + B) * n,), float("nan"), dtype=torch.float64, device="cuda") if want_samples else None
    ctx.price_localvol_greeks_enqueue(opt, sim, job, surfaces["skew"], stats, s)
    ms = ctx.enqueued_kernel_ms(1)
    torch.cuda.synchronize()
    rec = stats.cpu().numpy()
    assert np.array_equal(rec[0:28:2], sa) and np.array_equal(rec[1:28:2], qa)
    assert rec[28:].tolist() == [float(n), 0.0, 0.0, 0.0]
    if want_samples:
        assert np.array_equal(s.cpu().numpy().reshape(N_EST + B, n), y_a)
    fin = capi.finalize_localvol_greeks_stats(rec, BASE["r"], BASE["T"], B, True)
    assert list(fin.value) == list(a.value) and list(fin.std_err) == list(a.std_err) and fin.n == n
    assert list(fin.bucket_value) == list(a.bucket_value) and list(fin.bucket_std_err) == list(a.bucket_std_err)
    assert 0.0 < ms[0] < 1e4
    # the buckets add up to vega on the summed record, to the rounding of the path precision (U and the U^b are rounded
    # apart at every step: a few ulp of the path precision each, far below the sums' tolerance)
    assert abs(sa[N_EST:].sum() - sa[gr.VEGA]) <= SUM_RTOL[prec] * math.sqrt(n * qa[gr.VEGA])
    # no bump, no gamma: NaN, zero sums; the other estimators are the same samples
    c, y_c = run(ctx, opt, sim, capi.make_localvol_greeks_job(gr.PUT, B, Q_DIV, 0.0), surfaces["skew"], want_samples)
    assert math.isnan(c.value[2]) and math.isnan(c.std_err[2]) and c.sum[2] == c.sumsq[2] == 0.0
    assert [c.sum[e] for e in (0, 1, 3, 4, 5)] == [a.sum[e] for e in (0, 1, 3, 4, 5)] and list(c.bucket_sum) == list(a.bucket_sum)
    if want_samples:
        assert not y_c[2].any() and np.array_equal(np.delete(y_c, 2, axis=0), np.delete(y_a, 2, axis=0))
    # an empty shard: zeros, still ordered on the stream
    empty = capi.make_sim(n, n_steps, prec, seed=4, path_offset=5, n_paths_local=0)
    ctx.price_localvol_greeks_enqueue(opt, empty, job, surfaces["skew"], stats)
    torch.cuda.synchronize()
    assert not stats.cpu().numpy().any()
    res, _ = run(ctx, opt, empty, job, surfaces["skew"], False)
    assert res.n == 0 and res.grid == 0 and not any(list(res.value) + list(res.sum) + list(res.bucket_sum))


@pytest.mark.parametrize("prec", [capi.F64, capi.F32])
def test_two_surfaces_alive_in_one_context(ctx, surfaces, prec):
    """priced alternately, enqueued back to back without a wait between them: each call sees its own table"""
    n, B = 5000, 2
    sim = capi.make_sim(n, 13, prec, seed=21)
    opt, job = option(), capi.make_localvol_greeks_job(gr.CALL, B, Q_DIV, ETA)
    names = ("skew", "two", "full", "narrow")
    alone = {name: run(ctx, opt, sim, job, surfaces[name])[1] for name in names}
    assert all(not np.array_equal(alone[a], alone[b]) for a in names for b in names if a < b)
    stats = [torch.zeros(32, dtype=torch.float64, device="cuda") for _ in range(8)]
    outs = [torch.full(((N_EST + B) * n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(8)]
    for i in range(8):
        ctx.price_localvol_greeks_enqueue(opt, sim, job, surfaces[names[i % 4]], stats[i], outs[i])
    torch.cuda.synchronize()
    for i in range(8):
        assert np.array_equal(outs[i].cpu().numpy().reshape(N_EST + B, n), alone[names[i % 4]])
        assert stats[i][28].item() == n


def test_existing_calls_before_and_after_see_the_widened_record_unchanged(ctx, surfaces):
    """the pinned final record grew from 16 to 32 doubles: a Greeks call and a smile call give their usual results
    before and after a local-volatility Greeks call"""
    opt_g, sim_g = capi.make_option(), capi.make_sim(100_000, 12, capi.F64, seed=8)
    smile = capi.make_smile(2, 3, capi.PAYOFF_CALL, Q_DIV)
    sim_s = capi.make_sim(50_000, 12, capi.F64, seed=9)

    def old_calls():
        g = ctx.price_greeks(opt_g, sim_g)
        price, se, stats, _ = ctx.price_localvol_smile(option(), sim_s, smile, (6, 12), (90.0, 100.0, 110.0), surfaces["skew"])
        return list(g.value[:5]) + list(g.sum) + list(g.sumsq) + [g.n], np.array(price), np.array(stats)

    before = old_calls()
    res, _ = run(ctx, option(), capi.make_sim(100_000, 12, capi.F64, seed=8),
                 capi.make_localvol_greeks_job(gr.CALL, 8, Q_DIV, ETA), surfaces["skew"], False)
    after = old_calls()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    bs = capi.bs_greeks_f64(100.0, 100.0, 1.0, 0.1, 0.2)
    g = ctx.price_greeks(opt_g, sim_g)
    assert abs(g.value[1] - bs[1]) <= 4.0 * g.std_err[1] and res.n == 100_000 and all(res.bucket_sumsq)


def test_refusals_with_a_live_context(ctx, surfaces):
    opt, job, sim = option(), capi.make_localvol_greeks_job(), capi.make_sim(1000, 12)
    ok, _ = run(ctx, opt, sim, job, surfaces["skew"], False)
    same, _ = run(ctx, opt, capi.make_sim(1000, 12, flags=capi.FLAG_LOG_SPACE), job, surfaces["skew"], False)
    assert list(ok.sum) == list(same.sum) and ok.sum[0] > 0
    stats = torch.zeros(32, dtype=torch.float64, device="cuda")
    bad = [(opt, capi.make_sim(1000, 12, flags=flags), job, "flags")
           for flags in (capi.FLAG_ANTITHETIC, capi.FLAG_PRODUCT_FORM, capi.FLAG_CONTROL_VARIATE, capi.FLAG_SEPARATE_REDUCE)]
    bad += [(opt, sim, capi.make_localvol_greeks_job(n_vega_buckets=9), "n_vega_buckets"),
            (opt, sim, capi.make_localvol_greeks_job(gamma_bump=0.2), "gamma_bump"),
            (opt, sim, capi.make_localvol_greeks_job(payoff=2), "payoff")]
    for o, s, j, words in bad:
        with pytest.raises(capi.McamdError) as e:
            ctx.price_localvol_greeks(o, s, j, surfaces["skew"])
        assert e.value.code == capi.ERR_INVALID and words in str(e.value)
        with pytest.raises(capi.McamdError):
            ctx.price_localvol_greeks_enqueue(o, s, j, surfaces["skew"], stats)
    # a surface serves the context it was created on and no other
    other = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        with other.localvol_surface(*cases.SURFACES["skew"]) as foreign:
            for call in (lambda: ctx.price_localvol_greeks(opt, sim, job, foreign),
                         lambda: ctx.price_localvol_greeks_enqueue(opt, sim, job, foreign, stats)):
                with pytest.raises(capi.McamdError) as e:
                    call()
                assert e.value.code == capi.ERR_INVALID and "another context" in str(e.value)
            mine = other.price_localvol_greeks(opt, sim, job, foreign)
            assert list(mine.sum) == list(ok.sum) and list(mine.sumsq) == list(ok.sumsq)
    finally:
        other.close()
    # the fp64 exponent-range bound is taken at the surface's largest entry, with the bump added
    with ctx.localvol_surface((1, 2, -1.0, 1.0), [[0.2, 100.0]]) as wild:
        with pytest.raises(capi.McamdError) as e:
            ctx.price_localvol_greeks(capi.make_option(**dict(BASE, T=100.0, v=0.0)), capi.make_sim(1000, 50), job, wild)
        assert e.value.code == capi.ERR_INVALID and "exponent range" in str(e.value)
    # a missing record is refused before anything is enqueued
    with pytest.raises(capi.McamdError) as e:
        ctx.price_localvol_greeks_enqueue(opt, sim, job, surfaces["skew"], None)
    assert e.value.code == capi.ERR_INVALID and "d_stats" in str(e.value)
