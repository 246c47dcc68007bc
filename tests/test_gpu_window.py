"""GPU tests of the window paths one by one: mcamd_price_paths with a bullet window, with and without the antithetic
twin, the control variate and the product form (csrc/mc_device.hpp simulate_sample, csrc/price_impl.hpp price_kernel),
and the nested-MC inner stage by its four routes (csrc/nmc.hip, csrc/nmc_compact.hpp).  Run with -m gpu on an MI355X.

Every sample and every point is compared with the numpy restatement of tests/window_restate.py on the inputs of
tests/window_cases.py, whose docstring states the cases, the margin, the tolerance rule and the caps;
tests/test_window_cpu.py pins the restatement to the oracle and shows that each restated mistake lies beyond the
tolerances used here.  A flipped barrier comparison is isolated, not averaged over: a path with a step within MARGIN of
the barrier is *undecided* only if a flip there moves its count across P1 or P2, and then has to equal one of its
candidate payoffs; every other sample is held to fp32 (fp64) rounding.

  1. test_every_path_of_price_paths: the 256 single-path records (n_paths_local = 1) of every case x form x precision;
  2. test_shard_is_the_sum_of_its_paths: the shard of all 256 paths against the fp64 sum of those records, all five
     sums, 1e-13 — a path priced alone leaves the loop when its own window closes, inside a full wavefront it runs on;
  3. test_nested_mc_points: every point of every case by the wave, block, plain-block and fused routes, from the rows
     simulate_trajectories stored, inside [lo - tol, hi + tol]; closed points exactly 0; the fused rows and points
     bit-identical to the two-launch route; res.sum the sum of the points; compaction shown by work_steps;
  4. the window-less nested-MC case is the `windowless` case of test 3: every point at its tolerance, no intervals.

From the restatements (tests/test_window_cpu.py prints them; none is fitted to a kernel): |ln S_t| between the two
restatements at most 4.6e-16 (fp64) and 2.3e-7 (fp32) against MARGIN = 2e-5; sample spreads at most 6.4e-14 / 3.8e-5, so
a sample's tolerance is 1.6e-11 .. 1.1e-8 (fp64) and 2.3e-5 .. 2.4e-3 (fp32: 4 spreads at the low end, the floor 2e-5 of
the payoff at the high end); at most 1 of a case's 256 samples undecided, at least 19 non-zero; nested-MC points
without an undecided inner path 96 % .. 100 % of the priced ones, point tolerance 1.2e-9 .. 5.4e-9 (fp64) and 1.9e-4 ..
6.4e-4 (fp32) where tests/test_gpu_parity.py allows rtol 5e-3 + atol 2e-3.

Which restated mistakes the older tolerances of tests/test_gpu_parity.py would have let through (CPU figures, printed by
tests/test_window_cpu.py).  On the sum of a case's 256 samples: the last block one step long at 33 steps moves an fp32
sum by 1.2e-3 (plain) and 3.2e-3 (antithetic), one step short at 61 steps by 3.1e-3 — inside or at the edge of the 2e-3
to 3e-3 allowed there, while 56 and 36 single samples lie beyond the tolerance used here.  Every other restated mistake
moves a case's sum by 6e-3 or more, so a sum-level test would have seen it on these shapes; the older tests did not run
them: their windowed price_paths jobs have 100 steps, a multiple of both block sizes, so no windowed job took a partial
last block, none ran shorter than one block, and no windowed variance-reduction job ran in the product form.  On
nested-MC points (rtol 5e-3 + atol 2e-3 in fp32): a whole step too few or too many is flagged on 49 and 48 of the 49
affected paying points of the edges case and on 69 and 66 of 73 of the compaction case, where the tolerance here flags
all of them; the older test looks at 30 points of one 61-step case.

Measured on the MI355X (printed by the tests), largest share of the tolerance used over all cases:
  price_paths sample   fp32: log form 0.23 (plain, cv), 0.20 - 0.22 (antithetic); product form 0.42 and 0.38;
                       window-less antithetic 0.058 / 0.065; fp64: at most 4.3e-4 in every form
  control              fp32 at most 0.017 (log) and 0.060 (product); fp64 at most 2.2e-5
  shard of 256         at most 2.4e-16: of the sum for sum, sumsq and sum_cc, of the summed magnitudes for sum_c, sum_yc
  nested-MC point      fp32: edges 0.015, compaction 0.019, deep 0.012, windowless 0.010; fp64 at most 1.5e-5;
                       the four routes agree to the printed digits, fused and wave bit for bit
  undecided            fp64 normals: one sample in each of w-7-deep (antithetic), w-6-straddle and w-33-straddle
                       (antithetic); fp32 normals: one in w-61-deep (antithetic forms); each equals a restated candidate,
                       using at most 8.2e-5 (fp64) and 0.23 (fp32) of the tolerance; on the GPU's rows the edges case
                       prices 1 (fp64) and 3 (fp32) points through an interval, compaction 2 (fp32)
  last-step point      at most 1.7 (fp64 log form), 0.83 (fp64 product), 0.56 and 0.11 (fp32) ulp of the stored price,
                       where LAST_STEP_ULPS allows 8; its zeros are exact
No kernel needed a change."""
import importlib
import math

import numpy as np
import pytest

import window_cases as wc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

TORCH_T = {capi.F64: torch.float64, capi.F32: torch.float32}
SUMS = ("sum", "sumsq", "sum_c", "sum_cc", "sum_yc")
# A point with no step to go never steps, but the log form (and every fp64 form, for its barrier test) still sends the
# stored price through log_ratio and back (csrc/nmc.hip price_group, mc_device.hpp exp_of_logreturn): a division (0.5
# ulp), a logarithm (2 ulp of |ln(St / S_start)| < 0.5: 1 ulp of the price), its scaling (0.5), the exponential (4.5 ulp,
# the bound of tests/fast64_bounds.py; 1 ulp for v_exp_f32) and a multiply (0.5): under 8 ulp of the stored PRICE — not
# of the payoff, which near the strike is a small difference of it.  St - K, the sum of n_inner equal terms and the
# compare are exact; the scaling and the rounding to the output type add 2 ulp of the point.
LAST_STEP_ULPS = 8


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


_records = {}


def records(ctx, prec, case, form):
    """[N_PATHS, 6] the single-path records of the case's paths under the form; computed once"""
    key = (prec, case.name, form)
    if key not in _records:
        stats = torch.zeros(wc.N_PATHS, 6, dtype=torch.float64, device="cuda")
        opt, first = wc.option(case), case.where[1]
        for i in range(wc.N_PATHS):
            ctx.price_paths_enqueue(opt, wc.sim(case, prec, wc.FORMS[form], first + i, 1), stats[i])
        rec = stats.cpu().numpy()
        rec.setflags(write=False)
        _records[key] = rec
    return _records[key]


PP_IDS = [f"{c.name}-{f}" for c, f in wc.PP_CASES]


@pytest.mark.parametrize("prec", wc.PRECS)
@pytest.mark.parametrize("case,form", wc.PP_CASES, ids=PP_IDS)
def test_every_path_of_price_paths(ctx, prec, case, form):
    rec = records(ctx, prec, case, form)
    w = wc.wanted(case, prec, form)
    assert np.isfinite(rec).all() and (rec[:, 5] == 1).all()
    y = rec[:, 0]
    ref = wc.nearest_candidate(y, w)
    used = np.abs(y - ref) / w.tol_y
    print(f"f{prec} {case.name} {form}: {np.count_nonzero(y)} of {len(y)} samples pay, {np.count_nonzero(~w.want.decided)} "
          f"undecided, largest share of the tolerance {used.max():.2e}" +
          ("" if w.tol_c is None else f", of the control's {(np.abs(rec[:, 2] - w.want.c) / w.tol_c).max():.2e}"))
    assert not wc.outside(y, w).any(), np.argwhere(wc.outside(y, w))[:8]
    assert (ref[w.want.decided] == w.want.y[w.want.decided]).all()
    assert np.allclose(rec[:, 1], y * y, rtol=1e-15, atol=0.0)
    if w.tol_c is None:
        assert (rec[:, 2:5] == 0).all()
        return
    c, want_c = rec[:, 2], w.want.c
    assert (np.abs(c - want_c) <= w.tol_c).all(), np.argwhere(np.abs(c - want_c) > w.tol_c)[:8]
    assert (np.abs(rec[:, 3] - want_c ** 2) <= 2 * np.abs(want_c) * w.tol_c + w.tol_c ** 2).all()
    assert (np.abs(rec[:, 4] - ref * want_c) <= np.abs(ref) * w.tol_c + np.abs(want_c) * w.tol_y + w.tol_y * w.tol_c).all()
    # and the record is consistent with itself: c^2 and y c of its own y and c
    assert np.allclose(rec[:, 3], c * c, rtol=1e-15, atol=0.0)
    assert np.allclose(rec[:, 4], y * c, rtol=1e-15, atol=1e-300)


@pytest.mark.parametrize("prec", wc.PRECS)
@pytest.mark.parametrize("case,form", wc.PP_CASES, ids=PP_IDS)
def test_shard_is_the_sum_of_its_paths(ctx, prec, case, form):
    rec = records(ctx, prec, case, form)
    res = ctx.price_paths(wc.option(case), wc.sim(case, prec, wc.FORMS[form]))
    assert res.n == wc.N_PATHS
    got = [getattr(res, k) for k in SUMS]
    want = [math.fsum(rec[:, k]) for k in range(5)]
    # sum, sumsq and sum_cc have terms of one sign: 1e-13 of the sum.  The centred sums sum_c and sum_yc cancel (sum c =
    # -0.7 of terms that add up to 520 in one case) and round on the scale of their terms, where (n - 1) eps = 2.8e-14
    # bounds every order of summation: 1e-13 of the summed magnitudes
    scale = [math.fsum(np.abs(rec[:, k])) if SUMS[k] in ("sum_c", "sum_yc") else abs(want[k]) for k in range(5)]
    print(f"f{prec} {case.name} {form}: deviation of the five sums relative to 1e-13 of their scale "
          f"{[abs(g - x) / (1e-13 * s) if s else abs(g) for g, x, s in zip(got, want, scale)]}")
    for k, g, x, s in zip(SUMS, got, want, scale):
        assert abs(g - x) <= 1e-13 * s, (k, g, x)


# ---------------- nested MC ----------------
NMC_PARAMS = [(c, layout) for c in wc.NMC_CASES for layout in c.layouts]
NMC_IDS = [f"{c.name}-{'step' if layout == capi.STEP_MAJOR else 'path'}-major" for c, layout in NMC_PARAMS]
_rows, _wanted = {}, {}


def by_point(a, case, layout):
    """[n_local, n_steps] view of a buffer in the layout"""
    a = a.cpu().numpy()
    return a.reshape(case.n_steps, case.n_local).T if layout == capi.STEP_MAJOR else a.reshape(case.n_local, case.n_steps)


def stored_rows(ctx, case, layout, prec):
    """the device buffers (prices, counts) simulate_trajectories stored for the case's outer paths; computed once"""
    key = (case.name, layout, prec)
    if key not in _rows:
        n = case.n_local * case.n_steps
        traj, cnt = torch.zeros(n, dtype=TORCH_T[prec], device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        res = ctx.simulate_trajectories(wc.nmc_option(case), wc.nmc_outer_sim(case, prec), traj, cnt, None, layout)
        assert res.n == case.n_local
        _rows[key] = (traj, cnt)
    return _rows[key]


def nmc_wanted(oracle, case, layout, prec, St, cnt):
    """wc.nmc_wanted from the GPU's own rows; the same for every route, form and layout of (case, precision)"""
    key = (case.name, prec)
    if key not in _wanted:
        _wanted[key] = (St.copy(), cnt.copy(), wc.nmc_wanted(oracle, case, prec, St, cnt))
    St0, cnt0, w = _wanted[key]
    assert np.array_equal(St0, St) and np.array_equal(cnt0, cnt), "the stored rows depend on the layout"
    return w


@pytest.mark.parametrize("prec", wc.PRECS)
@pytest.mark.parametrize("flags", [0, capi.FLAG_PRODUCT_FORM], ids=["log", "product"])
@pytest.mark.parametrize("case,layout", NMC_PARAMS, ids=NMC_IDS)
def test_nested_mc_points(ctx, oracle, prec, flags, case, layout):
    opt, inner = wc.nmc_option(case), wc.nmc_inner_sim(case, prec, flags)
    traj, cnt = stored_rows(ctx, case, layout, prec)
    St, Cn = by_point(traj, case, layout), by_point(cnt, case, layout)
    assert np.isfinite(St).all() and (St > 0).all()
    w = nmc_wanted(oracle, case, layout, prec, St, Cn)
    want, live = w.want, ~w.want.closed
    if opt.use_window:
        assert (np.diff(Cn, axis=1) >= 0).all() and want.closed.any() and live.sum() >= case.n_steps
        assert w.free.sum() >= wc.MIN_FREE * live.sum()
    else:
        assert live.all() and w.free.all() and (want.lo == want.hi).all()
    n = case.n_local * case.n_steps
    outs, results = {}, {}
    for route, variant in wc.NMC_ROUTES.items():
        out = torch.full((n,), -1.0, dtype=TORCH_T[prec], device="cuda")
        if variant is None:
            t2, c2 = torch.zeros_like(traj), torch.zeros_like(cnt)
            res = ctx.nmc_fused(opt, inner, wc.OUTER_SEED[case.seed], t2, c2, out, layout)
            assert torch.equal(t2, traj), "the fused kernel's rows are not simulate_trajectories'"
            assert torch.equal(c2, cnt) or not opt.use_window
        else:
            res = ctx.nmc_inner(opt, inner, traj, cnt, out, layout, variant)
        outs[route], results[route] = out, res
        got = by_point(out, case, layout).astype(np.float64)
        bad = wc.nmc_outside(got, w)
        used = (np.abs(got - want.price) / np.where(w.tol > 0, w.tol, 1.0))[w.free]
        # the last step's points, in ulp of the stored price (discounted): see LAST_STEP_ULPS
        unit = np.spacing(St[:, -1]).astype(np.float64) * math.exp(-opt.r * opt.T)
        last = np.abs(got[:, -1] - want.price[:, -1]) / unit
        print(f"f{prec} {case.name} {route} flags {flags}: {live.sum()} of {live.size} points priced, "
              f"{w.free.sum() / live.sum():.3f} of them held to a zero-width interval, largest share of the tolerance "
              f"{used.max():.2e}; last step's points off by at most {last.max():.2f} ulp of the stored price")
        assert res.n == n
        assert not bad.any(), (route, np.argwhere(bad)[:8], got[bad][:8], want.lo[bad][:8], want.hi[bad][:8], w.tol[bad][:8])
        assert (got[want.closed] == 0).all(), route                  # a closed point is exactly 0
        # the last step's points: no step to go, the discounted window payoff of the stored price and nothing else
        assert (w.free | want.closed)[:, -1].all() and ((got[:, -1] == 0) == (want.price[:, -1] == 0)).all(), route
        ulp_out = np.spacing(want.price[:, -1].astype(wc.OWN[prec])).astype(np.float64)
        assert (np.abs(got[:, -1] - want.price[:, -1]) <= LAST_STEP_ULPS * unit + 2 * ulp_out).all(), (route, last.max())
        # res.sum adds the double prices BEFORE they are rounded to the output type (csrc/nmc.hip price_group: rec[0] +=
        # price, then out = static_cast<T>(price)), so against the sum of the fp32 outputs it is off by up to half an ulp
        # of each output: that much slack in fp32, none in fp64.  This is a new check; no existing bound is involved.
        total = math.fsum(got.ravel())
        slack = 0.0 if prec == capi.F64 else 0.5 * float(np.spacing(got.astype(np.float32)).astype(np.float64).sum())
        assert abs(res.sum - total) <= 1e-12 * abs(total) + slack, (route, res.sum, total)
    assert torch.equal(outs["fused"], outs["wave"])
    if case.name == "compaction":
        # the pool of up to 1040 paths did hand over and resume: fewer wave-steps than the kernel that does not compact
        assert 0 < results["wave"].work_steps < results["block-plain"].work_steps
        assert 0 < results["wave"].live_steps <= results["wave"].work_steps
