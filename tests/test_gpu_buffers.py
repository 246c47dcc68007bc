"""GPU tests of the kernels that read or write caller-owned buffers, at every alignment, tail and guard band: the
array-driven pricer with and without a window (csrc/aux.hip from_normals_kernel), the bulk normal fill
(normals_kernel), the trajectory store (csrc/store.hip store_kernel, both offset widths), the store pattern
(store_pattern_kernel) and the four reductions (reduce_kernel).  Run with -m gpu on an MI355X.

Every buffer is a slice of a larger poisoned tensor (tests/buffer_cases.py placed()): its address mod 128 is chosen, and
the bytes on both sides are compared bit for bit after the call.  tests/buffer_cases.py states the cases, the
restatements and the tolerance rule; tests/test_buffer_cpu.py pins them on the CPU and shows that a row read one vector
late, a row's last vector dropped and a count that takes the neighbouring row's vectors lie beyond the tolerances.

  1. test_array_driven_pricer_at_every_placement: 130 paths (and 1 and 64) x the step counts whose rows sit at, under,
     on and over the 128-byte line x {no window, window} x the normals at every multiple of 16 and at element skews
     (scalar path): payoffs against window_restate.samples, res.sum / res.sumsq against the returned payoffs (1e-13),
     every placement bit-identical to skew 0 (the VEC and the scalar path too), NaN guards never consumed, the payoff
     buffer's guards untouched; the restart cases pin the row length n_steps - Tk;
  2. test_bulk_normals_at_every_placement: sizes around the Philox block and the workgroup, vector and scalar stores;
  3. test_store_at_every_placement / test_store_with_wide_offsets: every ragged tail x step remainder x layout x
     {aligned, each buffer off, all off, counts or payoffs absent}, bit-identical to the aligned run; one shape per
     precision and layout against window_restate.price_paths; n_local = 2^29 and 2^29 + 1 take the 64-bit row offsets;
  4. test_store_pattern: the counter pattern, its guards and its three refusals;
  5. test_reduce_at_every_placement: the four variants at every element skew with NaN on both sides of the input.

Measured on the MI355X (printed by the tests), largest share of the tolerance used:
  array-driven payoff   fp32 0.71 without a window (the 64-step restart) and 0.65 with one (252 steps); fp64 2.0e-4 and
                        8.4e-4; the one undecided sample (fp32, 28 steps, window) equals its restated candidate, 0.23
  placements            the payoffs, res.sum and res.sumsq of all 12 (fp32) / 11 (fp64) placements of the normals are
                        those of skew 0 bit for bit in every case, VEC against scalar included: a dead vector does
                        leave the price where it is; d_payoffs = NULL gives the same sums
  stored price          fp32 0.021, fp64 8.3e-6; payoff 0.20 and 3.9e-5; the one fp32 comparison within MARGIN of the
                        barrier came out as restated; every placement bit-identical to the aligned run
  wide store            2^29 and 2^29 + 1 paths x 2 steps: 0.02 .. 0.1 s and 1.1 .. 1.4 s (the ragged one stores
                        element by element); first and last 64 columns are the small shards' bit for bit
  reductions            at most 1.8e-16 of the sum (fp64 input), exact for fp32 input, where 1e-12 is allowed
No guard band was touched and no kernel needed a change; include/mcamd.h now states the row length of d_normals as
n_steps - Tk, which the restart cases pin."""
import importlib
import math

import numpy as np
import pytest

import buffer_cases as bc
import window_cases as wc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

TORCH_T = {capi.F64: torch.float64, capi.F32: torch.float32}
NAN = float("nan")
LAYOUTS = {"step-major": capi.STEP_MAJOR, "path-major": capi.PATH_MAJOR}


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


def same_bits(a, b):
    """two host arrays or two device tensors hold the same bytes"""
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bc._as_int(a), bc._as_int(b))


def close_to(got, want, rel):
    return abs(got - want) <= rel * abs(want)


def check_payoffs(got, w, label):
    """the payoffs `got` against the PPWanted w by the candidate rule; returns the largest share of the tolerance used"""
    got = got.astype(np.float64)
    bad = wc.outside(got, w)
    assert not bad.any(), (label, np.argwhere(bad)[:8].ravel(), got[bad][:8], w.want.y[bad][:8], w.tol_y[bad][:8])
    ref = wc.nearest_candidate(got, w)
    assert (ref[w.want.decided] == w.want.y[w.want.decided]).all(), label
    return float((np.abs(got - ref) / w.tol_y).max())


# ---------------- 1. array-driven pricer ----------------
FN_PARAMS = [(prec, case) for prec in wc.PRECS for case in bc.fn_cases(prec)]


@pytest.mark.parametrize("use_window", [0, 1], ids=["no-window", "window"])
@pytest.mark.parametrize("prec,case", FN_PARAMS, ids=[f"f{p}-{c.name}" for p, c in FN_PARAMS])
def test_array_driven_pricer_at_every_placement(ctx, prec, case, use_window):
    opt, item, T, n_sim = bc.fn_option(case, use_window), bc.ITEM[prec], TORCH_T[prec], bc.n_sim(case)
    z_all, w_all = bc.fn_normals(case, prec), bc.fn_wanted(case, prec, use_window)
    for n in bc.job_sizes(case):
        w, sim = bc.first(w_all, n), bc.fn_sim(case, prec, n)
        z = torch.from_numpy(z_all[:n].ravel().copy())
        base = None
        for skew in bc.SKEWS_16 + bc.SKEWS_ELEMENT[prec]:
            _, zv = bc.placed(n * n_sim, T, skew, NAN)
            zv.copy_(z)
            pw, pv = bc.placed(n, T, item, NAN)       # the payoffs one element off a line: never 16-byte aligned
            before = bc.guards(pw, pv)
            res = ctx.price_from_normals(opt, sim, zv, pv)
            assert bc.untouched(pw, pv, before), (n, skew)
            got = pv.cpu().numpy()
            assert np.isfinite(got).all(), (n, skew)          # no NaN of the guards around the normals was consumed
            assert res.n == n
            assert close_to(res.sum, math.fsum(got), 1e-13) and close_to(res.sumsq, math.fsum(got.astype(np.float64) ** 2), 1e-13)
            if base is None:
                base, base_res = got, res
                used = check_payoffs(got, w, (n, skew))
                print(f"f{prec} {case.name} window {use_window}, {n} paths: {np.count_nonzero(got)} pay, "
                      f"{np.count_nonzero(~w.want.decided)} undecided, largest share of the tolerance {used:.2e}")
            else:
                differ = np.flatnonzero(got != base)
                assert same_bits(got, base), (n, skew, bc.on_vec_path(case, prec, skew), differ[:8], got[differ][:8], base[differ][:8])
                assert (res.sum, res.sumsq) == (base_res.sum, base_res.sumsq)
            if skew in (0, bc.SKEWS_ELEMENT[prec][0]):
                none = ctx.price_from_normals(opt, sim, zv, None)
                assert (none.sum, none.sumsq, none.n) == (res.sum, res.sumsq, n), skew


# ---------------- 2. bulk normals ----------------
BULK_PARAMS = [(prec, n) for prec in wc.PRECS for n in bc.BULK_SIZES[prec]]


@pytest.mark.parametrize("prec,n", BULK_PARAMS, ids=[f"f{p}-{n}" for p, n in BULK_PARAMS])
def test_bulk_normals_at_every_placement(ctx, oracle, prec, n):
    want = oracle.generate_normals(bc.BULK_SEED, n, prec)
    base = None
    for skew in bc.BULK_SKEWS[prec]:
        whole, view = bc.placed(n, TORCH_T[prec], skew, NAN)
        before = bc.guards(whole, view)
        ctx.generate_normals(bc.BULK_SEED, n, prec, view)
        assert bc.untouched(whole, view, before), skew
        got = view.cpu().numpy()
        if prec == capi.F64:     # the tolerances of test_gpu_parity.py test_bulk_normals_vs_oracle
            assert np.allclose(got, want, rtol=1e-13, atol=1e-15), skew
        else:
            assert np.allclose(got, want, rtol=0, atol=4e-6), skew
        base = got if base is None else base
        assert same_bits(got, base), skew


# ---------------- 3. trajectory store ----------------
def run_store(ctx, opt, sim, layout, skews):
    """simulate_trajectories into three placed buffers (skews in elements; None: not passed); the guards are checked here"""
    T, n = TORCH_T[sim.precision], sim.n_paths_local
    cells = n * (sim.n_steps - opt.Tk)
    specs = ((cells, T, NAN), (cells, torch.int32, bc.COUNT_POISON), (n, T, NAN))
    bufs = [(None, None) if s is None else bc.placed(m, t, s * torch.empty(0, dtype=t).element_size(), poison)
            for s, (m, t, poison) in zip(skews, specs)]
    before = [None if v is None else bc.guards(wh, v) for wh, v in bufs]
    res = ctx.simulate_trajectories(opt, sim, bufs[0][1], bufs[1][1], bufs[2][1], layout)
    for (wh, v), b, name in zip(bufs, before, ("traj", "counts", "payoffs")):
        assert v is None or bc.untouched(wh, v, b), (name, skews)
    return res, [v for _, v in bufs]


def by_path(a, n_local, n_steps, layout):
    a = a.cpu().numpy()
    return a.reshape(n_steps, n_local).T if layout == capi.STEP_MAJOR else a.reshape(n_local, n_steps)


STORE_PARAMS = [(prec, n) for prec in wc.PRECS for n in bc.store_sizes(prec)]


@pytest.mark.parametrize("layout", list(LAYOUTS), ids=list(LAYOUTS))
@pytest.mark.parametrize("prec,n_local", STORE_PARAMS, ids=[f"f{p}-{n}" for p, n in STORE_PARAMS])
def test_store_at_every_placement(ctx, prec, n_local, layout):
    opt = bc.store_option()
    for n_steps in bc.STORE_STEPS:
        sim = bc.store_sim(prec, n_local, n_steps)
        base = None
        for name, skews in bc.STORE_PLACEMENTS.items():
            res, out = run_store(ctx, opt, sim, LAYOUTS[layout], skews)
            assert res.n == n_local
            if base is None:
                base, base_res = out, res
                traj, cnt, pay = out
                assert torch.isfinite(traj).all() and (traj > 0).all() and torch.isfinite(pay).all() and (pay >= 0).all()
                assert (cnt >= 0).all() and (cnt <= n_steps).all()
                assert close_to(res.sum, math.fsum(pay.cpu().numpy()), 1e-13)
                continue
            for got, want, what in zip(out, base, ("traj", "counts", "payoffs")):
                assert got is None or same_bits(got, want), (n_steps, name, what)
            assert (res.sum, res.sumsq) == (base_res.sum, base_res.sumsq), (n_steps, name)
        if n_local == bc.restated_size(prec) and n_steps == 9:
            check_stored_rows(prec, layout, base, n_local, n_steps)


def check_stored_rows(prec, layout, out, n_local, n_steps):
    w = bc.store_wanted(prec, n_steps)
    traj, cnt, pay = out
    rows = by_path(traj, n_local, n_steps, LAYOUTS[layout]).astype(np.float64)
    counts = by_path(cnt, n_local, n_steps, LAYOUTS[layout])
    off = np.abs(rows - w.rows)
    assert (off <= w.tol_rows).all(), (np.argwhere(off > w.tol_rows)[:8], off.max())
    flags = np.diff(counts, axis=1, prepend=0)
    assert ((flags == 0) | (flags == 1)).all()
    wrong = (flags != w.below) & w.clear
    assert not wrong.any(), np.argwhere(wrong)[:8]
    used = check_payoffs(pay.cpu().numpy(), w.pp, layout)
    print(f"f{prec} {layout} store of {n_local} x {n_steps}: largest share of the tolerance of a stored price "
          f"{(off / w.tol_rows).max():.2e}, of a payoff {used:.2e}; {np.count_nonzero(~w.clear)} comparisons within MARGIN of "
          f"the barrier, {np.count_nonzero((flags != w.below) & ~w.clear)} of them decided the other way")


@pytest.mark.parametrize("n_local", bc.WIDE, ids=["2^29", "2^29+1"])
@pytest.mark.parametrize("prec", wc.PRECS)
def test_store_with_wide_offsets(ctx, prec, n_local):
    # n_local + V > (2^32 - 1) / 8: store_kernel's `narrow` is false and a row's byte offsets are 64-bit; 2^29 is a
    # multiple of V (vector stores), 2^29 + 1 is not (guarded scalar stores).  Allocation plus a few ms of kernel.
    n_steps, item = 2, bc.ITEM[prec]
    need = n_local * (n_steps * (item + 4) + item)
    free, _ = torch.cuda.mem_get_info()
    if free < need + (2 << 30):
        pytest.skip(f"not enough free HBM for the {need / 1e9:.1f} GB of the wide store's buffers")
    opt = bc.store_option(bc.WIDE_WINDOW)
    res, (traj, cnt, pay) = run_store(ctx, opt, bc.store_sim(prec, n_local, n_steps, first=0, n_job=n_local), capi.STEP_MAJOR, (0, 0, 0))
    assert res.n == n_local
    assert torch.isfinite(traj).all() and (cnt >= 0).all() and (cnt <= n_steps).all() and torch.isfinite(pay).all()
    assert close_to(res.sum, pay.double().sum().item(), 1e-12)
    rows, crows = traj.view(n_steps, n_local), cnt.view(n_steps, n_local)
    for lo in (0, n_local - 64):
        small = bc.store_sim(prec, 64, n_steps, first=lo, n_job=n_local)
        t2 = torch.full((n_steps * 64,), NAN, dtype=TORCH_T[prec], device="cuda")
        c2 = torch.full((n_steps * 64,), bc.COUNT_POISON, dtype=torch.int32, device="cuda")
        p2 = torch.full((64,), NAN, dtype=TORCH_T[prec], device="cuda")
        assert ctx.simulate_trajectories(opt, small, t2, c2, p2, capi.STEP_MAJOR).n == 64
        assert torch.isfinite(t2).all() and torch.isfinite(p2).all()
        assert same_bits(rows[:, lo:lo + 64].contiguous(), t2.view(n_steps, 64)), lo
        assert same_bits(crows[:, lo:lo + 64].contiguous(), c2.view(n_steps, 64)), lo
        assert same_bits(pay[lo:lo + 64].contiguous(), p2), lo
    del traj, cnt, pay, rows, crows
    torch.cuda.empty_cache()


# ---------------- 4. store pattern ----------------
@pytest.mark.parametrize("prec", wc.PRECS)
def test_store_pattern(ctx, prec):
    T, item, V, n, steps = TORCH_T[prec], bc.ITEM[prec], bc.VEC[prec], bc.pattern_size(prec), bc.PATTERN_STEPS
    want = np.arange(n)[None, :] + np.arange(steps)[:, None]
    for with_payoffs in (True, False):
        tw, tv = bc.placed(n * steps, T, 0, NAN)
        pw, pv = bc.placed(n, T, 0, NAN)
        before = bc.guards(tw, tv), bc.guards(pw, pv)
        ms = ctx.diag_store_pattern(n, steps, prec, tv, pv if with_payoffs else None)
        assert ms > 0
        assert bc.untouched(tw, tv, before[0]) and bc.untouched(pw, pv, before[1])
        assert np.array_equal(tv.cpu().numpy().reshape(steps, n), want.astype(bc.NP_T[prec]))
        if with_payoffs:
            assert np.array_equal(pv.cpu().numpy(), (np.arange(n) + steps).astype(bc.NP_T[prec]))
        else:
            assert torch.isnan(pv).all()
    # n = 0 writes nothing
    tw, tv = bc.placed(n * steps, T, 0, NAN)
    assert ctx.diag_store_pattern(0, steps, prec, tv, None) == 0.0 and torch.isnan(tw).all()
    # the refusals: a ragged n, d_traj or d_payoffs one element off; nothing is written
    pw, pv = bc.placed(n, T, 0, NAN)
    _, t_off = bc.placed(n * steps, T, item, NAN)
    _, p_off = bc.placed(n, T, item, NAN)
    for args in ((n - 1, steps, prec, tv, pv), (n, steps, prec, t_off, pv), (n, steps, prec, tv, p_off)):
        with pytest.raises(capi.McamdError, match=bc.PATTERN_REFUSAL):
            ctx.diag_store_pattern(*args)
    assert all(torch.isnan(t).all() for t in (tw, pw, t_off, p_off))
    assert V * item == 16


# ---------------- 5. reductions ----------------
@pytest.mark.parametrize("prec", wc.PRECS)
@pytest.mark.parametrize("variant", bc.REDUCE_VARIANTS)
def test_reduce_at_every_placement(ctx, variant, prec):
    worst = 0.0
    for n in bc.reduce_sizes(prec):
        x = bc.reduce_input(prec, n)
        want = math.fsum(x.astype(np.float64))
        xt = torch.from_numpy(x)
        for skew in bc.reduce_skews(prec):
            whole, view = bc.placed(n, TORCH_T[prec], skew, NAN)
            view.copy_(xt)
            assert torch.isnan(whole).sum().item() == whole.numel() - n
            s, _ = ctx.reduce_sum(view, n, prec, variant)
            assert math.isfinite(s), (n, skew)
            assert close_to(s, want, 1e-12), (n, skew, s, want)
            worst = max(worst, abs(s - want) / abs(want))
    print(f"f{prec} variant {variant}: largest relative deviation from the host's fp64 sum {worst:.1e}")
