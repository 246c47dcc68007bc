"""CPU checks of what tests/test_gpu_buffers.py compares the kernels with (tests/buffer_cases.py): the placement helper
puts a buffer where it says and sees a touched guard band, the float64 restatement of the array-driven pricer is the
oracle's, the chosen inputs meet the caps the tolerances rest on, and each restated mistake of the cache-line-tiled
loop lies beyond the tolerance the GPU test allows.  No kernel runs here.

Measured here (printed by the tests; pytest -s), over the 130 paths of every case of the array-driven pricer:
  * |ln S_t| between the two restatements at most 3.9e-16 (float64 / longdouble) and 2.9e-7 (float32 / float64, 252
    steps), so MARGIN = 2e-5 is 68 times the fp32 figure where 4 are asked for;
  * payoff spreads at most 4.7e-14 (fp64) and 4.2e-5 (fp32; 4.1e-5 with a window): a payoff's tolerance is 1.7e-11 ..
    1.3e-8 (fp64) and 3.5e-5 .. 2.1e-3 (fp32; four spreads at the low end, the floor 2e-5 of the payoff at the high end);
  * windowed cases: 4 (fp32) and 10 (fp64) paying paths at 1 step, at least 13 elsewhere (the restart cases; 23 without
    them); at least 25 paths in the money and shut out by the window; one undecided sample (fp32, 28 steps);
  * a row read one vector late or short of its last vector moves 14 .. 117 of a case's 130 payoffs beyond the
    tolerance.  The count that also takes the neighbour's vectors in the row's first line moves 3 .. 71 of them at
    every skew 16 .. 112 and at skew 0 none where a row is a whole number of lines (128-byte rows, the 64-step
    restart): the suite ran skew 0 alone before;
  * the stored rows of 256 V + 1 paths x 9 steps: price spread 3.3e-14 / 3.1e-5, so a price's tolerance is 5.5e-9 ..
    2.1e-8 (fp64) and 1.2e-3 .. 4.1e-3 (fp32, the floor); all but 0.01 % of the comparisons are clear of the barrier."""
import numpy as np
import pytest

import buffer_cases as bc
import window_cases as wc

capi = bc.capi
MIN_SHUT_OUT = 0.10    # of a windowed case's paths: in the money at T and paid nothing


def test_placed_puts_the_buffer_where_it_says_and_untouched_sees_a_write():
    torch = pytest.importorskip("torch")
    for dtype, poison in ((torch.float32, float("nan")), (torch.float64, float("nan")), (torch.int32, bc.COUNT_POISON)):
        item = torch.empty(0, dtype=dtype).element_size()
        for n in (1, 5, 130):
            for skew in sorted({0, item, 16, 16 + item, 112, 128 - item}):
                whole, view = bc.placed(n, dtype, skew, poison, device="cpu")
                assert view.numel() == n and view.data_ptr() % 128 == skew
                lo = (view.data_ptr() - whole.data_ptr()) // item
                assert lo * item >= bc.GUARD and (whole.numel() - lo - n) * item >= bc.GUARD
                before = bc.guards(whole, view)
                assert before[0].numel() == lo and before[1].numel() == whole.numel() - lo - n
                assert bc.untouched(whole, view, before)
                view.fill_(1)                                   # the buffer itself may be written
                assert bc.untouched(whole, view, before)
                for at in (lo - 1, lo + n, 0, whole.numel() - 1):   # the elements next to it and the far ends may not
                    kept = whole[at].clone()
                    whole[at] = 1
                    assert not bc.untouched(whole, view, before), (dtype, n, skew, at)
                    whole[at] = kept
                    assert bc.untouched(whole, view, before)
    # every base address mod 128 gives a start with the asked skew and a full guard before it
    for item in (4, 8):
        for base in range(0, 256, item):
            for skew in range(0, 128, item):
                s = bc.start_of(base, item, skew)
                assert (base + s * item) % 128 == skew and bc.GUARD <= s * item < bc.GUARD + 128
    assert bc.COUNT_POISON < 0 and np.int32(bc.COUNT_POISON).view(np.float32) == np.float32(-777.25)


@pytest.mark.parametrize("prec", wc.PRECS)
def test_float64_restatement_is_the_oracle_without_a_window(oracle, prec):
    for case in bc.fn_cases(prec):
        if "Tk" in case.extra:
            continue    # the oracle's array-driven pricer has no restart
        z = bc.fn_normals(case, prec)
        opt = bc.fn_option(case, 0)
        _, want = oracle.price_from_normals(z.astype(np.float64).ravel(), bc.N_PATHS, case.n_steps, opt.S0, opt.v, opt.r,
                                            opt.K, opt.T)
        got = bc.fn_restated(case, prec, 0, np.float64)
        assert got.decided.all() and np.allclose(got.y, want, rtol=1e-12, atol=1e-12), case.name
        assert ((got.y == 0) == (want == 0)).all()


@pytest.mark.parametrize("prec", wc.PRECS)
def test_rows_are_the_buffers_rows_and_the_step_counts_sit_where_the_table_says(prec):
    item, V = bc.ITEM[prec], bc.VEC[prec]
    cases = bc.fn_cases(prec)
    row_bytes = sorted({bc.n_sim(c) * item for c in cases if bc.n_sim(c) % V == 0 and "Tk" not in c.extra})
    assert set(row_bytes) >= {16, 112, 128, 144, 240, 1008} and all(b % 16 == 0 for b in row_bytes)
    assert {bc.n_sim(c) for c in cases if bc.n_sim(c) % V} == {1, 33, 63}
    assert [bc.n_sim(c) for c in cases if "Tk" in c.extra] == [63, 64]
    assert {s % 16 for s in bc.SKEWS_ELEMENT[prec]} - {0} and all(s % item == 0 and s % 16 for s in bc.SKEWS_ELEMENT[prec])
    for case in cases:
        z = bc.fn_normals(case, prec)
        flat = z.ravel()
        assert z.shape == (bc.N_PATHS, bc.n_sim(case)) and z.dtype == bc.NP_T[prec]
        assert np.array_equal(flat[5 * bc.n_sim(case):6 * bc.n_sim(case)], z[5])
        assert bc.on_vec_path(case, prec, 0) == (bc.n_sim(case) % V == 0) and not bc.on_vec_path(case, prec, item)
        assert bc.job_sizes(case)[0] == bc.N_PATHS and bc.N_PATHS == 2 * 64 + 2
    assert sum(len(bc.job_sizes(c)) > 1 for c in cases) == 2


@pytest.mark.parametrize("prec", wc.PRECS)
def test_margin_spreads_and_caps_of_the_array_driven_cases(prec):
    worst_log, worst_spread, tol_lo, tol_hi = 0.0, 0.0, np.inf, 0.0
    for case in bc.fn_cases(prec):
        ls = bc.fn_log_spread(case, prec)
        worst_log = max(worst_log, ls)
        assert wc.MARGIN >= 4.0 * ls, (case.name, ls)
        for use_window in (0, 1):
            w = bc.fn_wanted(case, prec, use_window)
            m = w.want.members[0]
            undecided, paying = np.count_nonzero(~w.want.decided), np.count_nonzero(w.want.y)
            shut_out = np.count_nonzero((m.full > 0) & (w.want.y == 0) & w.want.decided)
            worst_spread, tol_lo, tol_hi = max(worst_spread, w.spread_y), min(tol_lo, w.tol_y.min()), max(tol_hi, w.tol_y.max())
            print(f"f{prec} {case.name} window {use_window}: paying {paying}, shut out {shut_out}, undecided {undecided}, "
                  f"ln S spread {ls:.2e}, spread y {w.spread_y:.2e}, tolerance {w.tol_y.min():.1e} .. {w.tol_y.max():.1e}")
            assert undecided <= 1
            assert paying >= wc.MIN_PAYING * bc.N_PATHS
            assert (w.tol_y > 0).all()
            if use_window:
                assert shut_out >= MIN_SHUT_OUT * bc.N_PATHS
            else:
                assert w.want.decided.all() and shut_out == 0
    print(f"f{prec}: largest ln S spread {worst_log:.2e} (MARGIN / spread = {wc.MARGIN / worst_log:.0f}), largest spread y "
          f"{worst_spread:.2e}, tolerances {tol_lo:.1e} .. {tol_hi:.1e}")


@pytest.mark.parametrize("prec", wc.PRECS)
def test_mistakes_of_the_tiled_loop_are_beyond_the_tolerances(prec):
    for case in bc.fn_cases(prec):
        if not bc.on_vec_path(case, prec, 0):
            continue
        for use_window in (0, 1):
            w = bc.fn_wanted(case, prec, use_window)
            for mistake in (bc.ROW_ONE_VECTOR_LATE, bc.LAST_VECTOR_DROPPED):
                moved = wc.outside(bc.mistaken(case, prec, use_window, mistake), w) & w.want.decided
                print(f"f{prec} {case.name} window {use_window} mistake {mistake}: {moved.sum()} of {bc.N_PATHS} payoffs "
                      f"beyond the tolerance")
                assert moved.any(), (case.name, use_window, mistake)
            if use_window:
                # what a row shares its first line with depends on where the buffer starts: at every start but a
                # multiple of 128 the mistake shows, and rows of whole lines hide it from a test that only runs skew 0
                n_moved = [int((wc.outside(bc.mistaken(case, prec, 1, bc.COUNT_TAKES_NEIGHBOUR, skew), w) & w.want.decided).sum())
                           for skew in bc.SKEWS_16]
                print(f"f{prec} {case.name} window 1 mistake {bc.COUNT_TAKES_NEIGHBOUR}: payoffs beyond the tolerance at "
                      f"skew 0, 16, .. 112: {n_moved}")
                assert all(n_moved[1:]), (case.name, n_moved)
                assert (n_moved[0] == 0) == (bc.n_sim(case) * bc.ITEM[prec] % 128 == 0)


@pytest.mark.parametrize("prec", wc.PRECS)
def test_store_restatement_and_the_shapes(oracle, prec):
    V = bc.VEC[prec]
    assert set(bc.store_sizes(prec)) == {1, V - 1, V, V + 1, 2 * V - 1, 256 * V, 256 * V + 1, 256 * V + V - 1}
    assert {s % 4 for s in bc.STORE_STEPS} == {1, 3} and {s % 2 for s in bc.STORE_STEPS} == {1} and bc.restated_size(prec) % V
    assert all(n + V > 0xffffffff // 8 for n in bc.WIDE) and bc.WIDE[0] % 4 == 0 and bc.WIDE[1] % 2 == 1
    w = bc.store_wanted(prec)
    opt, sim = bc.store_option(), bc.store_sim(prec, bc.restated_size(prec), 9)
    paying, undecided = np.count_nonzero(w.pp.want.y), np.count_nonzero(~w.pp.want.decided)
    print(f"f{prec} store rows: price spread {w.spread_rows:.2e}, tolerance {w.tol_rows.min():.1e} .. {w.tol_rows.max():.1e}; "
          f"{w.clear.mean():.4f} of the comparisons clear of the barrier; paying {paying}, undecided {undecided}, payoff "
          f"spread {w.pp.spread_y:.2e}")
    assert w.clear.mean() > 0.999 and undecided <= wc.MAX_UNDECIDED * sim.n_paths_local
    assert paying >= wc.MIN_PAYING * sim.n_paths_local
    if prec == capi.F64:    # the float64 restatement is the oracle's stored rows
        ref = oracle.mc_paths(wc.oracle_params(oracle, opt, sim), prec, sim.path_offset, sim.n_paths_local,
                              want_payoffs=True, want_traj=True, want_counts=True)
        assert np.allclose(w.rows, ref["traj"].T, rtol=1e-12, atol=0)
        assert np.array_equal(np.cumsum(w.below, axis=1), ref["counts"].T)
        assert np.allclose(w.pp.want.y, ref["payoffs"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("prec", wc.PRECS)
def test_reduce_inputs_have_one_sign(prec):
    for n in bc.reduce_sizes(prec):
        x = bc.reduce_input(prec, n)
        assert x.dtype == bc.NP_T[prec] and len(x) == n and (x >= 0.5).all() and (x < 1.5).all()
    assert set(bc.reduce_skews(prec)) == {0, 16} | set(range(bc.ITEM[prec], 16, bc.ITEM[prec]))
