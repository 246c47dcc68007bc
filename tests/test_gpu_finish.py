"""The record finish — block sum, publication, hand-off, the last workgroup's sum, the separate sums — at every record
count, width and hand-off, against tests/finish_restate.py (the order the code documents, in numpy float64) and math.fsum.

Every pricing call ends in this code, and before this module nothing compared it with anything independent: grid_finish
was compared with small_final_kernel (both call small_final_sum), final_reduce_kernel with itself, a call with its own
repeat.  tests/finish_check.hip runs the shipped functions on records the tests supply; nothing here walks a path, except
section 7, which goes through the public calls.

Two kinds of data.  Integers: record i, slot k holds (i + 1)(k + 1); every sum is exact, and a dropped, doubled or
misplaced record changes slot 0 by its number.  Wide floats: normals scaled by 2^[-20, 20); the sums must be the
restatement's bits (tests/test_finish_cpu.py shows that most of them are not the front-to-back sum's) and within
n 2^-53 sum |x| of math.fsum, the worst case of any order.  Every tolerance is one of the two: exact, or that bound.

  1. block_sumN<256, N> for N = 2, 3, 4, 5, 6, 7, 12, 28, block_sumN<1024, N> for N = 2, 4, 5, block_sum2<256>: integers,
     wide floats, and a one-hot input in every lane (lane l arrives unchanged).
  2. small_final_sum<256, N, ACC> for (2, 4), (4, 4), (5, 4), (6, 4), (7, 4), (12, 4), (28, 1) at every record count
     0 .. 1100, 2047-2049, 3071-3073, 4095-4097, 8191, 8192, one workgroup per count; the records beyond 8192 are NaN.
  3. finish_paths<N, ACC> (N = 2, 4, 6 with ACC 4; N = 28 with ACC 1) at grids 1, 2, 7, 8, 9, 255-257, 767-769,
     1023-1025, 4096, 8191, 8192: sixteen launches back to back on one stream over ONE partials array and ONE ticket,
     launch r adding r 2^32 to every record, eight workgroups (3 r + j) % grid delayed by a bounded sleep.  A record
     left over from launch r - 1 leaves the sum short by 2^32.  The ticket reads 0 afterwards, the guard bands around it
     and beyond the partials keep their poison.  The final records in device memory and in pinned host memory.
     Wide floats (N = 2, 5): the bits of the restatement and of launch_small_final on the same records.
  4. write_final: the statistics layout at N = 2, 4, 5, 6 (out[5] is n, not the sixth sum), poison kept with n < 0.
  5. launch_small_final (widths 2, 5; section 2's counts) and launch_final_reduce (widths 2, 4, 5; 1, 1023-1025, ..,
     8191-8193, 16384, 16385, 2^20 - 1, 2^20): both kinds of data, the statistics layout, and a width nobody instantiated.
  6. launch_smile_finish at n_nodes in {1, 63, 64, 255, 256, 257, 2048} x n_waves in {1, 7, 8, 9, 16, 17, 2048} (the
     largest is the whole kSmilePartialsBudget).
  7. Through the public calls, one per record width that hands back samples: Heston (4), cliquet (5), Asian with its
     control (6), autocall (7; 6 from its enqueue form), at n_steps = 1 in fp64 and grids 255, 257, 769, 1025, 8192 and
     8192 x 256 + 1 paths (grid-stride): res.sum and res.sumsq within the bound of math.fsum over the samples, every
     integer counter equal to its count.  Each enqueue form twice in a row with different seeds into two rows.
     Widths only the harness covers: 2 (the plain pricer hands back no samples), 12 (Greeks, American sweep) and 28
     (local-volatility Greeks, whose samples are not the record's slots).

Largest deviations on an MI355X (printed by each test and recorded as junit properties).  No sum differed in bits from
the restatement anywhere (sections 1, 2, 3, 5, 6), no hot lane changed, no record was stale in any of the 2176 hand-off
launches, every integer sum was exact.  Largest error as a fraction of the bound n 2^-53 sum |x|: small_final_sum
0.39, 0.46, 0.38, 0.34, 0.49, 0.63, 0.47 for the seven (N, ACC) in the order above; the hand-off's wide floats 0.21 (N = 2) and 0.24 (N = 5); launch_final_reduce
2.2e-4, 3.7e-4, 4.0e-4 (widths 2, 4, 5); the public calls 2.4e-5 (Heston), 2.2e-5 (cliquet), 2.7e-5 (Asian), 1.7e-5
(autocall).  The whole module takes ten seconds, the harness's compilation included."""
import importlib
import math

import numpy as np
import pytest

import buffer_cases as bc
import finish_harness as fh
import finish_restate as fr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

NAN = float("nan")
HIP_INVALID = 1          # hipErrorInvalidValue
TWO32 = 2.0 ** 32
ROW = 32                 # doubles of a final record's row in these tests: the widest record and room to spare
PAD = 64                 # NaN records beyond the largest count
HANDOFF_GRIDS = (1, 2, 7, 8, 9, 255, 256, 257, 767, 768, 769, 1023, 1024, 1025, 4096, 8191, 8192)
HANDOFF = ((2, 4), (4, 4), (6, 4), (28, 1))
ROUNDS = 16


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    import os
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    torch.cuda.set_device(0)
    lib = fh.load(fh.compile_harness(tmp_path_factory.mktemp("finish")))

    class Synced:
        """the harness runs on streams of its own: what torch enqueued (copies, poison fills) is finished first"""
        def __getattr__(self, name):
            call = getattr(lib, name)

            def synced(*args):
                torch.cuda.synchronize()
                return call(*args)
            return synced
    return Synced()


def dev(a):
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def poisoned(*shape):
    return torch.full(shape, NAN, dtype=torch.float64, device="cuda")


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def padded(rec):
    """rec with PAD records of NaN behind it: a read past the end shows in the sum"""
    return np.concatenate([rec, np.full((PAD, rec.shape[1]), NAN)])


def within_bound(got, exact, sum_abs, n):
    """(ok, largest |got - exact| as a fraction of the bound n 2^-53 sum |x|)"""
    bound = np.asarray(n, dtype=np.float64) * 2.0 ** -53 * sum_abs
    err = np.abs(got - exact)
    frac = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    return bool(np.all(err <= bound)), float(frac.max(initial=0.0))


_wide = {}


def wide(n, width):
    """the wide floats [n, width] with the math.fsum of every prefix, computed once"""
    key = (n, width)
    if key not in _wide:
        rec = fr.wide_floats(n, width)
        rec.setflags(write=False)
        _wide[key] = (rec,) + fr.prefix_fsums(rec)
    return _wide[key]


# ---- 1. block sums -----------------------------------------------------------------------------------------------------

BLOCK_SUMS = [(256, n, 0) for n in fr.BLOCK_SUM_WIDTHS] + [(1024, n, 0) for n in fr.FINAL_WIDTHS] + [(256, 2, 1)]


@pytest.mark.parametrize("block,width,sum2", BLOCK_SUMS, ids=lambda v: str(v))
def test_block_sums(L, block, width, sum2, record_property):
    n_blocks = 3
    ints = fr.integers(n_blocks * block, width).reshape(n_blocks, block, width)      # thread t of block 0: (t + 1)(k + 1)
    out = poisoned(n_blocks, width)
    d_in = dev(ints)
    assert L.fc_block_sum(block, width, sum2, 0, n_blocks, d_in.data_ptr(), out.data_ptr()) == 0
    assert np.array_equal(host(out), ints.sum(axis=1)) and np.array_equal(host(out)[0], fr.integer_sum(block, width))
    floats = fr.wide_floats(n_blocks * block, width).reshape(n_blocks, block, width)
    out = poisoned(n_blocks, width)
    d_in = dev(floats)
    assert L.fc_block_sum(block, width, sum2, 0, n_blocks, d_in.data_ptr(), out.data_ptr()) == 0
    want = np.stack([fr.block_sum(floats[b]) for b in range(n_blocks)])
    differing = int(np.count_nonzero(host(out).view(np.uint64) != want.view(np.uint64)))
    record_property("sums_differing_from_the_restatement", differing)
    assert differing == 0, (host(out), want)
    # one workgroup per hot lane: thread b of workgroup b holds vals[b], every other thread 0
    vals = fr.wide_floats(block, width, fr.SEED + 1)
    out = poisoned(block, width)
    d_in = dev(vals)
    assert L.fc_block_sum(block, width, sum2, 1, block, d_in.data_ptr(), out.data_ptr()) == 0
    lanes = np.flatnonzero((host(out).view(np.uint64) != vals.view(np.uint64)).any(axis=1))
    print(f"block_sum{'2' if sum2 else 'N'}<{block}, {width}>: {differing} sums differ from the restatement, "
          f"{lanes.size} of {block} hot lanes changed")
    assert lanes.size == 0, lanes[:8]


# ---- 2. small_final_sum ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width,acc", fr.INSTANTIATED)
def test_small_final_sum_at_every_record_count(L, width, acc, record_property):
    counts = np.array(fr.SMALL_COUNTS, dtype=np.uint32)
    top = int(counts.max())
    d_counts = dev(counts)
    out = poisoned(counts.size, width)
    d_rec = dev(padded(fr.integers(top, width)))
    assert L.fc_small_final_sum(width, acc, d_rec.data_ptr(), d_counts.data_ptr(), counts.size, out.data_ptr()) == 0
    c = counts.astype(np.float64)
    want = np.outer(c * (c + 1.0) / 2.0, np.arange(width) + 1.0)
    bad = np.flatnonzero((host(out) != want).any(axis=1))
    assert bad.size == 0, [(int(counts[b]), (host(out)[b] - want[b]).tolist()) for b in bad[:4]]
    rec, exact, sum_abs = wide(top, width)
    out = poisoned(counts.size, width)
    d_rec = dev(padded(rec))
    assert L.fc_small_final_sum(width, acc, d_rec.data_ptr(), d_counts.data_ptr(), counts.size, out.data_ptr()) == 0
    got = host(out)
    want = np.stack([fr.small_final_sum(rec[:n], 256, acc) for n in counts])
    bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
    ok, frac = within_bound(got, exact[counts], sum_abs[counts], counts[:, None])
    record_property("counts_differing_from_the_restatement", int(bad.size))
    record_property("largest_error_over_bound", frac)
    print(f"small_final_sum<256, {width}, {acc}>: {bad.size} of {counts.size} record counts differ from the restatement; "
          f"largest error {frac:.3g} of the bound")
    assert bad.size == 0, [(int(counts[b]), got[b].tolist(), want[b].tolist()) for b in bad[:4]]
    assert ok


# ---- 3. the hand-off ---------------------------------------------------------------------------------------------------

def handoff(L, width, acc, grid, rec, add_unit, n_value, pinned):
    """ROUNDS launches over one partials array and one ticket -> rows [ROUNDS, ROW] (numpy), after checking that the
    ticket is zero again and that the guard bands of both buffers kept their poison"""
    part_whole, part = bc.placed(grid * width, torch.float64, 0, NAN)
    tick_whole, tick = bc.placed(1, torch.int32, 0, bc.COUNT_POISON)
    tick.zero_()
    before = bc.guards(part_whole, part), bc.guards(tick_whole, tick)
    d_rec = dev(rec)
    if pinned:
        rows = np.full((ROUNDS, ROW), NAN)
        where = rows.ctypes.data
    else:
        d_rows = poisoned(ROUNDS, ROW)
        where = d_rows.data_ptr()
    torch.cuda.synchronize()
    rc = L.fc_handoff(width, acc, grid, ROUNDS, d_rec.data_ptr(), add_unit, n_value, part.data_ptr(), tick.data_ptr(),
                      where, ROW, 1 if pinned else 0)
    assert rc == 0, rc
    if not pinned:
        rows = host(d_rows)
    assert int(tick.item()) == 0, "the last workgroup leaves the ticket zero"
    assert bc.untouched(part_whole, part, before[0]), "a write beyond grid x N doubles of the partials"
    assert bc.untouched(tick_whole, tick, before[1]), "a write beside the ticket"
    return rows


@pytest.mark.parametrize("pinned", [False, True], ids=["device-record", "pinned-host-record"])
@pytest.mark.parametrize("width,acc", HANDOFF)
def test_handoff_under_changing_values(L, width, acc, pinned, record_property):
    stale_most = 0
    for grid in HANDOFF_GRIDS:
        n_value = float(grid) if pinned and width <= 6 else -1.0    # the synchronous calls' record is pinned host memory
        rows = handoff(L, width, acc, grid, fr.integers(grid, width), TWO32, n_value, pinned)
        want = np.full((ROUNDS, ROW), NAN)
        want[:, :width] = fr.integer_sum(grid, width)[None, :] + grid * TWO32 * np.arange(ROUNDS)[:, None]
        if n_value >= 0.0:
            want[:, width:5] = 0.0
            want[:, 5] = n_value                                   # at N = 6 too: n, never the sixth sum
        short = (want[:, 0] - rows[:, 0]) / TWO32                  # slot 0: a stale record leaves the sum short by 2^32
        stale = np.where(np.isfinite(short), np.round(short), -1.0)
        stale_most = max(stale_most, int(np.abs(stale).max()))
        assert same_bits(rows, want), (
            f"N {width} grid {grid}: launches {np.flatnonzero((rows[:, :width] != want[:, :width]).any(axis=1)).tolist()} "
            f"are wrong; stale records per launch {stale.tolist()}, what is left of slot 0 beyond them "
            f"{(want[:, 0] - rows[:, 0] - stale * TWO32).tolist()}; launch 1's row {rows[1, :8].tolist()}")
    record_property("most_stale_records", stale_most)
    print(f"finish_paths<{width}, {acc}> {'pinned' if pinned else 'device'} record: {len(HANDOFF_GRIDS)} grids x {ROUNDS} "
          f"launches, most stale records in a launch {stale_most}")


@pytest.mark.parametrize("width", [2, 5])
def test_handoff_sum_is_the_restatement_and_the_separate_launch(L, width, record_property):
    rec_all, exact, sum_abs = wide(8192, width)
    counts = np.array(HANDOFF_GRIDS, dtype=np.uint32)
    separate = poisoned(counts.size, 8)
    status = fh.C.c_int(-1)
    d_all = dev(padded(rec_all))
    assert L.fc_library_sum(0, d_all.data_ptr(), counts.ctypes.data, counts.size, width, -1.0,
                            separate.data_ptr(), 8, fh.C.byref(status), None) == 0 and status.value == 0
    worst = 0.0
    for row, grid in enumerate(HANDOFF_GRIDS):
        rows = handoff(L, width, 4, grid, rec_all[:grid], 0.0, -1.0, False)
        want = fr.small_final_sum(rec_all[:grid], 256, 4)
        for r in range(ROUNDS):
            assert same_bits(rows[r, :width], want), (grid, r, rows[r, :width], want)
        assert same_bits(host(separate)[row, :width], want), (grid, host(separate)[row], want)
        ok, frac = within_bound(want, exact[grid], sum_abs[grid], grid)
        worst = max(worst, frac)
        assert ok
    record_property("largest_error_over_bound", worst)
    print(f"finish_paths<{width}, 4> on wide floats: the restatement's and launch_small_final's bits at {counts.size} grids; "
          f"largest error {worst:.3g} of the bound")


# ---- 4. write_final ----------------------------------------------------------------------------------------------------

def test_write_final_layouts(L):
    v = np.array([1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5])
    d_v = dev(v)
    for n in (2, 4, 5, 6):
        out = poisoned(8)
        assert L.fc_write_final(d_v.data_ptr(), n, 1234.0, out.data_ptr()) == 0
        want = np.concatenate([v[:min(n, 5)], np.zeros(max(5 - n, 0)), [1234.0, NAN, NAN]])
        assert same_bits(host(out), want), (n, host(out))          # at N = 6 out[5] is n, not the sixth sum
        out = poisoned(8)
        assert L.fc_write_final(d_v.data_ptr(), n, -1.0, out.data_ptr()) == 0
        assert same_bits(host(out), np.concatenate([v[:n], np.full(8 - n, NAN)])), (n, host(out))
    out = poisoned(8)
    assert L.fc_write_final(d_v.data_ptr(), 2, 0.0, out.data_ptr()) == 0      # n = 0 is a count, not "none"
    assert same_bits(host(out), np.array([1.5, 2.5, 0.0, 0.0, 0.0, 0.0, NAN, NAN]))


# ---- 5. the library's separate sums --------------------------------------------------------------------------------------

def library_sum(L, which, d_rec, counts, width, n_value):
    """(status, out [len(counts), 8], after [8])"""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    out, after = poisoned(counts.size, 8), poisoned(8)
    status = fh.C.c_int(-1)
    assert L.fc_library_sum(which, d_rec.data_ptr(), counts.ctypes.data, counts.size, width, n_value, out.data_ptr(), 8,
                            fh.C.byref(status), after.data_ptr()) == 0
    return status.value, host(out), host(after)


def layout(sums, width, n_value):
    """[rows, 8]: what a launcher leaves of `sums` [rows, width] in rows of 8 poisoned doubles"""
    rows = np.full((sums.shape[0], 8), NAN)
    rows[:, :width] = sums
    if n_value >= 0.0:
        rows[:, width:5] = 0.0
        rows[:, 5] = n_value
    return rows


LIBRARY = [(0, w) for w in (2, 5)] + [(1, w) for w in fr.FINAL_WIDTHS]


@pytest.mark.parametrize("which,width", LIBRARY, ids=lambda v: str(v))
def test_library_sums(L, which, width, record_property):
    name = ("launch_small_final", "launch_final_reduce")[which]
    counts = np.array((fr.SMALL_COUNTS, fr.FINAL_COUNTS)[which], dtype=np.uint32)
    restated = (lambda r: fr.small_final_sum(r, 256, 4), fr.final_reduce)[which]
    top = int(counts.max())
    c = counts.astype(np.float64)
    d_ints = dev(padded(fr.integers(top, width)))
    for n_value in (-1.0, 7.0):
        status, out, _ = library_sum(L, which, d_ints, counts, width, n_value)
        want = layout(np.outer(c * (c + 1.0) / 2.0, np.arange(width) + 1.0), width, n_value)
        assert status == 0 and same_bits(out, want), np.flatnonzero((out != want).any(axis=1))[:8]
    del d_ints
    rec = fr.wide_floats(top, width)
    status, out, _ = library_sum(L, which, dev(padded(rec)), counts, width, 7.0)
    want = np.stack([restated(rec[:n]) for n in counts])
    bad = np.flatnonzero((out[:, :width].view(np.uint64) != want.view(np.uint64)).any(axis=1))
    record_property("counts_differing_from_the_restatement", int(bad.size))
    assert status == 0 and bad.size == 0, [(int(counts[b]), out[b].tolist(), want[b].tolist()) for b in bad[:4]]
    assert same_bits(out, layout(want, width, 7.0))
    worst = 0.0
    cols, abs_cols = [rec[:, k].tolist() for k in range(width)], [np.abs(rec[:, k]).tolist() for k in range(width)]
    for row, n in enumerate(counts):
        n = int(n)
        exact = np.array([math.fsum(col[:n]) for col in cols])
        sum_abs = np.array([math.fsum(col[:n]) for col in abs_cols])
        ok, frac = within_bound(out[row, :width], exact, sum_abs, n)
        worst = max(worst, frac)
        assert ok, (n, out[row, :width] - exact)
    record_property("largest_error_over_bound", worst)
    print(f"{name} width {width}: the restatement's bits at {counts.size} record counts; largest error {worst:.3g} of the bound")


@pytest.mark.parametrize("which,width", [(0, 3), (0, 4), (0, 6), (1, 3), (1, 6), (1, 0)], ids=lambda v: str(v))
def test_a_width_nobody_instantiated_is_refused(L, which, width):
    rec = fr.integers(1025, 8)
    status, out, after = library_sum(L, which, dev(rec), [1025, 7], width, 7.0)
    assert status == HIP_INVALID
    assert same_bits(out, np.full((2, 8), NAN)), out                 # nothing written
    # the stream still takes work: the first 1025 records of the same array read at width 2
    flat = rec.reshape(-1, 2)[:1025]
    want = (lambda r: fr.small_final_sum(r, 256, 4), fr.final_reduce)[which](flat)
    assert same_bits(after, np.concatenate([want, np.full(6, NAN)])), after


# ---- 6. the smile's sum --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def smile_entries():
    n = max(fr.SMILE_NODES) * max(fr.SMILE_WAVES)
    assert n * 16 == 64 << 20                                         # kSmilePartialsBudget, csrc/smile.hpp
    j = np.arange(n, dtype=np.float64)
    e = np.stack([np.mod(j, 1021.0) + 1.0, (np.mod(j, 509.0) + 1.0) ** 2], axis=1)
    d = dev(e)
    e.setflags(write=False)
    assert d.data_ptr() % 16 == 0
    return e, d


def smile(L, d_entries, n_waves, n_nodes, n_value):
    out = poisoned(2 * n_nodes + 8)
    status = fh.C.c_int(-1)
    assert L.fc_smile_finish(d_entries.data_ptr(), n_waves, n_nodes, out.data_ptr(), n_value, fh.C.byref(status)) == 0
    assert status.value == 0
    return host(out)


@pytest.mark.parametrize("n_nodes", fr.SMILE_NODES)
def test_smile_finish(L, smile_entries, n_nodes):
    e, d = smile_entries
    for n_waves in fr.SMILE_WAVES:
        s = e[:n_waves * n_nodes].reshape(n_waves, n_nodes, 2).sum(axis=0)       # integers: exact in any order
        for n_value in (-1.0, 5.0):
            tail = np.full(8, NAN)
            if n_value >= 0.0:
                tail[0] = n_value
            got = smile(L, d, n_waves, n_nodes, n_value)
            assert same_bits(got, np.concatenate([s[:, 0], s[:, 1], tail])), (n_waves, n_nodes, n_value)
    w = fr.wide_floats(17 * n_nodes, 2)
    got = smile(L, dev(w), 17, n_nodes, -1.0)
    assert same_bits(got[:2 * n_nodes], fr.smile_finish(w, 17, n_nodes))          # in wave order


# ---- 7. through the public calls -----------------------------------------------------------------------------------------

PUBLIC_GRIDS = (255, 257, 769, 1025, 8192)
STRIDED = 8192 * 256 + 1
R, T_ = 0.05, 1.0


def paths_of(grid):
    """a path count whose launch has `grid` workgroups, the last one partly filled"""
    return (grid - 1) * 256 + 1 + grid % 200


def full_work(n, n_steps=1):
    return 64 * -(-n // 64) * n_steps


@pytest.fixture(scope="module")
def ctx(L):
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    c = capi.Context(0, stream.cuda_stream)
    yield c
    c.close()
    torch.cuda.set_stream(torch.cuda.default_stream())


@pytest.fixture(scope="module")
def surface(ctx):
    x = np.linspace(-1.5, 1.5, 33)
    s = ctx.localvol_surface((1, 33, -1.5, 1.5), [0.2 - 0.05 * x])
    yield s
    s.close()


def _heston(ctx, surface, sim, y):
    opt = capi.make_option(S0=100.0, K=100.0, r=R, T=T_, v=NAN, B=NAN)
    return ctx.price_heston(opt, sim, capi.make_heston(capi.PAYOFF_CALL, 0.01), y)


def _heston_counters(res, y, n):
    # one step entered at v0 > 0: nothing truncated; the mean variance is n copies of v0 summed and divided by n
    assert res.truncated_steps == 0.0 and res.work_steps == full_work(n)
    assert abs(res.mean_variance * n - n * 0.04) <= n * 2.0 ** -53 * (n * 0.04)


def _heston_enqueue(ctx, surface, sim, stats):
    opt = capi.make_option(S0=100.0, K=100.0, r=R, T=T_, v=NAN, B=NAN)
    ctx.price_heston_enqueue(opt, sim, capi.make_heston(capi.PAYOFF_CALL, 0.01), stats)


def _heston_row(res, n):
    return [res.sum, res.sumsq, res.truncated_steps, None, 0.0, float(n)]


CLIQUET_FLOOR, CLIQUET_CAP = -0.1, 0.15


def _cliquet_terms():
    return capi.make_cliquet(capi.CLIQUET_SUM, 1, 1, global_floor=CLIQUET_FLOOR, global_cap=CLIQUET_CAP, q=0.01)


def _cliquet(ctx, surface, sim, y):
    return ctx.price_cliquet(capi.make_option(S0=100.0, r=R, T=T_, v=NAN, K=NAN, B=NAN), sim, _cliquet_terms(), surface, y)


def _cliquet_counters(res, y, n):
    assert res.n_floored == int((y == CLIQUET_FLOOR).sum()) > 0 and res.n_capped == int((y == CLIQUET_CAP).sum()) > 0
    assert res.work_steps == full_work(n)


def _cliquet_enqueue(ctx, surface, sim, stats):
    ctx.price_cliquet_enqueue(capi.make_option(S0=100.0, r=R, T=T_, v=NAN, K=NAN, B=NAN), sim, _cliquet_terms(), surface, stats)


def _cliquet_row(res, n):
    return [res.sum, res.sumsq, float(res.n_floored), float(res.n_capped), 0.0, float(n)]


def _asian_terms():
    return capi.make_asian(capi.ASIAN_ARITHMETIC, capi.ASIAN_FIXED, capi.PAYOFF_PUT, 1, capi.ASIAN_CONTROL_GEOMETRIC)


def _asian(ctx, surface, sim, y):
    return ctx.price_asian(capi.make_option(S0=100.0, K=101.0, r=R, T=T_, v=0.2), sim, _asian_terms(), y)


def _asian_counters(res, y, n):
    assert res.work_steps == full_work(n) and res.live_steps == 0.0 and res.sum_cc > 0.0


def _asian_enqueue(ctx, surface, sim, stats):
    ctx.price_asian_enqueue(capi.make_option(S0=100.0, K=101.0, r=R, T=T_, v=0.2), sim, _asian_terms(), stats)


def _asian_row(res, n):
    return [res.sum, res.sumsq, res.sum_c, res.sum_cc, res.sum_yc, float(n)]


def _autocall_terms():
    return capi.make_autocall([0.2, 0.3], [[1.0, 0.5], [0.5, 1.0]], 1, 1.0, 0.05, 0.8, capi.AUTOCALL_KI_AT_MATURITY)


def _autocall(ctx, surface, sim, y):
    return ctx.price_autocall(capi.make_option(S0=0.0, v=0.0, K=0.0, r=R, T=T_), sim, _autocall_terms(), y)


def _autocall_counters(res, y, n):
    # called: 1 + coupon; not called and the worst below the knock-in level: the worst itself (< 0.8); else 1
    called, knocked = int((y > 1.0).sum()), int((y < 0.8).sum())
    assert res.n_called == called > 0 and res.n_knocked_in == knocked > 0 and called + knocked < n
    assert res.sum_t_call == called * T_ and res.work_steps == full_work(n) and res.live_steps == n


def _autocall_enqueue(ctx, surface, sim, stats):
    ctx.price_autocall_enqueue(capi.make_option(S0=0.0, v=0.0, K=0.0, r=R, T=T_), sim, _autocall_terms(), stats)


def _autocall_row(res, n):
    return [res.sum, res.sumsq, float(res.n_called), res.sum_t_call, float(res.n_knocked_in), float(n)]


PUBLIC = {"heston-4": (_heston, _heston_counters, _heston_enqueue, _heston_row),
          "cliquet-5": (_cliquet, _cliquet_counters, _cliquet_enqueue, _cliquet_row),
          "asian-6": (_asian, _asian_counters, _asian_enqueue, _asian_row),
          "autocall-7": (_autocall, _autocall_counters, _autocall_enqueue, _autocall_row)}


def priced(ctx, surface, call, n, seed):
    y = torch.full((n,), NAN, dtype=torch.float64, device="cuda")
    res = call(ctx, surface, capi.make_sim(n + 5, 1, capi.F64, seed=seed, path_offset=5, n_paths_local=n), y)
    torch.cuda.synchronize()
    return res, host(y)


@pytest.mark.parametrize("product", list(PUBLIC))
def test_public_call_sums_are_the_samples_sums(ctx, surface, product, record_property):
    call, counters, _, _ = PUBLIC[product]
    worst = 0.0
    for n, grid in [(paths_of(g), g) for g in PUBLIC_GRIDS] + [(STRIDED, 8192)]:
        res, y = priced(ctx, surface, call, n, 11 + grid)
        assert np.isfinite(y).all() and (res.n, res.grid, res.block) == (n, grid, 256)
        # the kernel adds y and fma(y, y, .): against math.fsum of y and of the ROUNDED squares the bound holds with the
        # squares' own rounding (2^-53 each) inside it: (n - 1) + 1 roundings of at most 2^-53 sum y^2
        for got, terms in ((res.sum, y), (res.sumsq, y * y)):
            exact, bound = math.fsum(terms), n * 2.0 ** -53 * math.fsum(np.abs(terms))
            worst = max(worst, abs(got - exact) / bound)
            assert abs(got - exact) <= bound, (product, n, got, exact, bound)
        counters(res, y, n)
    record_property("largest_error_over_bound", worst)
    print(f"{product}: sum and sumsq at {len(PUBLIC_GRIDS) + 1} path counts, largest error {worst:.3g} of the bound")


@pytest.mark.parametrize("grid", [257, 8192])
@pytest.mark.parametrize("product", list(PUBLIC))
def test_two_enqueued_jobs_keep_their_own_records(ctx, surface, product, grid):
    call, _, enqueue, row = PUBLIC[product]
    n = paths_of(grid)
    sims = [capi.make_sim(n + 5, 1, capi.F64, seed=seed, path_offset=5, n_paths_local=n) for seed in (21, 22)]
    stats = poisoned(2, 6)
    for r, sim in enumerate(sims):
        enqueue(ctx, surface, sim, stats[r])
    torch.cuda.synchronize()
    got = host(stats)
    for r, sim in enumerate(sims):
        res = call(ctx, surface, sim, None)
        torch.cuda.synchronize()
        want = row(res, n)
        for k, w in enumerate(want):
            assert w is None or got[r, k] == w, (product, grid, r, k, got[r].tolist(), want)
    assert got[0, 0] != got[1, 0]
