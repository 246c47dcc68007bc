"""CPU checks of the record finish's tests: the harness (tests/finish_check.hip, run on the GPU by
tests/test_gpu_finish.py) must compile for gfx950 with the library's own flags and link against the built library, and
the restatement of the summation order (tests/finish_restate.py) must be a sum, and not the plain one.

Three properties of the restated small_final_sum, for every (N, ACC) the library instantiates — (2, 4), (4, 4), (5, 4),
(6, 4), (7, 4), (12, 4), (28, 1), enumerated from the grid_finish<, finish_paths and small_final_sum< calls in csrc/ (file
by file in finish_restate's docstring) — at both block sizes (256 and 1024) and the record counts finish_restate.CPU_COUNTS
(0, 1, 2, and 64 m, 256 m, 1024 m and their neighbours up to 8192):
  * on integer records it equals the integer sum;
  * on wide floats (normals scaled by 2^[-20, 20)) it stays within n 2^-53 sum |x| of math.fsum;
  * at least half of the wide-float sums of each (N, ACC, block) differ in bits from the front-to-back sum: the
    condition under which bit-equality with the restatement on the GPU says anything about the order.
The first two also hold final_reduce (widths 2, 4, 5) and smile_finish to account at their GPU cases' sizes."""
import importlib
import os

import numpy as np
import pytest

import finish_harness as fh
import finish_restate as fr


def test_harness_compiles_and_links_against_the_library(tmp_path):
    pkg = importlib.import_module("monte-carlo-project-cuda_amd")
    if not os.path.exists(pkg.capi.LIB_PATH):
        pkg.build()
    L = fh.load(fh.compile_harness(tmp_path))
    for name in ("fc_block_sum", "fc_small_final_sum", "fc_handoff", "fc_write_final", "fc_library_sum", "fc_smile_finish"):
        assert getattr(L, name) is not None


def test_wave_and_block_sums_are_sums_in_tree_order():
    v = fr.integers(1024, 3)
    assert np.array_equal(fr.wave_sum(v[:64]), fr.integer_sum(64, 3))
    for block in (64, 256, 1024):
        assert np.array_equal(fr.block_sum(v[:block]), fr.integer_sum(block, 3))
    # a one-hot lane arrives unchanged, whichever lane
    x = fr.wide_floats(1024, 1)[:, 0]
    for block in (256, 1024):
        assert np.array_equal(fr.block_sum(np.diag(x[:block])), x[:block])
    # lane 0 of the wave tree: ((v0 + v32) + (v16 + v48)) + ... : pinned on four lanes that no other order adds alike
    w = np.zeros((64, 1))
    w[[0, 16, 32, 48], 0] = [1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53]
    assert fr.wave_sum(w)[0] == (1.0 + 2.0 ** -53) + (2.0 ** -53 + 2.0 ** -53) == 1.0 + 2.0 ** -52


def test_prefix_fsums_are_math_fsum():
    import math
    rec = fr.wide_floats(3000, 3)
    exact, sum_abs = fr.prefix_fsums(rec)
    assert not exact[0].any() and not sum_abs[0].any()
    for n in (1, 2, 257, 1024, 3000):
        assert exact[n].tolist() == [math.fsum(rec[:n, k]) for k in range(3)]
        assert sum_abs[n].tolist() == [math.fsum(np.abs(rec[:n, k])) for k in range(3)]
        assert np.array_equal(np.stack([exact[n], n * 2.0 ** -53 * sum_abs[n]]), np.stack(fr.fsum_bound(rec[:n])))


@pytest.fixture(scope="module")
def prefixes():
    """front-to-back sums of every prefix of the wide floats, per width: row n - 1 is the plain sum of n records"""
    out = {}
    for width in sorted({n for n, _ in fr.INSTANTIATED}):
        rec = fr.wide_floats(max(fr.CPU_COUNTS), width)
        run, rows = np.zeros(width), np.empty_like(rec)
        for i, r in enumerate(rec):
            run = run + r
            rows[i] = run
        assert np.array_equal(rows[999], fr.front_to_back(rec[:1000]))
        out[width] = (rec, rows)
    return out


@pytest.mark.parametrize("block", (256, 1024))
@pytest.mark.parametrize("width,acc", fr.INSTANTIATED)
def test_small_final_sum_restated(width, acc, block, prefixes):
    ints = fr.integers(max(fr.CPU_COUNTS), width)
    rec, plain = prefixes[width]
    differ = total = 0
    worst = 0.0
    for n in fr.CPU_COUNTS:
        assert np.array_equal(fr.small_final_sum(ints[:n], block, acc), fr.integer_sum(n, width)), n
        got = fr.small_final_sum(rec[:n], block, acc)
        exact, bound = fr.fsum_bound(rec[:n])
        assert np.all(np.abs(got - exact) <= bound), (n, got - exact, bound)
        if n:
            worst = max(worst, float(np.max(np.abs(got - exact) / bound)))
            differ += int(np.count_nonzero(got != plain[n - 1]))
        total += width
    print(f"N={width} ACC={acc} block={block}: {differ} of {total} sums differ from front-to-back, "
          f"largest error {worst:.3g} of the bound")
    assert 2 * differ >= total, (differ, total)


@pytest.mark.parametrize("width", fr.FINAL_WIDTHS)
def test_final_reduce_restated(width):
    top = 16385
    ints, rec = fr.integers(top, width), fr.wide_floats(top, width)
    differ = total = 0
    for n in [c for c in fr.FINAL_COUNTS if c <= top]:
        assert np.array_equal(fr.final_reduce(ints[:n]), fr.integer_sum(n, width)), n
        got = fr.final_reduce(rec[:n])
        exact, bound = fr.fsum_bound(rec[:n])
        assert np.all(np.abs(got - exact) <= bound), n
        differ += int(np.count_nonzero(got != np.cumsum(rec[:n], axis=0)[-1]))
        total += width
    assert 2 * differ >= total, (differ, total)
    for n in (2 ** 20 - 1, 2 ** 20):
        assert np.array_equal(fr.final_reduce(fr.integers(n, width)), fr.integer_sum(n, width)), n


def test_smile_finish_restated():
    e = np.stack([np.arange(17 * 257) % 1021 + 1.0, (np.arange(17 * 257) % 509 + 1.0) ** 2], axis=1)
    for n_waves, n_nodes in ((1, 1), (7, 63), (9, 64), (17, 257)):
        want = e[:n_waves * n_nodes].reshape(n_waves, n_nodes, 2).sum(axis=0)
        assert np.array_equal(fr.smile_finish(e, n_waves, n_nodes), np.concatenate([want[:, 0], want[:, 1]]))
    w = fr.wide_floats(17 * 257, 2)
    got = fr.smile_finish(w, 17, 257)
    for node in (0, 100, 256):
        assert got[node] == fr.front_to_back(w[node::257][:17])[0] and got[257 + node] == fr.front_to_back(w[node::257][:17])[1]
