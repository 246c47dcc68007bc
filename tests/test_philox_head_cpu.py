"""The wave-uniform Philox head (csrc/mc_device.hpp: PhiloxLane, PhiloxHead, philox_block_uniform) without a device:
its numpy restatement (tests/philox_head_restate.py) gives the four words of the ten plain rounds, and those are the
oracle's rocRAND-exact words.  The kernels themselves are compared in tests/test_gpu_philox_head.py."""
import numpy as np
import pytest

import philox_head_restate as ph


def random_inputs(n, rng):
    seed = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    sub = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    k = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    return seed, sub, k


def test_head_gives_the_words_of_the_ten_plain_rounds():
    rng = np.random.default_rng(20)
    seed, sub, k = random_inputs(20_000, rng)
    assert (sub >> np.uint64(32)).min() > 0           # high words of the subsequence that are not zero
    assert (ph.with_head(seed, sub, k) == ph.plain(seed, sub, k)).all()


@pytest.mark.parametrize("seed", [0, 77, 2 ** 40 + 77, 2 ** 64 - 1])
def test_head_at_the_edges_of_its_inputs(seed):
    edge32 = [0, 1, 2, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]
    sub = np.array([(hi << 32) | lo for hi in edge32 for lo in edge32], dtype=np.uint64)
    for k in edge32 + [126, 63]:
        assert (ph.with_head(seed, sub, k) == ph.plain(seed, sub, k)).all(), k


def test_head_is_shared_by_the_lanes_of_a_wavefront():
    """what the kernels rely on: the three scalars depend on (seed, sub_hi, k) alone, the lane constants on
    (seed, sub_lo) alone — 64 consecutive ids under one high word, walked over consecutive blocks"""
    seed, first = 2 ** 40 + 77, 2 ** 33 + 5003
    ids = np.arange(first, first + 64, dtype=np.uint64)
    ln = ph.lane(seed, ids & ph.MASK)
    for k in range(5):
        hd = ph.head(seed, first >> 32, k)
        assert all(np.ndim(s) == 0 for s in hd)
        assert (ph.block_uniform(seed, ln, hd) == ph.plain(seed, ids, k)).all()


def test_plain_rounds_are_the_oracles(oracle):
    rng = np.random.default_rng(21)
    seed, sub, k = random_inputs(200, rng)
    got = ph.plain(seed, sub, k)
    uni = ph.with_head(seed, sub, k)
    for i in range(len(seed)):
        want = oracle.philox(int(seed[i]), int(sub[i]), int(k[i]))
        assert (got[:, i] == want).all() and (uni[:, i] == want).all(), (seed[i], sub[i], k[i])

