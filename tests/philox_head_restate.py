"""numpy restatement of the two ways the kernels compute a Philox4x32-10 block in a step loop (csrc/mc_device.hpp), used
by tests/test_philox_head_cpu.py.  No kernel runs here.

  * plain(): the ten rounds of philox4x32_10 on the counter (block_lo, block_hi, sub_lo, sub_hi);
  * lane(), head(), block_uniform(): PhiloxLane::make, PhiloxHead::make and philox_block_uniform — the lane constants
    of a path id's low word, the three scalars of (sub_hi, k), and rounds 3 to 10 on both.  The counter they stand for
    is (k, 0, sub_lo, sub_hi).
Everything is uint64 arithmetic masked to 32 bits, elementwise over arrays."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
SH = np.uint64(32)


def u(x):
    return np.asarray(x, dtype=np.uint64) & MASK


def keys(seed):
    """(k0[10], k1[10]) of the seed(s): uint64 arrays of 32-bit values, round i at index i"""
    seed = np.asarray(seed, dtype=np.uint64)
    a, b = seed & MASK, seed >> SH
    k0 = [(a + np.uint64(i * W0 % 2 ** 32)) & MASK for i in range(10)]
    k1 = [(b + np.uint64(i * W1 % 2 ** 32)) & MASK for i in range(10)]
    return k0, k1


def _round(c, k0, k1):
    c0, c1, c2, c3 = c
    p0, p1 = M0 * c0, M1 * c2
    return ((p1 >> SH) ^ c1 ^ k0, p1 & MASK, (p0 >> SH) ^ c3 ^ k1, p0 & MASK)


def plain(seed, subsequence, block):
    """[4, ...] words of philox_block(key(seed), subsequence, block)"""
    k0, k1 = keys(seed)
    subsequence, block = np.asarray(subsequence, dtype=np.uint64), np.asarray(block, dtype=np.uint64)
    c = (block & MASK, block >> SH, subsequence & MASK, subsequence >> SH)
    for i in range(10):
        c = _round(c, k0[i], k1[i])
    return np.stack(np.broadcast_arrays(*c))


def lane(seed, sub_lo):
    """(x0, x2, c3) of PhiloxLane::make"""
    k0, k1 = keys(seed)
    p1 = M1 * u(sub_lo)
    p0 = M0 * ((p1 >> SH) ^ k0[0])
    return (p1 & MASK) ^ k0[1], (p0 >> SH) ^ k1[1], p0 & MASK


def head(seed, sub_hi, k):
    """(s0, s2, s3) of PhiloxHead::make"""
    k0, k1 = keys(seed)
    pk = M0 * u(k)
    c2 = (pk >> SH) ^ k1[0] ^ u(sub_hi)
    p1 = M1 * c2
    return p1 >> SH, pk & MASK, (p1 & MASK) ^ k0[2]


def block_uniform(seed, ln, hd):
    """[4, ...] words of philox_block_uniform"""
    k0, k1 = keys(seed)
    x0, x2, c3 = ln
    s0, s2, s3 = hd
    p0, p1 = M0 * (x0 ^ s0), M1 * (x2 ^ s2)
    c = ((p1 >> SH) ^ s3, p1 & MASK, (p0 >> SH) ^ c3 ^ k1[2], p0 & MASK)
    for i in range(3, 10):
        c = _round(c, k0[i], k1[i])
    return np.stack(np.broadcast_arrays(*c))


def with_head(seed, subsequence, k):
    """plain(seed, subsequence, k) through lane(), head() and block_uniform(); k below 2^32"""
    subsequence = np.asarray(subsequence, dtype=np.uint64)
    return block_uniform(seed, lane(seed, subsequence & MASK), head(seed, subsequence >> SH, k))
