"""The order in which a grid's records are added (csrc/mc_device.hpp wave_sum, block_sumN, small_final_sum; csrc/aux.hip
final_reduce_kernel; csrc/smile.hip smile_finish_kernel), restated in numpy float64 from the code's comments and loops:
every `+` below is one fp64 addition of the kernel, in the kernel's order, so the results are the kernel's bits.  No
kernel runs here; tests/test_finish_cpu.py checks the restatement, tests/test_gpu_finish.py holds the kernels to it.

Every instantiated (record width N, accumulator sets ACC) of grid_finish / finish_paths / small_final_sum in csrc/:
  (2, 4)   price_impl.hpp (plain and window kernels), american_dual.hip (continuation), aux.hip small_final_kernel<2>
  (4, 4)   barrier, lookback, basket, localvol, heston, american_dual (scan)
  (5, 4)   price_impl.hpp (control variate), cliquet, american (pricing), aux.hip small_final_kernel<5>
  (6, 4)   asian, heston_cliquet, heston_barrier, autocall / autocall_localvol (statistics layout)
  (7, 4)   autocall, autocall_localvol
  (12, 4)  american (sweep), greeks (both kernels; their statistics record is 16 doubles, its sum 12)
  (28, 1)  localvol_greeks
block_sumN<256, N> also runs at N = 3 (nmc.hip, american_dual.hip) and block_sumN<1024, N> at N = 2, 4, 5
(final_reduce_kernel)."""
import numpy as np

WAVE = 64
INSTANTIATED = ((2, 4), (4, 4), (5, 4), (6, 4), (7, 4), (12, 4), (28, 1))
BLOCK_SUM_WIDTHS = (2, 3, 4, 5, 6, 7, 12, 28)      # block_sumN<256, N>
FINAL_WIDTHS = (2, 4, 5)                           # final_reduce_kernel<N>, block_sumN<1024, N>
FINAL_BLOCK = 1024


def shfl_down(v, off):
    """__shfl_down(v, off, 64) along axis 0 of v [64, ...]: lane l reads lane l + off, its own value beyond the wave"""
    return np.concatenate([v[off:], v[WAVE - off:]])


def wave_sum(v):
    """v [64, ...] -> lane 0 of six shfl_down rounds (offsets 32, 16, .. 1)"""
    v = np.array(v, dtype=np.float64)
    assert v.shape[0] == WAVE
    off = WAVE // 2
    while off > 0:
        v = v + shfl_down(v, off)
        off >>= 1
    return v[0]


def block_sum(v):
    """block_sumN<BLOCK, N> (and block_sum2<BLOCK>): v [BLOCK, N] -> thread 0's [N].  A wave tree per wavefront, one LDS
    slot per wave, lanes >= kWaves hold 0, log2(kWaves) more shfl_down rounds."""
    v = np.asarray(v, dtype=np.float64)
    block = v.shape[0]
    n_waves = block // WAVE
    assert block % WAVE == 0 and n_waves & (n_waves - 1) == 0
    slots = np.stack([wave_sum(v[w * WAVE:(w + 1) * WAVE]) for w in range(n_waves)])
    if n_waves == 1:
        return slots[0]
    lanes = np.zeros((WAVE,) + v.shape[1:])
    lanes[:n_waves] = slots
    off = n_waves // 2
    while off > 0:
        lanes = lanes + shfl_down(lanes, off)
        off >>= 1
    return lanes[0]


def small_final_sum(rec, block=256, acc=4):
    """small_final_sum<BLOCK, N, ACC>: rec [n, N] -> [N].  Record i goes to thread i % BLOCK, set (i / BLOCK) % ACC, a
    thread's records in rising i; the sets are added pairwise in the code's loop order (w = 1, 2, ..: s[u] += s[u + w] for
    u = 0, 2 w, ..); block_sumN finishes."""
    rec = np.asarray(rec, dtype=np.float64)
    n, width = rec.shape
    s = np.zeros((acc, block, width))
    for sweep in range((n + block - 1) // block):
        chunk = rec[sweep * block:(sweep + 1) * block]
        s[sweep % acc, :chunk.shape[0]] += chunk
    w = 1
    while w < acc:
        for u in range(0, acc - w, 2 * w):
            s[u] = s[u] + s[u + w]
        w *= 2
    return block_sum(s[0])


def final_reduce(rec):
    """final_reduce_kernel<N>: rec [n, N] -> [N].  Thread t of 1024 walks i = t, t + 4096, .. while i + 3072 < n and adds
    records i + 1024 u to set u = 0..3; its remainder (i, i + 1024, .. < n) goes to set 0; then (s0 + s1) + (s2 + s3);
    then block_sumN<1024, N>."""
    rec = np.asarray(rec, dtype=np.float64)
    n, width = rec.shape
    B = FINAL_BLOCK
    t = np.arange(B)
    s = np.zeros((4, B, width))
    i = t.copy()
    while True:
        full = i + 3 * B < n
        if not full.any():
            break
        for u in range(4):
            s[u, full] += rec[i[full] + u * B]
        i[full] += 4 * B
    while True:
        left = i < n
        if not left.any():
            break
        s[0, left] += rec[i[left]]
        i[left] += B
    return block_sum((s[0] + s[1]) + (s[2] + s[3]))


def smile_finish(entries, n_waves, n_nodes):
    """smile_finish_kernel: entries [>= n_waves n_nodes, 2] (sum, sumsq) -> out [2 n_nodes]: a node's entries over the
    wavefronts in wave order, the sums first, then the sums of squares"""
    e = np.asarray(entries, dtype=np.float64)[:n_waves * n_nodes].reshape(n_waves, n_nodes, 2)
    out = np.zeros((n_nodes, 2))
    for w in range(n_waves):
        out = out + e[w]
    return np.concatenate([out[:, 0], out[:, 1]])


def front_to_back(rec):
    """the plain loop over the records, first to last: what the orders above are NOT"""
    rec = np.asarray(rec, dtype=np.float64)
    out = np.zeros(rec.shape[1])
    for r in rec:
        out = out + r
    return out


# ---------------- the two kinds of data ----------------
SEED = 20261021


def integers(n, width, first=0):
    """record i, slot k holds (i + 1)(k + 1): exact in fp64, and a dropped, doubled or misplaced record changes slot 0
    by the record's number"""
    return np.outer(np.arange(first, first + n, dtype=np.float64) + 1.0, np.arange(width, dtype=np.float64) + 1.0)


def integer_sum(n, width):
    return (n * (n + 1) // 2) * (np.arange(width, dtype=np.float64) + 1.0)


def wide_floats(n, width, seed=SEED):
    """normals scaled by 2^e, e uniform in [-20, 20)"""
    r = np.random.default_rng(seed)
    return r.standard_normal((n, width)) * np.exp2(r.integers(-20, 20, size=(n, width)).astype(np.float64))


def fsum_bound(rec):
    """(exact [N], bound [N]): math.fsum of each slot and n 2^-53 sum |x|, the worst case of any summation order (each
    of the n - 1 additions rounds by at most 2^-53 of a partial sum no larger than sum |x|)"""
    import math
    rec = np.asarray(rec, dtype=np.float64)
    exact = np.array([math.fsum(rec[:, k]) for k in range(rec.shape[1])])
    bound = rec.shape[0] * 2.0 ** -53 * np.array([math.fsum(np.abs(rec[:, k])) for k in range(rec.shape[1])])
    return exact, bound


def prefix_fsums(rec):
    """(exact [n + 1, N], sum_abs [n + 1, N]): row m holds math.fsum of the first m records of each slot, and of their
    absolute values — computed once for every m.  The values are scaled by 2^200 to integers (exactly, which is asserted),
    added as Python integers and divided back by one correctly rounded division, which is what math.fsum returns."""
    import itertools
    rec = np.asarray(rec, dtype=np.float64)
    scaled = rec * 2.0 ** 200
    assert np.all(np.isfinite(scaled)) and np.all(np.mod(scaled, 1.0) == 0.0)
    one = 1 << 200
    exact, sum_abs = np.zeros((rec.shape[0] + 1, rec.shape[1])), np.zeros((rec.shape[0] + 1, rec.shape[1]))
    for k in range(rec.shape[1]):
        ints = [int(x) for x in scaled[:, k].tolist()]
        exact[1:, k] = [s / one for s in itertools.accumulate(ints)]
        sum_abs[1:, k] = [s / one for s in itertools.accumulate(abs(x) for x in ints)]
    return exact, sum_abs


# record counts where small_final_sum changes branch (256 m +- 1 partial sweeps, 1024 m +- 1 full ones), with both ends
SMALL_COUNTS = tuple(range(0, 1101)) + (2047, 2048, 2049, 3071, 3072, 3073, 4095, 4096, 4097, 8191, 8192)
CPU_COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1279, 1281,
              2047, 2048, 2049, 3071, 3072, 3073, 4095, 4096, 4097, 8191, 8192)
FINAL_COUNTS = (1, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, 4095, 4096, 4097, 5119, 5120, 5121,
                8191, 8192, 8193, 16384, 16385, 2 ** 20 - 1, 2 ** 20)
SMILE_NODES = (1, 63, 64, 255, 256, 257, 2048)
SMILE_WAVES = (1, 7, 8, 9, 16, 17, 2048)
