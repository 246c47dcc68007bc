"""Where the elementwise GPU tests of the barrier, lookback, basket and Asian pricers draw their paths: (seed, first
global path id, paths of the job), shared so that the four modules cannot drift apart.

SHALLOW is the shard every module's test 1 started from.  DEEP is a shard far into a job of 2^40 paths under a seed
beyond 32 bits: its low words are SHALLOW's, so a kernel that dropped the high word of the path id, of the seed or of
both would draw the numbers of (DEEP_SEED, 5003 + p), (77, 2^33 + 5003 + p) or (77, 5003 + p) instead of the
restatement's.  check_deep_draws_differ shows that this cannot go unnoticed."""
import numpy as np

N_JOB, OFFSET, SEED = 20_000, 5003, 77
DEEP_JOB, DEEP_OFFSET, DEEP_SEED = 2 ** 40, 2 ** 33 + 5003, 2 ** 40 + 77
SHALLOW, DEEP = (SEED, OFFSET, N_JOB), (DEEP_SEED, DEEP_OFFSET, DEEP_JOB)


def check_deep_draws_differ(draw):
    """draw(seed, first) -> one array, or a tuple of arrays, of what some paths first.. draw under seed.  No number of
    the deep draws may be that of the same path, step and slot of a stream a dropped high word lands on."""
    as_tuple = lambda a: a if isinstance(a, tuple) else (a,)
    deep = as_tuple(draw(DEEP_SEED, DEEP_OFFSET))
    assert all(np.isfinite(a).all() and a.std() > 0.1 for a in deep)
    for seed, first in ((SEED, OFFSET), (DEEP_SEED, OFFSET), (SEED, DEEP_OFFSET)):
        assert seed % 2 ** 32 == DEEP_SEED % 2 ** 32 and first % 2 ** 32 == DEEP_OFFSET % 2 ** 32
        for a, b in zip(as_tuple(draw(seed, first)), deep):
            assert a.shape == b.shape and not (a == b).any(), (seed, first)
