"""GPU tests of the wave-uniform Philox head in the path loops (csrc/mc_device.hpp: philox_hi_uniform, PhiloxLane,
PhiloxHead, philox_block_uniform).  Run with -m gpu on an MI355X.

A wavefront whose path ids share one high word computes the head of every Philox block on the scalar unit; the one
wavefront per 2^32 paths that straddles a multiple of 2^32 walks the ten plain rounds.  Both must draw the same words,
so a path's sample does not depend on which wavefront it ran in.  A path is looked at through a shard of one
(n_paths_local = 1): its record's sum is the path's sample and sumsq its square.

  * the straddling shard (test_straddling_shard_sums_its_paths): 300 paths from id 2^32 - 101 — an odd offset, so one
    pair-sum thread owns ids 2^32 - 1 and 2^32 — against the fp64 sum of its 300 single-path records.  The samples are
    bit-identical and only the order of the summation differs: 1e-13 relative on both sums, several hundred times the
    rounding of a 300-term fp64 sum and ten orders of magnitude below what one wrong Philox word does to a sample;
  * the eight ids 2^32 - 4 .. 2^32 + 3 one by one (test_the_eight_ids_around_the_boundary): differences of consecutive
    records of shards of 1 .. 8 paths against the single-path records.  A difference of two rounded sums is the sample
    only up to their rounding (each record is at most three additions away from exact, the subtraction one more:
    4 ulp of the larger record is allowed, 9e-16 relative); what CAN be exact is asserted with ==: a shard of two paths
    is one addition, so its sum is the rounded sum of the two single-path samples — for every pair of neighbours,
    the pair (2^32 - 1, 2^32) that one thread owns included.  The eight samples are also compared with the numpy
    restatement, at the tolerance below;
  * stored trajectories (test_stored_trajectories_of_the_straddling_shard): every element of the shard's buffer equals
    (==) the element the single-path shards store, both layouts;
  * ordinary and deep uniform ids against the numpy restatement of tests/greeks_restate.py
    (test_uniform_ids_restate): 256 paths from id 5003 under seed 77 and from id 2^33 + 5003 of a 2^40-path job under
    seed 2^40 + 77 (tests/deep_inputs.py).  Tolerance: the per-path tolerance of the pathwise price sample of
    tests/greeks_cases.py — the same kernel loop, the same restatement, nothing new;
  * launch remainders (test_launch_remainders_across_the_boundary): shards of 1 .. 513 paths from id 2^32 - 64 at two
    steps against their single-path records, 1e-13 relative as above."""
import importlib
import math

import numpy as np
import pytest

import greeks_cases as gc
from deep_inputs import DEEP, SHALLOW
from greeks_restate import restate

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

PRECS = (capi.F64, capi.F32)
TORCH_T = {capi.F64: torch.float64, capi.F32: torch.float32}
BENCH = dict(S0=100.0, T=1.0, K=100.0, r=0.1, v=0.2)
TWO32 = 2 ** 32
JOB, SEED = 2 ** 33, 2 ** 40 + 77
FIRST, N_SHARD = TWO32 - 101, 300
STEPS = (1, 2, 3, 4, 5, 8, 252)


def window_of(n_steps):
    """the window jobs: B = 120, [1, 4] at 8 steps, the benchmark's bullet window [10, 50] at 252"""
    return dict(B=120.0, use_window=1, **({8: dict(P1=1, P2=4), 252: dict(P1=10, P2=50)}[n_steps]))


# form -> (option overrides of n_steps, flags); "window-all" is a window no path leaves, so that every sample counts
FORMS = {
    "default": (lambda n: {}, 0),
    "product": (lambda n: {}, capi.FLAG_PRODUCT_FORM),
    "window": (window_of, 0),
    "window-product": (window_of, capi.FLAG_PRODUCT_FORM),
    "window-all": (lambda n: dict(B=120.0, use_window=1, P1=0, P2=n), 0),
}
SHARD_CASES = [(f, n) for f in ("default", "product") for n in STEPS] + [
    (f, n) for f in ("window", "window-product", "window-all") for n in (8, 252)]


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


def option(form, n_steps):
    return capi.make_option(**dict(BENCH, **FORMS[form][0](n_steps)))


def shard(ctx, prec, form, n_steps, first, n, seed=SEED, job=JOB):
    """(sum, sumsq) of the shard of n paths from id `first`"""
    res = ctx.price_paths(option(form, n_steps), capi.make_sim(job, n_steps, prec, seed=seed, path_offset=first,
                                                             n_paths_local=n, flags=FORMS[form][1]))
    assert res.n == n
    return res.sum, res.sumsq


_singles = {}


def singles(ctx, prec, form, n_steps, first, n, seed=SEED, job=JOB):
    """[n, 2] (sample, its square) of the paths first .. first + n - 1, each priced as a shard of one; computed once"""
    key = (prec, form, n_steps, first, n, seed, job)
    if key not in _singles:
        stats = torch.zeros(n, 6, dtype=torch.float64, device="cuda")
        opt = option(form, n_steps)
        for i in range(n):
            ctx.price_paths_enqueue(opt, capi.make_sim(job, n_steps, prec, seed=seed, path_offset=first + i,
                                                       n_paths_local=1, flags=FORMS[form][1]), stats[i])
        rec = stats.cpu().numpy()
        assert np.isfinite(rec).all() and (rec[:, 5] == 1).all()
        rec = rec[:, :2].copy()
        rec.setflags(write=False)
        _singles[key] = rec
    return _singles[key]


def assert_sums(got, rec, what):
    want = math.fsum(rec[:, 0]), math.fsum(rec[:, 1])
    print(f"{what}: {np.count_nonzero(rec[:, 0])} of {len(rec)} samples pay; relative deviation of (sum, sumsq) "
          f"{[abs(g - w) / w if w else abs(g) for g, w in zip(got, want)]}")
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-13 * abs(w), (what, got, want)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("form,n_steps", SHARD_CASES)
def test_straddling_shard_sums_its_paths(ctx, prec, form, n_steps):
    rec = singles(ctx, prec, form, n_steps, FIRST, N_SHARD)
    if form in ("default", "product", "window-all"):
        assert np.count_nonzero(rec[:, 0]) > N_SHARD // 4      # an at-the-money call: the sums are not sums of zeros
    assert_sums(shard(ctx, prec, form, n_steps, FIRST, N_SHARD), rec, f"{form} {n_steps} steps f{prec}")


EIGHT = TWO32 - 4


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("form,n_steps", [("default", 1), ("default", 5), ("default", 8), ("product", 5),
                                          ("window-all", 8)])
def test_the_eight_ids_around_the_boundary(ctx, oracle, prec, form, n_steps):
    one = singles(ctx, prec, form, n_steps, FIRST, N_SHARD)[EIGHT - FIRST:EIGHT - FIRST + 8]
    assert np.count_nonzero(one[:, 0]) >= 2
    recs = [(0.0, 0.0)] + [shard(ctx, prec, form, n_steps, EIGHT, m) for m in range(1, 9)]
    assert recs[1] == tuple(one[0])                      # the shard of one IS the single-path record
    for m in range(1, 9):
        for k in (0, 1):
            diff, bound = recs[m][k] - recs[m - 1][k], 4 * np.spacing(recs[m][k])
            assert abs(diff - one[m - 1, k]) <= bound, (m, k, diff, one[m - 1, k])
    for i in range(7):                                   # two paths: one addition, exact
        s, s2 = shard(ctx, prec, form, n_steps, EIGHT + i, 2)
        assert s == one[i, 0] + one[i + 1, 0], (i, s, one[i:i + 2, 0])
        assert abs(s2 - (one[i, 1] + one[i + 1, 1])) <= 2 * np.spacing(s2)
    if form == "default":                                # and they are the restated samples
        sim = capi.make_sim(JOB, n_steps, prec, seed=SEED, path_offset=EIGHT, n_paths_local=8)
        want = restate(oracle, option(form, n_steps), sim, gc.PW).q
        tol = gc.tolerance(prec, gc.PW, want)[:, 0]
        assert (np.abs(one[:, 0] - want[:, 0]) <= tol).all(), (one[:, 0], want[:, 0], tol)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n_steps", [5, 8])
def test_stored_trajectories_of_the_straddling_shard(ctx, prec, n_steps):
    opt, dt = capi.make_option(**BENCH), TORCH_T[prec]
    sim = lambda first, n: capi.make_sim(JOB, n_steps, prec, seed=SEED, path_offset=first, n_paths_local=n)
    alone = torch.zeros(N_SHARD, n_steps, dtype=dt, device="cuda")
    alone_pay = torch.zeros(N_SHARD, 4, dtype=dt, device="cuda")   # a row of its own per path, 16-byte aligned
    stats = torch.zeros(6, dtype=torch.float64, device="cuda")
    for i in range(N_SHARD):
        ctx.simulate_trajectories_enqueue(opt, sim(FIRST + i, 1), alone[i], None, alone_pay[i], stats)
    alone, alone_pay = alone.cpu().numpy(), alone_pay.cpu().numpy()[:, 0]
    assert np.isfinite(alone).all() and (alone > 0).all() and np.count_nonzero(alone_pay) > N_SHARD // 4
    for layout in (capi.STEP_MAJOR, capi.PATH_MAJOR):
        traj = torch.zeros(N_SHARD * n_steps, dtype=dt, device="cuda")
        pay = torch.zeros(N_SHARD, dtype=dt, device="cuda")
        res = ctx.simulate_trajectories(opt, sim(FIRST, N_SHARD), traj, None, pay, layout)
        assert res.n == N_SHARD
        got = traj.cpu().numpy()
        got = got.reshape(n_steps, N_SHARD).T if layout == capi.STEP_MAJOR else got.reshape(N_SHARD, n_steps)
        assert (got == alone).all(), (layout, np.argwhere(got != alone)[:8])
        assert (pay.cpu().numpy() == alone_pay).all(), layout


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("where", [SHALLOW, DEEP], ids=["ordinary", "deep"])
@pytest.mark.parametrize("n_steps", [1, 2, 7])
def test_uniform_ids_restate(ctx, oracle, prec, where, n_steps):
    seed, first, job = where
    n = gc.N_PATHS
    opt = capi.make_option(**BENCH)
    sim = capi.make_sim(max(job, first + n), n_steps, prec, seed=seed, path_offset=first, n_paths_local=n)
    want = restate(oracle, opt, sim, gc.PW).q
    tol = gc.tolerance(prec, gc.PW, want)[:, 0]
    want = want[:, 0]
    one = singles(ctx, prec, "default", n_steps, first, n, seed, sim.n_paths)
    err = np.abs(one[:, 0] - want)
    print(f"f{prec} {n_steps} steps from id {first}: largest share of the tolerance {(err / tol).max():.3f}")
    assert (err <= tol).all(), np.argwhere(err > tol)[:8]
    assert np.allclose(one[:, 1], one[:, 0] ** 2, rtol=1e-15, atol=0.0)
    got = shard(ctx, prec, "default", n_steps, first, n, seed, sim.n_paths)
    assert abs(got[0] - want.sum()) <= tol.sum()
    assert_sums(got, one, f"f{prec} {n_steps} steps, 256 paths from id {first}")


REMAINDERS = (1, 63, 64, 65, 127, 128, 129, 513)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("form", ["default", "product"])
def test_launch_remainders_across_the_boundary(ctx, prec, form):
    first = TWO32 - 64
    rec = singles(ctx, prec, form, 2, first, max(REMAINDERS))
    for m in REMAINDERS:
        assert_sums(shard(ctx, prec, form, 2, first, m), rec[:m], f"{form} f{prec} {m} paths from 2^32 - 64")
