"""GPU tests of the fp64 pair-sum loop (csrc/mc_device.hpp pair_sums_of_paths): mcamd_price_paths in fp64, window-less,
default form, against the CPU oracle, at the shapes where a loop that walks two paths per thread, block by block, can go
wrong — whichever way its two chains are laid out against each other (side by side as shipped, or half an iteration
apart as profiles/pairsum_skew_ab.txt tried).

A thread owns two consecutive paths (chains A and B) and a Philox block is two steps, so
  n_steps  1        no whole block: an odd last step alone
           2, 3     one whole block; 3 adds the odd step
           4, 5     two blocks
           6, 7     three
           252, 253 the benchmark's length, and an odd step after 126 blocks
  n_paths  1, 2, 3 (a last thread owning one path), 127, 128, 129 (one wavefront is 128 paths), 511, 512, 513 (a workgroup
           is 512), 1000.
Tolerance: what tests/test_gpu_parity.py uses for this kernel, 1e-11 relative on sum and sumsq (fp64 path error < 1e-12
after 252 steps); the centred control-variate sums cancel and are compared on the scale of their terms, as there.
Bit-for-bit claims (a path's payoff is the same wherever the path sits) are asserted with ==."""
import importlib
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

BENCH = dict(S0=100.0, T=1.0, K=100.0, r=0.1, v=0.2)
ES = 100.0 * math.exp(0.1)
RTOL = 1e-11
STEPS = [1, 2, 3, 4, 5, 6, 7, 252, 253]
PATHS = [1, 2, 3, 127, 128, 129, 511, 512, 513, 1000]
VR = {"plain": 0, "antithetic": capi.FLAG_ANTITHETIC, "control_variate": capi.FLAG_CONTROL_VARIATE,
      "both": capi.FLAG_ANTITHETIC | capi.FLAG_CONTROL_VARIATE}
TWO32 = 1 << 32


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    c = capi.Context(0, stream.cuda_stream)
    yield c
    c.close()
    torch.cuda.set_stream(torch.cuda.default_stream())


def params(oracle, opt, n_total, n_steps, seed):
    return oracle.make_params(S0=opt.S0, T=opt.T, K=opt.K, r=opt.r, v=opt.v, n_paths=n_total, n_steps=n_steps, seed=seed)


def check_against_oracle(ctx, oracle, opt, n_total, n_steps, seed, flags, lo, n_local):
    sim = capi.make_sim(n_total, n_steps, capi.F64, seed=seed, flags=flags, path_offset=lo, n_paths_local=n_local)
    res = ctx.price_paths(opt, sim)
    want = oracle.mc_paths_vr(params(oracle, opt, n_total, n_steps, seed), capi.F64, lo, n_local,
                              bool(flags & capi.FLAG_ANTITHETIC), ES)
    print(f"steps {n_steps} paths {n_local} at {lo} flags {flags}: sum {res.sum!r} oracle {want[0]!r} "
          f"rel {abs(res.sum - want[0]) / max(abs(want[0]), 1e-300):.2e}; sumsq rel "
          f"{abs(res.sumsq - want[1]) / max(abs(want[1]), 1e-300):.2e}")
    assert res.n == n_local
    assert math.isclose(res.sum, want[0], rel_tol=RTOL, abs_tol=1e-9), (n_steps, n_local, lo, flags)
    assert math.isclose(res.sumsq, want[1], rel_tol=RTOL, abs_tol=1e-9), (n_steps, n_local, lo, flags)
    if flags & capi.FLAG_CONTROL_VARIATE:
        scale = 20.0 * n_local     # |c| ~ 20 per path: the centred sums cancel
        assert abs(res.sum_c - want[2]) <= RTOL * scale + 1e-6
        assert math.isclose(res.sum_cc, want[3], rel_tol=10 * RTOL, abs_tol=1e-3)
        assert abs(res.sum_yc - want[4]) <= 10 * RTOL * 20.0 * scale + 1e-3
    return res


@pytest.mark.parametrize("vr", list(VR))
@pytest.mark.parametrize("n_steps", STEPS)
def test_every_path_count_and_length_against_the_oracle(ctx, oracle, vr, n_steps):
    opt = capi.make_option(**BENCH)
    for n_paths in PATHS:
        check_against_oracle(ctx, oracle, opt, n_paths, n_steps, 1234, VR[vr], 0, n_paths)


# A wavefront of the pair-sum kernel walks 128 consecutive path ids, two per thread.
@pytest.mark.parametrize("vr", ["plain", "both"])
@pytest.mark.parametrize("n_steps", STEPS)
@pytest.mark.parametrize("lo,n_local", [(TWO32 - 100, 1000),    # the first wavefront's ids straddle 2^32: the rare route
                                        (TWO32 - 101, 1000),    # ... and 2^32 falls between one thread's two paths
                                        (TWO32 - 512, 512),     # the last wavefront ends exactly at 2^32 - 1
                                        (TWO32, 1000)])         # the first wavefront starts at 2^32
def test_path_ids_around_two_to_the_32_against_the_oracle(ctx, oracle, vr, n_steps, lo, n_local):
    check_against_oracle(ctx, oracle, capi.make_option(**BENCH), 1 << 40, n_steps, 9, VR[vr], lo, n_local)


@pytest.mark.parametrize("n_steps", STEPS)
def test_a_path_pays_the_same_bits_wherever_it_sits(ctx, oracle, n_steps):
    """Of 1000 paths, only the one with the highest terminal price is left in the money (the strike is put halfway
    between the two highest), so a job's sum IS that path's payoff, whatever else the job holds — adding zeros is exact.
    The job that holds that path alone (lane 0, chain A), the whole 1000, and windows that shift it to the
    other chain, to another lane and to another wavefront must all return the same bits."""
    n, seed = 1000, 77
    free = capi.make_option(S0=100.0, T=1.0, K=0.0, r=0.1, v=0.2)            # payoff = S_T
    st = oracle.mc_paths(params(oracle, free, n, n_steps, seed), capi.F64, 0, n, want_payoffs=True)["payoffs"]
    order = np.argsort(st)
    p, top, second = int(order[-1]), float(st[order[-1]]), float(st[order[-2]])
    assert top - second > 1e-9 * top        # far above the kernel's rounding: the same path is on top on the GPU
    opt = capi.make_option(S0=100.0, T=1.0, K=0.5 * (top + second), r=0.1, v=0.2)

    def job(lo, cnt):
        return ctx.price_paths(opt, capi.make_sim(n, n_steps, capi.F64, seed=seed, path_offset=lo, n_paths_local=cnt))
    alone = job(p, 1)
    print(f"steps {n_steps}: path {p} pays {alone.sum!r}, oracle {top - opt.K!r}")
    assert alone.sum > 0 and abs(alone.sum - (top - opt.K)) <= RTOL * top
    windows = [(0, n), (1, n - 1), (max(p - 1, 0), 2), (max(p - 64, 0), 130), (max(p - 129, 0), 131), (max(p - 300, 0), 301)]
    for lo, cnt in windows:
        cnt = min(cnt, n - lo)
        assert lo <= p < lo + cnt
        got = job(lo, cnt)
        assert got.sum == alone.sum and got.sumsq == alone.sumsq, (n_steps, p, lo, cnt, got.sum, alone.sum)
    # both chains were exercised: the path's position in its window is even (chain A) in some and odd (chain B) in others
    assert {(p - lo) % 2 for lo, _ in windows} == {0, 1}


@pytest.mark.parametrize("n_steps", [1, 2, 5, 252, 253])
def test_a_shard_that_starts_at_an_odd_path_id_adds_up_to_the_whole_job(ctx, n_steps):
    opt, n = capi.make_option(**BENCH), 1000
    whole = ctx.price_paths(opt, capi.make_sim(n, n_steps, capi.F64, seed=5))
    for cut in (1, 333, 641):
        a = ctx.price_paths(opt, capi.make_sim(n, n_steps, capi.F64, seed=5, path_offset=0, n_paths_local=cut))
        b = ctx.price_paths(opt, capi.make_sim(n, n_steps, capi.F64, seed=5, path_offset=cut, n_paths_local=n - cut))
        print(f"steps {n_steps} cut {cut}: {a.sum + b.sum!r} whole {whole.sum!r}")
        assert a.n + b.n == n
        assert math.isclose(a.sum + b.sum, whole.sum, rel_tol=1e-13)
        assert math.isclose(a.sumsq + b.sumsq, whole.sumsq, rel_tol=1e-13)
