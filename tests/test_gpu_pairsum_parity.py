"""The fp64 pair-sum kernels against the CPU oracle at the shapes where their loop changes route.

The window-less log-space pricer (price_kernel<double, false, true, VR>) and the pathwise Greeks kernel walk two paths
per thread through pair_sums_of_paths (csrc/mc_device.hpp), whose radius comes from f64::neg2log_1k on the 1024-entry
log table.  The shapes:
  n_paths  1, 2 (one lane, its one or two paths), 127, 128, 129 (a full wavefront of two-path threads, one path less,
           one more), 513 (a second workgroup);
  n_steps  1 (the block's first normal alone: head_words), 2, 3, 4, 5 (odd last steps, the split pair), 252;
  plain, antithetic and control-variate runs (VR = 0, 1, 2);
  a path_offset that makes one wavefront straddle a multiple of 2^32, where the chains cannot share the Philox head and
  the loop takes its plain-rounds route.
sum and sumsq are compared with the oracle at 1e-11 relative.  The strike is 60 on a spot of 100: every path ends in
the money and its payoff S_T - K keeps the path's own relative error (< 1e-12 after 252 steps, tests/test_gpu_parity.py)
within a factor 3, so a sum of one path is held to the same relative bound as a sum of 513."""
import importlib
import math

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
capi = importlib.import_module("monte-carlo-project-cuda_amd").capi

OPT = dict(S0=100.0, T=1.0, K=60.0, r=0.1, v=0.2)
RTOL = 1e-11
N_PATHS = [1, 2, 127, 128, 129, 513]
N_STEPS = [1, 2, 3, 4, 5, 252]
MODES = {"plain": 0, "antithetic": capi.FLAG_ANTITHETIC, "control_variate": capi.FLAG_CONTROL_VARIATE}
STRADDLE = (1 << 32) - 37      # 129 paths from here: the first wavefront's 128 span 2^32 - 37 .. 2^32 + 90


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


def compare(ctx, oracle, sim, flags):
    opt = capi.make_option(**OPT)
    res = ctx.price_paths(opt, sim)
    p = oracle.make_params(**OPT, n_paths=sim.n_paths, n_steps=sim.n_steps, seed=sim.seed)
    want = oracle.mc_paths_vr(p, capi.F64, sim.path_offset, sim.n_paths_local, bool(flags & capi.FLAG_ANTITHETIC),
                              OPT["S0"] * math.exp(OPT["r"] * OPT["T"]))
    e1, e2 = abs(res.sum - want[0]) / want[0], abs(res.sumsq - want[1]) / want[1]
    print(f"n_local {sim.n_paths_local} steps {sim.n_steps} offset {sim.path_offset} flags {flags}: "
          f"sum rel {e1:.2e} sumsq rel {e2:.2e}")
    assert res.n == sim.n_paths_local and want[0] > 0
    assert e1 <= RTOL and e2 <= RTOL, (e1, e2)
    return res


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_steps", N_STEPS)
def test_price_pair_sum_vs_oracle(ctx, oracle, mode, n_steps):
    for n in N_PATHS:
        compare(ctx, oracle, capi.make_sim(n, n_steps, capi.F64, seed=20261020, flags=MODES[mode]), MODES[mode])


@pytest.mark.parametrize("mode", MODES)
def test_price_pair_sum_straddling_a_multiple_of_2_pow_32(ctx, oracle, mode):
    for n_steps in N_STEPS:
        sim = capi.make_sim(1 << 33, n_steps, capi.F64, seed=20261020, path_offset=STRADDLE, n_paths_local=129,
                            flags=MODES[mode])
        compare(ctx, oracle, sim, MODES[mode])


def test_pathwise_greeks_price_sample_is_the_pricer_s(ctx, oracle):
    # greeks_pathwise_kernel runs the same loop: its price sample must be price_kernel's sum, at the same shapes
    opt = capi.make_option(**OPT)
    for n_steps in N_STEPS:
        for n, lo in [(n, 0) for n in N_PATHS] + [(129, STRADDLE)]:
            sim = capi.make_sim(max(n, 1 << 33) if lo else n, n_steps, capi.F64, seed=20261020, path_offset=lo,
                                n_paths_local=n)
            g, p = ctx.price_greeks(opt, sim, capi.GREEKS_PATHWISE), ctx.price_paths(opt, sim)
            assert g.n == p.n == n
            assert abs(g.sum[0] - p.sum) <= 1e-12 * p.sum and abs(g.sumsq[0] - p.sumsq) <= 1e-12 * p.sumsq
