"""What the GPU tests of the two smile pricers (tests/test_gpu_localvol_smile.py, tests/test_gpu_heston_smile.py) check
of a call's result in the same words, whatever model walked the paths: the strikes of the strike-phase cases, the work a
call reports, the fields of its mcamd_result, and the node sums against sums formed in numpy from the returned spots.
No fixtures; nothing here runs a kernel."""
import importlib

import numpy as np

import localvol_smile_restate as sm

capi = importlib.import_module("monte-carlo-project-cuda_amd").capi

# of a node's sum: the strike phase sums in float64 whatever the path precision, h is formed in the path precision
SUM_RTOL = {capi.F64: 1e-11, capi.F32: 2e-5}


def strikes_for(n_K):
    """from deep in to deep out of the money: a call at 2000 and a put at 5 never pay, the other end always does"""
    return [100.0] if n_K == 1 else list(np.geomspace(5.0, 2000.0, n_K))


def full_work(n, last):
    return 64 * -(-n // 64) * last


def check_result_fields(res, stats, n, steps, n_K, n_steps, r, T):
    """r, T: the rate and the maturity of the job's option (the last node is discounted to its own expiry)"""
    nodes = len(steps) * n_K
    assert res.n == n and res.block == 256 and res.work_steps == res.live_steps == full_work(n, steps[-1])
    assert (res.sum, res.sumsq) == (stats[nodes - 1], stats[2 * nodes - 1])
    fin = capi.finalize(res.sum, res.sumsq, n, r, steps[-1] * (T / n_steps))
    assert (res.price, res.std_err, res.ci_lo, res.ci_hi) == (fin.price, fin.std_err, fin.ci_lo, fin.ci_hi)
    assert res.sum_c == res.sum_cc == res.sum_yc == res.cv_beta == res.cv_rho == 0.0
    assert 0.0 < res.kernel_ms < 1e4 and 0.0 < res.total_ms < 1e4


def check_sums_from_spots(prec, spots, strikes, payoff, stats, tag="", threads=1):
    """the strike phase alone: node sums against sums formed in numpy from the returned spots"""
    nodes = spots.shape[0] * len(strikes)
    want, wantsq, paying = sm.node_sums(spots, strikes, payoff, threads=threads)
    got, gotsq = stats[:nodes].reshape(want.shape), stats[nodes:].reshape(want.shape)
    rt = SUM_RTOL[prec]
    worst = float(np.max(np.abs(got - want) / np.where(want > 0, want, 1.0)))
    print(f"{tag}: worst relative deviation of a node sum {worst:.3e}, nodes that never pay {(want == 0).sum()}, "
          f"nodes where every path pays {(paying == spots.shape[1]).sum()}")
    assert (np.abs(got - want) <= rt * want).all() and (np.abs(gotsq - wantsq) <= rt * wantsq).all()
    assert (got[want == 0] == 0).all() and (gotsq[want == 0] == 0).all()
    return want, paying
