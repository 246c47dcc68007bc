"""Overlapped enqueues: consecutive large mcamd_price_paths_enqueue jobs run their simulation kernels on two
internal streams of the context and only their final reductions on the caller's stream.  What must not change: every
record's bits, and the order of d_stats writes on the caller's stream.

The smallest overlapped shape: fp64 or fp32, no window, n_steps = 32 (a thread owns two paths from 32 steps on) and more
than 8192 workgroups of 512 paths: n = 4 194 817 (8194 workgroups, odd path count) and n = 4 718 593 (9217).  Either is
about 0.15 ms of kernel.  The reference of every job is the synchronous mcamd_price_paths record of the same request, taken
once per request on a context of its own and compared exactly (sum, sumsq, the control variate's three sums, n).

Every sequence runs with MCAMD_ENQUEUE_OVERLAP unset, "0" (in order, as before) and "1"; the variable is read when a
context is created, so each mode is a context of its own.  No test captures a graph, and none provokes a device failure."""
import contextlib
import importlib
import math
import os
import time

import pytest

torch = pytest.importorskip("torch")

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

pytestmark = pytest.mark.gpu

VAR = "MCAMD_ENQUEUE_OVERLAP"
N_A, N_B = 4_194_817, 4_718_593   # 8194 and 9217 workgroups
STEPS = 32
MODES = [None, "0", "1"]
PLAIN, CV = 0, capi.FLAG_CONTROL_VARIATE
OPT = dict(S0=100.0, K=100.0, r=0.1, T=1.0, v=0.2)
WINDOW = dict(OPT, B=120.0, P1=2, P2=20, use_window=1)


@contextlib.contextmanager
def overlap_env(value):
    old = os.environ.get(VAR)
    if value is None:
        os.environ.pop(VAR, None)
    else:
        os.environ[VAR] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(VAR, None)
        else:
            os.environ[VAR] = old


@pytest.fixture(scope="module")
def stream():
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    yield s
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream())


def new_context(stream, mode):
    with overlap_env(mode):
        return capi.Context(0, stream.cuda_stream)


@pytest.fixture(scope="module", params=MODES, ids=lambda m: "unset" if m is None else "env" + m)
def ctx(request, stream):
    c = new_context(stream, request.param)
    yield c
    torch.cuda.synchronize()
    c.close()


@pytest.fixture(scope="module")
def reference(stream):
    """record(opt kwargs, sim kwargs) -> the six doubles the synchronous call implies; each request runs once"""
    c = new_context(stream, "0")
    seen = {}

    def record(opt_kw, n, prec, seed, flags, n_local=None):
        key = (tuple(sorted(opt_kw.items())), n, prec, seed, flags, n_local)
        if key not in seen:
            if n_local == 0:
                seen[key] = [0.0] * 6
            else:
                r = c.price_paths(capi.make_option(**opt_kw), capi.make_sim(n, STEPS, prec, seed, flags=flags))
                seen[key] = [r.sum, r.sumsq, r.sum_c, r.sum_cc, r.sum_yc, float(r.n)]
        return seen[key]

    yield record
    c.close()


def enqueue(ctx, row, opt_kw, n, prec, seed, flags, n_local=None):
    ctx.price_paths_enqueue(capi.make_option(**opt_kw), capi.make_sim(n, STEPS, prec, seed, n_paths_local=n_local, flags=flags), row)


def same_bits(got, want):
    """exact, NaN included (a NaN row is a row nobody wrote)"""
    import struct
    return struct.pack("6d", *got) == struct.pack("6d", *want)


def check_rows(stats, jobs, reference):
    torch.cuda.synchronize()
    rows = stats.cpu().tolist()
    for i, job in enumerate(jobs):
        want = reference(*job)
        assert same_bits(rows[i], want), (i, job[1:], rows[i], want)


def run_sequence(ctx, jobs, reference):
    stats = torch.full((len(jobs), 6), math.nan, dtype=torch.float64, device="cuda")
    for i, job in enumerate(jobs):
        enqueue(ctx, stats[i], *job)
    check_rows(stats, jobs, reference)


@pytest.mark.parametrize("prec,flags", [(capi.F64, PLAIN), (capi.F64, CV), (capi.F32, PLAIN)], ids=["f64", "f64-cv", "f32"])
def test_sixteen_jobs_back_to_back_keep_their_bits(ctx, reference, prec, flags):
    run_sequence(ctx, [(OPT, N_A if i % 2 == 0 else N_B, prec, 100 + i, flags) for i in range(16)], reference)


def test_mixed_sequence(ctx, reference):
    # overlapped (lane A, 8194 records), folded, empty shard, overlapped (lane B), a window job, overlapped (lane A again,
    # now 9217 records of 5 doubles), overlapped (lane B, 8194 records of 2)
    jobs = [(OPT, N_A, capi.F64, 1, PLAIN),
            (OPT, 1000, capi.F64, 2, PLAIN),
            (OPT, N_A, capi.F64, 3, PLAIN, 0),
            (OPT, N_B, capi.F64, 4, PLAIN),
            (WINDOW, 300_001, capi.F64, 5, PLAIN),
            (OPT, N_B, capi.F64, 6, CV),
            (OPT, N_A, capi.F64, 7, PLAIN)]
    run_sequence(ctx, jobs, reference)


def test_d_stats_is_ordered_on_the_callers_stream(ctx, reference):
    jobs = [(OPT, N_A if i % 2 == 0 else N_B, capi.F64, 200 + i, PLAIN) for i in range(6)]
    stats = torch.zeros((len(jobs), 6), dtype=torch.float64, device="cuda")
    copies = torch.zeros_like(stats)
    for i, job in enumerate(jobs):
        stats[i].fill_(math.nan)        # enqueued before the job: the job's record must land after it ...
        enqueue(ctx, stats[i], *job)
        copies[i].copy_(stats[i])       # ... and before what is enqueued after it
    check_rows(copies, jobs, reference)
    check_rows(stats, jobs, reference)


def test_two_jobs_into_one_row_leave_the_second(ctx, reference):
    first, second = (OPT, N_B, capi.F64, 301, PLAIN), (OPT, N_A, capi.F64, 302, PLAIN)
    stats = torch.full((1, 6), math.nan, dtype=torch.float64, device="cuda")
    enqueue(ctx, stats[0], *first)
    enqueue(ctx, stats[0], *second)
    check_rows(stats, [second], reference)


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "unset" if m is None else "env" + m)
def test_a_lane_buffer_grows_between_jobs(stream, reference, mode):
    # a fresh context: both lanes start with the small job's buffer (8194 x 2 doubles), then each needs 9217 x 5
    c = new_context(stream, mode)
    try:
        jobs = [(OPT, N_A, capi.F64, 401, PLAIN), (OPT, N_A, capi.F64, 402, PLAIN),
                (OPT, N_B, capi.F64, 403, CV), (OPT, N_B, capi.F64, 404, CV),
                (OPT, N_A, capi.F64, 405, PLAIN)]
        run_sequence(c, jobs, reference)
    finally:
        torch.cuda.synchronize()
        c.close()


def test_kernel_times_are_disjoint_intervals(stream):
    """Eight overlapped jobs: every time is positive, and as the times are disjoint parts of the stretch between the first
    enqueue and the end of the sync, their sum cannot exceed the host's wall time over it.  No tolerance.  The sizes
    alternate, and the smaller job regularly ends before the larger one enqueued just ahead of it: charged by enqueue
    order it would get 0 (seen on an MI355X: 0.1508, 0.3079, 0.0, 0.3089, 0.0, 0.3098, 0.0024, 0.1674), charged by the
    order of the ends it gets the part of its interval that is its own."""
    c = new_context(stream, "1")
    try:
        stats = torch.zeros((8, 6), dtype=torch.float64, device="cuda")
        enqueue(c, stats[0], OPT, N_A, capi.F64, 500, PLAIN)   # streams, events and buffers exist before the clock starts
        enqueue(c, stats[1], OPT, N_B, capi.F64, 501, PLAIN)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(8):
            enqueue(c, stats[i], OPT, N_A if i % 2 == 0 else N_B, capi.F64, 510 + i, PLAIN)
        ms = c.enqueued_kernel_ms(8)    # waits for the caller's stream and the internal ones
        wall_ms = (time.perf_counter() - t0) * 1e3
        print(f"kernel ms {[round(m, 4) for m in ms]}, sum {sum(ms):.4f}, wall {wall_ms:.4f}")
        assert all(m > 0.0 for m in ms), ms
        assert sum(ms) <= wall_ms, (ms, wall_ms)
    finally:
        torch.cuda.synchronize()
        c.close()
