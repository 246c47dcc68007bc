"""GPU: the synchronous and the enqueue form of every call share their refusals.  For each pair, malformed requests
are refused by both forms with the same code, and a refused enqueue does not advance the enqueue ring (the count
mcamd_enqueued_kernel_ms reads)."""
import importlib

import pytest
import torch

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi

pytestmark = pytest.mark.gpu

F64 = capi.F64


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


def dev(n, dtype=torch.float64):
    return torch.zeros(int(n), dtype=dtype, device="cuda")


def opt(**kw):
    return capi.make_option(**kw)


def sim(n=64, steps=4, **kw):
    return capi.make_sim(n, steps, kw.pop("precision", F64), **kw)


def nmc_sim(**kw):
    return sim(n=8, steps=4, n_paths_inner=16, **kw)


# (name, synchronous call, enqueue call): each takes (ctx, opt, sim, buffers, stats) and runs one form
def _paths(c, o, s, b, stats):
    return c.price_paths(o, s) if stats is None else c.price_paths_enqueue(o, s, stats)


def _store(c, o, s, b, stats):
    if stats is None:
        return c.simulate_trajectories(o, s, b["traj"], None, None, layout=b["layout"])
    return c.simulate_trajectories_enqueue(o, s, b["traj"], None, None, stats, layout=b["layout"])


def _inner(c, o, s, b, stats):
    if stats is None:
        return c.nmc_inner(o, s, b["prices"], b["counts"], b["points"], layout=b["layout"], variant=b["variant"])
    return c.nmc_inner_enqueue(o, s, b["prices"], b["counts"], b["points"], stats, layout=b["layout"],
                               variant=b["variant"])


def _fused(c, o, s, b, stats):
    if stats is None:
        return c.nmc_fused(o, s, b["outer_seed"], b["prices"], b["counts"], b["points"], layout=b["layout"])
    return c.nmc_fused_enqueue(o, s, b["outer_seed"], b["prices"], b["counts"], b["points"], stats, layout=b["layout"])


def _greeks(c, o, s, b, stats):
    if stats is None:
        return c.price_greeks(o, s, b["method"])
    return c.price_greeks_enqueue(o, s, stats, b["method"])


def _buffers(**kw):
    b = dict(traj=dev(64 * 4), prices=dev(8 * 4), counts=dev(8 * 4, torch.int32), points=dev(8 * 4), layout=capi.STEP_MAJOR,
             variant=capi.NMC_WAVE_PER_POINT, outer_seed=77, method=capi.GREEKS_AUTO)
    b.update(kw)
    return b


CASES = [
    ("paths: precision", _paths, opt(), sim(precision=33), {}),
    ("paths: n_steps", _paths, opt(), sim(steps=0), {}),
    ("paths: flags", _paths, opt(), sim(flags=1 << 20), {}),
    ("paths: Tk", _paths, opt(Tk=4), sim(), {}),
    ("paths: log and product form", _paths, opt(), sim(flags=capi.FLAG_LOG_SPACE | capi.FLAG_PRODUCT_FORM), {}),
    ("paths: exponent range", _paths, opt(v=400.0), sim(), {}),
    ("store: layout", _store, opt(), sim(), dict(layout=7)),
    ("store: variance reduction", _store, opt(), sim(flags=capi.FLAG_ANTITHETIC), {}),
    ("store: d_traj", _store, opt(), sim(), dict(traj=None)),
    ("store: T", _store, opt(T=0.0), sim(), {}),
    ("inner: variant", _inner, opt(), nmc_sim(), dict(variant=99)),
    ("inner: layout", _inner, opt(), nmc_sim(), dict(layout=5)),
    ("inner: Tk", _inner, opt(Tk=1), nmc_sim(), {}),
    ("inner: n_paths_inner", _inner, opt(), sim(n=8, steps=4), {}),
    ("inner: d_prices", _inner, opt(), nmc_sim(), dict(prices=None)),
    ("inner: window without counts", _inner, opt(B=100.0, P1=1, P2=2, use_window=1), nmc_sim(), dict(counts=None)),
    ("inner: subsequence", _inner, opt(), nmc_sim(path_offset=(1 << 62)), {}),
    ("fused: outer seed", _fused, opt(), nmc_sim(seed=77), {}),
    ("fused: variance reduction", _fused, opt(), nmc_sim(flags=capi.FLAG_CONTROL_VARIATE), {}),
    ("fused: d_point_prices", _fused, opt(), nmc_sim(), dict(points=None)),
    ("greeks: pathwise with a window", _greeks, opt(B=100.0, P1=1, P2=2, use_window=1), sim(),
     dict(method=capi.GREEKS_PATHWISE)),
    ("greeks: method", _greeks, opt(), sim(), dict(method=7)),
    ("greeks: v > 0", _greeks, opt(v=0.0), sim(), {}),
    ("greeks: flags", _greeks, opt(), sim(flags=capi.FLAG_ANTITHETIC), {}),
    ("greeks: n_steps", _greeks, opt(), sim(steps=0), {}),
]


@pytest.mark.parametrize("name,call,o,s,kw", CASES, ids=[c[0] for c in CASES])
def test_both_forms_refuse_alike_and_a_refused_enqueue_is_not_counted(ctx, name, call, o, s, kw):
    b = _buffers(**kw)
    with pytest.raises(capi.McamdError) as sync_err:
        call(ctx, o, s, b, None)
    # one accepted enqueue, so that the ring holds exactly one call before the refused one
    ctx.price_paths_enqueue(opt(), sim(), dev(capi.GREEKS_STATS))
    stats = dev(capi.GREEKS_STATS)
    with pytest.raises(capi.McamdError) as enq_err:
        call(ctx, o, s, b, stats)
    assert sync_err.value.code == enq_err.value.code == capi.ERR_INVALID, (sync_err.value, enq_err.value)
    assert len(ctx.enqueued_kernel_ms(1)) == 1
    torch.cuda.current_stream().synchronize()
    assert torch.all(stats == 0), "a refused enqueue wrote its statistics buffer"


# ---- the surface stage of the four calls that walk one local-volatility surface -------------------------------------------
# After everything a call refuses of the request alone: the surface NULL, its fp64 exponent range, the context, and
# whether the context owns the surface, in this order and in the same words for every call.  No CPU test reaches the
# last three, because a surface needs a live context.  Every request here is refused, so no kernel runs.

class _NoSurface:
    _h = None   # what the wrappers pass to the library: a NULL surface


LV_OPT = dict(S0=100.0, K=100.0, T=100.0, r=0.1, v=0.0)   # dt = 2 over 50 steps: a volatility of 100 leaves the range
LV_STEPS, LV_STRIKES = (25, 50), (90.0, 110.0)


def _lv(c, o, s, surface, stats):
    job = capi.make_localvol()
    return c.price_localvol(o, s, job, surface) if stats is None else c.price_localvol_enqueue(o, s, job, surface, stats)


def _lv_smile(c, o, s, surface, stats):
    sm = capi.make_smile(len(LV_STEPS), len(LV_STRIKES))
    if stats is None:
        return c.price_localvol_smile(o, s, sm, LV_STEPS, LV_STRIKES, surface)
    return c.price_localvol_smile_enqueue(o, s, sm, LV_STEPS, LV_STRIKES, surface, stats)


def _lv_greeks(c, o, s, surface, stats):
    job = capi.make_localvol_greeks_job(n_vega_buckets=2, gamma_bump=0.01)
    if stats is None:
        return c.price_localvol_greeks(o, s, job, surface)
    return c.price_localvol_greeks_enqueue(o, s, job, surface, stats)


def _cliquet(c, o, s, surface, stats):
    cq = capi.make_cliquet(capi.CLIQUET_SUM, reset_every=10)
    return c.price_cliquet(o, s, cq, surface) if stats is None else c.price_cliquet_enqueue(o, s, cq, surface, stats)


# (call, its own words for a NULL surface)
LV_CALLS = {
    "localvol": (_lv, "opt, sim, localvol and surface must be non-NULL"),
    "smile": (_lv_smile, "opt, sim, smile, h_expiry_steps, h_strikes and surface must be non-NULL"),
    "greeks": (_lv_greeks, "opt, sim, job and surface must be non-NULL"),
    "cliquet": (_cliquet, "opt, sim, cliquet and surface must be non-NULL"),
}
LV_FORMS = [(name, form) for name in LV_CALLS for form in ("sync", "enqueue")]
# (case, what every call's message holds whatever the product)
LV_STAGES = [("no surface", "and surface must be non-NULL"), ("wild on its own context", "exponent range"),
             ("wild on the other context", "exponent range"), ("flat of the other context", "another context")]


@pytest.fixture(scope="module")
def two(ctx):
    """two contexts on device 0, a flat 1 x 2 surface on each, and on the first one whose volatility of 100 an fp64
    job of 50 steps over T = 100 cannot carry in its exponent"""
    other = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    made = []
    try:
        for c, sigma in ((ctx, [[0.2, 0.2]]), (other, [[0.2, 0.2]]), (ctx, [[0.2, 100.0]])):
            made.append(c.localvol_surface((1, 2, -1.0, 1.0), sigma))
        yield dict(a=ctx, b=other, flat_a=made[0], flat_b=made[1], wild_a=made[2])
    finally:
        for s in made:
            s.close()
        other.close()


def _lv_refusal(two, name, form, case):
    """(code, message) of the refusal of one case by one form of one call"""
    c, surface = {"no surface": (two["a"], _NoSurface), "wild on its own context": (two["a"], two["wild_a"]),
                  "wild on the other context": (two["b"], two["wild_a"]),
                  "flat of the other context": (two["a"], two["flat_b"])}[case]
    with pytest.raises(capi.McamdError) as e:
        LV_CALLS[name][0](c, opt(**LV_OPT), capi.make_sim(1000, 50, F64, n_paths_local=256), surface,
                          None if form == "sync" else dev(64))
    return e.value.code, str(e.value)


@pytest.mark.parametrize("name,form", LV_FORMS, ids=[f"{n}-{f}" for n, f in LV_FORMS])
def test_the_surface_stage_refuses_in_one_order(two, name, form):
    for case, fixed in LV_STAGES:
        code, msg = _lv_refusal(two, name, form, case)
        assert code == capi.ERR_INVALID and fixed in msg, (case, msg)
        if case == "no surface":
            assert LV_CALLS[name][1] in msg, msg
    # the flat surface on its own context passes every refusal of the request: an empty shard is accepted
    empty = capi.make_sim(1000, 50, F64, n_paths_local=0)
    for c, surface in ((two["a"], two["flat_a"]), (two["b"], two["flat_b"])):
        LV_CALLS[name][0](c, opt(**LV_OPT), empty, surface, None if form == "sync" else dev(64))


@pytest.mark.parametrize("case,fixed", LV_STAGES, ids=[c for c, _ in LV_STAGES])
def test_the_surface_stage_speaks_alike_in_every_call(two, case, fixed):
    said = {(name, form): _lv_refusal(two, name, form, case) for name, form in LV_FORMS}
    # from the fixed words on for the NULL surface, whose message names the call's arguments before them; whole otherwise
    tails = {(code, msg[msg.index(fixed):] if case == "no surface" else msg) for code, msg in said.values()}
    assert len(tails) == 1, said


def test_a_refused_enqueue_leaves_the_ring_count(ctx):
    fresh = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        fresh.price_paths_enqueue(opt(), sim(), dev(capi.GREEKS_STATS))
        stats = dev(capi.GREEKS_STATS)
        for name, call, o, s, kw in CASES:
            with pytest.raises(capi.McamdError):
                call(fresh, o, s, _buffers(**kw), stats)
        assert len(fresh.enqueued_kernel_ms(1)) == 1
        with pytest.raises(capi.McamdError):
            fresh.enqueued_kernel_ms(2)   # the count is still 1
    finally:
        fresh.close()
