// capi_localvol.cpp — the calls of the C ABI that walk a local-volatility surface: the surface itself, European and
// barrier options, cliquets and variance swaps, Greeks by tangent paths, the strike-by-expiry smile and the worst-of
// autocallable on per-asset surfaces.  Each call is a prepare_* step (the refusals and the job) and its synchronous
// and enqueue forms; the refusals keep one order: the request alone, then the surface, then the context.  What a smile
// call is whatever the model (its nodes, its call, its two drivers) is capi_smile.cpp's.
#include "capi_internal.hpp"
#include "autocall_localvol.hpp"
#include "cliquet.hpp"
#include "localvol.hpp"
#include "localvol_greeks.hpp"
#include "localvol_smile.hpp"

#include <vector>

static_assert(sizeof(mcamd_localvol_grid) == 24 && sizeof(mcamd_localvol) == 24,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(MCAMD_LOCALVOL_MAX_NODES == mcamd::kLocalVolMaxNodes, "the kernel's LDS budget holds MCAMD_LOCALVOL_MAX_NODES");
static_assert(sizeof(mcamd_cliquet) == 56 && sizeof(mcamd_cliquet_result) == 96,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(MCAMD_CLIQUET_SUM == mcamd::kCliquetSum && MCAMD_CLIQUET_COMPOUND == mcamd::kCliquetCompound &&
                  MCAMD_CLIQUET_VARIANCE == mcamd::kCliquetVariance,
              "the kernels' kinds are MCAMD_CLIQUET_*");
static_assert(sizeof(mcamd_localvol_greeks_job) == 24 && sizeof(mcamd_localvol_greeks) == 472,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(MCAMD_LOCALVOL_GREEKS_MAX_BUCKETS == mcamd::kLvGreeksMaxBuckets && MCAMD_LOCALVOL_GREEK_RHO_Q + 1 == mcamd::kLvGreeks,
              "the kernel's record holds six estimators and MCAMD_LOCALVOL_GREEKS_MAX_BUCKETS buckets");
static_assert(sizeof(mcamd_autocall_localvol) == 632, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");

using namespace mcamd::capi;

namespace mcamd::capi {

// What mcamd_localvol_surface_create and the host lookup refuse of a grid and its table; *sigma_max (nullable) receives
// the largest entry.
int check_localvol_grid(const mcamd_localvol_grid *grid, const double *h_sigma, double *sigma_max)
{
    if (!grid || !h_sigma) return fail(MCAMD_ERR_INVALID, "grid and h_sigma must be non-NULL");
    if (grid->n_t < 1 || grid->n_x < 2)
        return fail(MCAMD_ERR_INVALID, "a surface needs n_t >= 1 and n_x >= 2, got n_t = %u, n_x = %u", grid->n_t, grid->n_x);
    if (static_cast<uint64_t>(grid->n_t) * grid->n_x > MCAMD_LOCALVOL_MAX_NODES)
        return fail(MCAMD_ERR_INVALID, "n_t * n_x = %llu nodes; at most %d fit the kernel's LDS table",
                    static_cast<unsigned long long>(static_cast<uint64_t>(grid->n_t) * grid->n_x), MCAMD_LOCALVOL_MAX_NODES);
    if (!std::isfinite(grid->x_min) || !std::isfinite(grid->x_max) || !(grid->x_min < grid->x_max))
        return fail(MCAMD_ERR_INVALID, "the surface's axis needs finite x_min < x_max, got [%g, %g]", grid->x_min,
                    grid->x_max);
    double top = 0.0;
    const uint32_t n = grid->n_t * grid->n_x;
    for (uint32_t e = 0; e < n; ++e) {
        if (!std::isfinite(h_sigma[e]) || !(h_sigma[e] > 0.0))
            return fail(MCAMD_ERR_INVALID, "every surface entry must be finite and > 0: sigma[%u][%u] = %g", e / grid->n_x,
                        e % grid->n_x, h_sigma[e]);
        top = std::fmax(top, h_sigma[e]);
    }
    if (sigma_max) *sigma_max = top;
    return MCAMD_OK;
}

// What the cliquet call and its closed form refuse of the kind ...
int check_cliquet_kind(int kind)
{
    if (kind < MCAMD_CLIQUET_SUM || kind > MCAMD_CLIQUET_VARIANCE)
        return fail(MCAMD_ERR_INVALID, "kind must be MCAMD_CLIQUET_SUM (0), MCAMD_CLIQUET_COMPOUND (1) or "
                                       "MCAMD_CLIQUET_VARIANCE (2), got %d", kind);
    return MCAMD_OK;
}

// ... of the local bounds whatever the kind ...
int check_cliquet_local(double local_floor, double local_cap)
{
    if (std::isnan(local_floor) || std::isnan(local_cap))
        return fail(MCAMD_ERR_INVALID, "a bound must not be NaN (-inf / +inf: none): local_floor = %g, local_cap = %g",
                    local_floor, local_cap);
    if (!(local_floor < local_cap))
        return fail(MCAMD_ERR_INVALID, "local_floor must lie below local_cap, got %g and %g", local_floor, local_cap);
    return MCAMD_OK;
}

// ... and of the local bounds what depends on the kind.
int check_cliquet_kind_bounds(int kind, double local_floor, double local_cap)
{
    if (kind == MCAMD_CLIQUET_COMPOUND && (local_floor < -1.0 || !(local_cap > -1.0)))
        return fail(MCAMD_ERR_INVALID, "a compounding cliquet needs local_floor >= -1 and local_cap > -1 (a gross return "
                                       "is positive), got %g and %g", local_floor, local_cap);
    if (kind == MCAMD_CLIQUET_VARIANCE && (local_floor != -HUGE_VAL || local_cap != HUGE_VAL))
        return fail(MCAMD_ERR_INVALID, "realized variance takes no local bounds: local_floor must be -inf and local_cap "
                                       "+inf, got %g and %g", local_floor, local_cap);
    return MCAMD_OK;
}

// ... and of the job whatever walks the paths, in mcamd_price_cliquet's order: kind, reserved, the reset schedule against
// n_steps, the bounds.
int check_cliquet_job(const mcamd_cliquet *cq, uint32_t n_steps)
{
    if (int rc = check_cliquet_kind(cq->kind)) return rc;
    if (cq->reserved != 0) return fail(MCAMD_ERR_INVALID, "cliquet->reserved must be 0, got %d", cq->reserved);
    if (cq->reset_every == 0 || n_steps % cq->reset_every != 0)
        return fail(MCAMD_ERR_INVALID, "reset_every must be >= 1 and divide n_steps (reset_every = %u, n_steps = %u)",
                    cq->reset_every, n_steps);
    const uint32_t M = n_steps / cq->reset_every;
    if (M != 0 && (cq->first_period < 1 || cq->first_period > M))   // M == 0 is n_steps == 0, refused below
        return fail(MCAMD_ERR_INVALID, "first_period must be 1..%u (the periods), got %u", M, cq->first_period);
    if (std::isnan(cq->global_floor) || std::isnan(cq->global_cap))
        return fail(MCAMD_ERR_INVALID, "a bound must not be NaN (-inf / +inf: none): global_floor = %g, global_cap = %g",
                    cq->global_floor, cq->global_cap);
    if (int rc = check_cliquet_local(cq->local_floor, cq->local_cap)) return rc;
    if (!(cq->global_floor < cq->global_cap))
        return fail(MCAMD_ERR_INVALID, "global_floor must lie below global_cap, got %g and %g", cq->global_floor,
                    cq->global_cap);
    if (int rc = check_cliquet_kind_bounds(cq->kind, cq->local_floor, cq->local_cap)) return rc;
    return MCAMD_OK;
}

void finalize_localvol_greeks_into(const double stats[32], double r, double T, uint32_t n_buckets, int gamma_defined,
                                   mcamd_localvol_greeks *out)
{
    const double disc = std::exp(-r * T);
    const uint64_t n = static_cast<uint64_t>(std::llround(stats[kLvGreeksRecord]));
    out->n = n;
    for (int k = 0; k < kLvGreeks; ++k) {
        const Estimate e = estimate(stats[2 * k], stats[2 * k + 1], n, disc);
        out->sum[k] = stats[2 * k];
        out->sumsq[k] = stats[2 * k + 1];
        out->value[k] = e.value;
        out->std_err[k] = e.std_err;
    }
    if (!gamma_defined) {
        out->value[MCAMD_LOCALVOL_GREEK_GAMMA] = out->std_err[MCAMD_LOCALVOL_GREEK_GAMMA] = std::nan("");
        out->sum[MCAMD_LOCALVOL_GREEK_GAMMA] = out->sumsq[MCAMD_LOCALVOL_GREEK_GAMMA] = 0.0;
    }
    for (uint32_t b = 0; b < n_buckets; ++b) {
        const double *pair = stats + 2 * (kLvGreeks + b);
        const Estimate e = estimate(pair[0], pair[1], n, disc);
        out->bucket_sum[b] = pair[0];
        out->bucket_sumsq[b] = pair[1];
        out->bucket_value[b] = e.value;
        out->bucket_std_err[b] = e.std_err;
    }
}

}  // namespace mcamd::capi

namespace {

// check_request's fp64 bound with the largest drift and volatility any node of a surface can give; asset >= 0 names
// the asset the surface belongs to; start: the largest |X_0| of the call's walks.
int check_localvol_exponent_range(double mu, double sigma_max, double dt, uint32_t n_steps, int asset = -1,
                                  double start = 0.0)
{
    const double per_step = (std::fabs(mu) + 0.5 * sigma_max * sigma_max) * dt + 8.6 * sigma_max * std::sqrt(dt);
    if (per_step < 700.0 && per_step * static_cast<double>(n_steps) + start < 20000.0) return MCAMD_OK;
    if (asset < 0)
        return fail(MCAMD_ERR_INVALID,
                    "fp64 path: |drift| + 8.6 vol = %.3g per step over %u steps exceeds the exponent range "
                    "(per step < 700, per path < 20000)", per_step, n_steps);
    return fail(MCAMD_ERR_INVALID,
                "fp64 path: |drift| + 8.6 vol = %.3g per step over %u steps exceeds the exponent range "
                "(per step < 700, per path < 20000; asset %d)", per_step, n_steps, asset);
}

// whether the surface was created on this context (a NULL context owns none)
bool surface_belongs(const mcamd_localvol_surface *surface, const mcamd_ctx *ctx)
{
    return ctx && surface->ctx == ctx && surface->ctx_id == ctx->id;
}

// the surface as a job of the given path precision carries it
mcamd::LocalVolGrid job_surface(const mcamd_localvol_surface *surface, int precision)
{
    return {surface->grid.n_t, surface->grid.n_x, surface->grid.x_min, surface->grid.x_max,
            precision == MCAMD_F32 ? surface->d_tab32 : surface->d_tab64};
}

// The two refusal stages the four single-surface calls share; a call's own checks stand between them.
// The drift stage (name: how the messages call the product): the dividend yield q, the rate, then the option (seen: the
// caller's copy with every field it does not read made harmless), the flags and sim.  *mu receives r - q.
int check_walk_drift(const char *name, const mcamd_option &seen, const mcamd_sim *sim, double q, double *mu)
{
    if (!std::isfinite(q)) return fail(MCAMD_ERR_INVALID, "the dividend yield q must be finite, got %g", q);
    if (!std::isfinite(seen.r)) return fail(MCAMD_ERR_INVALID, "option parameters must be finite with T > 0");
    *mu = seen.r - q;
    return check_drift_request(name, seen, sim, mu, 1);
}

// The surface stage: the surface (null_message: the call's own words for a NULL one), its fp64 exponent range (start:
// the largest |X_0| of the call's walks), then the context and whether it owns the surface.  Fills *walk.
int make_walk(const char *null_message, const mcamd_ctx *ctx, const mcamd_localvol_surface *surface, double mu,
              const mcamd_option *opt, const mcamd_sim *sim, double start, mcamd::LocalVolWalk *walk)
{
    if (!surface) return fail(MCAMD_ERR_INVALID, "%s", null_message);
    const double dt = even_dt(opt, sim);
    if (sim->precision == MCAMD_F64)
        if (int rc = check_localvol_exponent_range(mu, surface->sigma_max, dt, sim->n_steps, -1, start)) return rc;
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (!surface_belongs(surface, ctx)) return fail(MCAMD_ERR_INVALID, "the surface was created on another context");
    *walk = {path_range(sim), mu, dt, job_surface(surface, sim->precision)};
    return MCAMD_OK;
}

// The local-volatility calls.  The kernel always finishes its own sum (one_path_per_thread_grid caps the grid); every
// refusal that depends on the request alone comes before the context is looked at, and all that do not need the
// surface before the surface is.  opt->v is ignored.
template <typename Drive>
int prepare_localvol(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_localvol *lv,
                     const mcamd_localvol_surface *surface, void *d_samples, Drive drive)
{
    if (!opt || !sim || !lv) return fail(MCAMD_ERR_INVALID, "opt, sim, localvol and surface must be non-NULL");
    if (int rc = check_payoff(lv->payoff)) return rc;
    if (lv->barrier != MCAMD_LOCALVOL_NO_BARRIER && (lv->barrier < MCAMD_BARRIER_DOWN_OUT || lv->barrier > MCAMD_BARRIER_UP_IN))
        return fail(MCAMD_ERR_INVALID, "localvol->barrier must be MCAMD_LOCALVOL_NO_BARRIER (-1) or MCAMD_BARRIER_DOWN_OUT (0) "
                                       ".. MCAMD_BARRIER_UP_IN (3), got %d", lv->barrier);
    if (int rc = check_monitoring(lv->monitoring)) return rc;
    if (lv->reserved != 0) return fail(MCAMD_ERR_INVALID, "localvol->reserved must be 0, got %d", lv->reserved);
    // a non-finite q is refused ahead of the barrier, which the drift stage comes after
    if (!std::isfinite(lv->q)) return fail(MCAMD_ERR_INVALID, "the dividend yield q must be finite, got %g", lv->q);
    const bool barrier = lv->barrier != MCAMD_LOCALVOL_NO_BARRIER;
    if (barrier) {
        if (int rc = check_barrier_kind(opt->S0, opt->B, lv->barrier, lv->payoff)) return rc;
    }
    double mu;
    if (int rc = check_walk_drift("local-volatility", *opt, sim, lv->q, &mu)) return rc;
    if (!(opt->S0 > 0.0)) return fail(MCAMD_ERR_INVALID, "local-volatility options need S0 > 0 (S0 = %g)", opt->S0);
    mcamd::LocalVolJob job;
    if (int rc = make_walk("opt, sim, localvol and surface must be non-NULL", ctx, surface, mu, opt, sim, 0.0, &job.walk))
        return rc;
    if (sim->n_paths_local == 0) return drive(empty_call());
    job.S0 = opt->S0;
    job.K = opt->K;
    job.B = opt->B;
    job.barrier = barrier;
    job.form = barrier_form(lv->barrier, lv->monitoring, lv->payoff);
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(sim->n_paths_local);
    return drive(DeviceCall{sim->n_paths_local, grid, mcamd::kLocalVolRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_localvol(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

// The cliquet calls: mcamd_price_localvol's paths without a barrier.  The refusals follow prepare_localvol's order: the
// request alone, then the surface, then the context.  opt->v, opt->K and opt->B are ignored, and S0 is read by nothing.
template <typename Drive>
int prepare_cliquet(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_cliquet *cq,
                    const mcamd_localvol_surface *surface, void *d_samples, Drive drive)
{
    if (!opt || !sim || !cq) return fail(MCAMD_ERR_INVALID, "opt, sim, cliquet and surface must be non-NULL");
    if (int rc = check_cliquet_job(cq, sim->n_steps)) return rc;
    const uint32_t M = sim->n_steps / cq->reset_every;
    // as prepare_localvol, on a copy that carries no spot, strike or barrier of its own either
    mcamd_option seen = *opt;
    seen.S0 = 1.0;
    seen.K = seen.B = 0.0;
    double mu;
    if (int rc = check_walk_drift("cliquet", seen, sim, cq->q, &mu)) return rc;
    mcamd::CliquetJob job;
    if (int rc = make_walk("opt, sim, cliquet and surface must be non-NULL", ctx, surface, mu, opt, sim, 0.0, &job.walk))
        return rc;
    if (sim->n_paths_local == 0) return drive(empty_call());
    job.kind = cq->kind;
    job.reset_every = cq->reset_every;
    job.first_period = cq->first_period;
    const bool compound = cq->kind == MCAMD_CLIQUET_COMPOUND;
    job.local_lo = compound ? std::log(1.0 + cq->local_floor) : cq->local_floor;
    job.local_hi = compound ? std::log(1.0 + cq->local_cap) : cq->local_cap;
    job.global_lo = cq->global_floor;
    job.global_hi = cq->global_cap;
    const double P = static_cast<double>(M - cq->first_period + 1);
    job.scale = 1.0 / (P * (static_cast<double>(cq->reset_every) * job.walk.dt));
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(sim->n_paths_local);
    return drive(DeviceCall{sim->n_paths_local, grid, mcamd::kCliquetRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_cliquet(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

// The local-volatility Greeks calls: prepare_localvol's refusals for a barrier-less job, in its order, with the
// job's own in between.  The kernel finishes its own sum into the 32-double statistics record.  opt->v is ignored.
template <typename Drive>
int prepare_localvol_greeks(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                            const mcamd_localvol_greeks_job *gj, const mcamd_localvol_surface *surface, double *d_samples,
                            Drive drive)
{
    if (!opt || !sim || !gj) return fail(MCAMD_ERR_INVALID, "opt, sim, job and surface must be non-NULL");
    if (int rc = check_payoff(gj->payoff)) return rc;
    if (gj->n_vega_buckets > MCAMD_LOCALVOL_GREEKS_MAX_BUCKETS)
        return fail(MCAMD_ERR_INVALID, "n_vega_buckets must lie in 0 .. %d, got %u", MCAMD_LOCALVOL_GREEKS_MAX_BUCKETS,
                    gj->n_vega_buckets);
    if (!std::isfinite(gj->gamma_bump) || gj->gamma_bump < 0.0 || gj->gamma_bump > 0.1)
        return fail(MCAMD_ERR_INVALID, "gamma_bump must be finite and lie in 0 .. 0.1, got %g", gj->gamma_bump);
    double mu;
    if (int rc = check_walk_drift("local-volatility Greeks", *opt, sim, gj->q, &mu)) return rc;
    if (!(opt->S0 > 0.0)) return fail(MCAMD_ERR_INVALID, "local-volatility Greeks need S0 > 0 (S0 = %g)", opt->S0);
    mcamd::LocalVolGreeksJob job;
    if (int rc = make_walk("opt, sim, job and surface must be non-NULL", ctx, surface, mu, opt, sim, gj->gamma_bump,
                           &job.walk))
        return rc;
    if (sim->n_paths_local == 0) return drive(empty_call(mcamd::kLvGreeksStats));
    job.S0 = opt->S0;
    job.K = opt->K;
    job.T = opt->T;
    job.put = gj->payoff == MCAMD_PAYOFF_PUT;
    job.n_buckets = gj->n_vega_buckets;
    job.gamma_bump = gj->gamma_bump;
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(sim->n_paths_local);
    return drive(DeviceCall{sim->n_paths_local, grid, mcamd::kLvGreeksRecord, mcamd::kLvGreeksStats, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_localvol_greeks(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

// The smile calls: mcamd_price_localvol's paths without a barrier, stopped at the expiry steps, every strike priced at
// every expiry.  The refusals follow prepare_localvol's order: the request alone, then the surface, then the context.
// drive(call) runs the form's driver (run_smile_sync, run_smile_enqueue of capi_smile.cpp: capi_internal.hpp explains why
// a smile has drivers of its own); call.n == 0 is the empty shard.  opt->v and opt->K are ignored.
template <typename Drive>
int prepare_smile(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_smile *sm,
                  const uint32_t *h_expiry_steps, const double *h_strikes, const mcamd_localvol_surface *surface,
                  void *d_spots, Drive drive)
{
    if (!opt || !sim || !sm || !h_expiry_steps || !h_strikes)
        return fail(MCAMD_ERR_INVALID, "opt, sim, smile, h_expiry_steps, h_strikes and surface must be non-NULL");
    if (int rc = check_payoff(sm->payoff)) return rc;
    if (sm->reserved != 0) return fail(MCAMD_ERR_INVALID, "smile->reserved must be 0, got %d", sm->reserved);
    mcamd::SmileJob job;
    if (int rc = check_smile_nodes(sm->n_expiries, sm->n_strikes, h_expiry_steps, sim->n_steps, h_strikes, sm->payoff,
                                   &job.nodes))
        return rc;
    // as prepare_localvol, on a copy that carries no strike of its own either
    mcamd_option seen = *opt;
    seen.K = 1.0;
    double mu;
    if (int rc = check_walk_drift("local-volatility smile", seen, sim, sm->q, &mu)) return rc;
    if (!(opt->S0 > 0.0)) return fail(MCAMD_ERR_INVALID, "local-volatility smile options need S0 > 0 (S0 = %g)", opt->S0);
    if (int rc = make_walk("opt, sim, smile, h_expiry_steps, h_strikes and surface must be non-NULL", ctx, surface, mu, opt,
                           sim, 0.0, &job.walk))
        return rc;
    job.S0 = opt->S0;
    job.d_spots = d_spots;
    return drive(make_smile_call(ctx, sim, job.nodes, opt->r, job.walk.dt,
                                 smile_launch<mcamd::SmileJob, mcamd::launch_localvol_smile>, &job));
}

// The autocall calls under per-asset local-volatility surfaces.  Every refusal that needs neither a surface nor the
// context comes first, in prepare_autocall's order; then the surfaces; then the context.  opt supplies r and T alone.
template <typename Drive>
int prepare_autocall_localvol(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                              const mcamd_autocall_localvol *ac, const mcamd_localvol_surface *const *surfaces,
                              void *d_samples, Drive drive)
{
    if (!opt || !sim || !ac) return fail(MCAMD_ERR_INVALID, "opt, sim, autocall and surfaces must be non-NULL");
    if (ac->reserved[0] != 0 || ac->reserved[1] != 0)
        return fail(MCAMD_ERR_INVALID, "autocall->reserved must be 0, got {%d, %d}", ac->reserved[0], ac->reserved[1]);
    // n_assets and corr through the basket's own checks and Cholesky factor, with unit volatilities
    double L[64];
    if (int rc = check_autocall_assets(ac->n_assets, nullptr, ac->corr, L)) return rc;
    const int d = ac->n_assets;
    for (int j = 0; j < d; ++j)
        if (!std::isfinite(ac->q[j]))
            return fail(MCAMD_ERR_INVALID, "every dividend yield q must be finite, got q[%d] = %g", j, ac->q[j]);
    const AutocallTerms terms = autocall_terms(ac);
    uint32_t M;
    if (int rc = check_autocall_schedule(terms, sim->n_steps, &M)) return rc;
    if (!std::isfinite(opt->r)) return fail(MCAMD_ERR_INVALID, "option parameters must be finite with T > 0");
    // as prepare_localvol, asset by asset, on a copy that carries no spot, strike or barrier of its own either
    double mu[MCAMD_BASKET_MAX_ASSETS];
    for (int j = 0; j < d; ++j) mu[j] = opt->r - ac->q[j];
    mcamd_option seen = *opt;
    seen.S0 = 1.0;
    seen.K = seen.B = 0.0;
    if (int rc = check_drift_request("local-volatility autocallable", seen, sim, mu, d)) return rc;
    // the surfaces
    if (!surfaces) return fail(MCAMD_ERR_INVALID, "opt, sim, autocall and surfaces must be non-NULL");
    for (int j = 0; j < d; ++j)
        if (!surfaces[j]) return fail(MCAMD_ERR_INVALID, "surfaces[%d] is NULL: every asset needs a surface", j);
    for (int j = 0; j < d; ++j)
        if (!surface_belongs(surfaces[j], ctx))
            return fail(MCAMD_ERR_INVALID, "the surface of asset %d was created on another context", j);
    uint64_t nodes = 0;
    for (int j = 0; j < d; ++j) nodes += static_cast<uint64_t>(surfaces[j]->grid.n_t) * surfaces[j]->grid.n_x;
    if (nodes > MCAMD_LOCALVOL_MAX_NODES)
        return fail(MCAMD_ERR_INVALID, "the %d surfaces hold %llu nodes together; at most %d fit the kernel's LDS tables "
                                       "(a surface passed for several assets counts once per asset)", d,
                    static_cast<unsigned long long>(nodes), MCAMD_LOCALVOL_MAX_NODES);
    const double dt = even_dt(opt, sim);
    if (sim->precision == MCAMD_F64)
        for (int j = 0; j < d; ++j)
            if (int rc = check_localvol_exponent_range(mu[j], surfaces[j]->sigma_max, dt, sim->n_steps, j)) return rc;
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (sim->n_paths_local == 0) return drive(empty_call());
    mcamd::AutocallLocalVolJob job{};
    job.paths = path_range(sim);
    job.d = d;
    for (int j = 0; j < d; ++j) {
        job.mu[j] = mu[j];
        for (int k = 0; k <= j; ++k) job.chol[j * (j + 1) / 2 + k] = L[8 * j + k];
        job.surface[j] = job_surface(surfaces[j], sim->precision);
    }
    make_autocall_schedule(terms, M, opt->r, opt->T, dt, &job.schedule);
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(sim->n_paths_local);
    return drive(DeviceCall{sim->n_paths_local, grid, mcamd::kAutocallRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_autocall_localvol(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

}  // namespace

extern "C" {

int mcamd_localvol_surface_create(mcamd_ctx *ctx, const mcamd_localvol_grid *grid, const double *h_sigma,
                                  mcamd_localvol_surface **surface)
{
    if (!surface) return fail(MCAMD_ERR_INVALID, "surface out-pointer is NULL");
    *surface = nullptr;
    double sigma_max = 0.0;
    if (int rc = check_localvol_grid(grid, h_sigma, &sigma_max)) return rc;
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    const uint32_t n_x = grid->n_x, n = grid->n_t * n_x;
    // the pairs: sigma_k and slope_k = sigma_{k+1} - sigma_k, the slope formed in double, then narrowed
    std::vector<mcamd::VolPair<double>> t64(n);
    std::vector<mcamd::VolPair<float>> t32(n);
    for (uint32_t e = 0; e < n; ++e) {
        const double slope = (e % n_x == n_x - 1) ? 0.0 : h_sigma[e + 1] - h_sigma[e];
        t64[e] = {h_sigma[e], slope};
        t32[e] = {static_cast<float>(h_sigma[e]), static_cast<float>(slope)};
    }
    mcamd_localvol_surface *s = new (std::nothrow) mcamd_localvol_surface;
    if (!s) return fail(MCAMD_ERR_NOMEM, "out of host memory");
    s->ctx = ctx;
    s->ctx_id = ctx->id;
    s->device = ctx->device;
    s->grid = *grid;
    s->sigma_max = sigma_max;
    const size_t bytes64 = n * sizeof(mcamd::VolPair<double>), bytes32 = n * sizeof(mcamd::VolPair<float>);
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(&s->d_tables, bytes64 + bytes32);
    if (e == hipSuccess) {
        s->d_tab64 = s->d_tables;
        s->d_tab32 = static_cast<char *>(s->d_tables) + bytes64;   // bytes64 is a multiple of 16
        e = hipMemcpy(s->d_tab64, t64.data(), bytes64, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMemcpy(s->d_tab32, t32.data(), bytes32, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (s->d_tables) (void)hipFree(s->d_tables);
        delete s;
        return fail(e == hipErrorOutOfMemory ? MCAMD_ERR_NOMEM : MCAMD_ERR_HIP, "surface upload: %s", hipGetErrorString(e));
    }
    *surface = s;
    return MCAMD_OK;
}

int mcamd_localvol_surface_destroy(mcamd_localvol_surface *surface)
{
    if (!surface) return MCAMD_OK;
    (void)hipSetDevice(surface->device);
    if (surface->d_tables) (void)hipFree(surface->d_tables);
    delete surface;
    return MCAMD_OK;
}

int mcamd_price_localvol(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_localvol *localvol,
                         const mcamd_localvol_surface *surface, void *d_samples, mcamd_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim, localvol, surface and res must be non-NULL");
    zero_result(res);
    return prepare_localvol(ctx, opt, sim, localvol, surface, d_samples, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) {
            finalize_counted_into(rec, sim->n_paths_local, opt->r, opt->T, res);
        });
    });
}

int mcamd_price_localvol_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                 const mcamd_localvol *localvol, const mcamd_localvol_surface *surface, void *d_samples,
                                 double *d_stats)
{
    return prepare_localvol(ctx, opt, sim, localvol, surface, d_samples,
                            [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

int mcamd_price_cliquet(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_cliquet *cliquet,
                        const mcamd_localvol_surface *surface, void *d_samples, mcamd_cliquet_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim, cliquet, surface and res must be non-NULL");
    std::memset(res, 0, sizeof *res);
    return prepare_cliquet(ctx, opt, sim, cliquet, surface, d_samples, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) {
            // {sum, sumsq, paths on the global floor, paths on the global cap, wave-steps}
            finalize_into(rec[0], rec[1], sim->n_paths_local, opt->r, opt->T, res);
            res->n_floored = static_cast<uint64_t>(std::llround(rec[2]));
            res->n_capped = static_cast<uint64_t>(std::llround(rec[3]));
            res->work_steps = 64.0 * rec[4];   // wave-steps x 64 lanes
        });
    });
}

int mcamd_price_cliquet_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                const mcamd_cliquet *cliquet, const mcamd_localvol_surface *surface, void *d_samples,
                                double *d_stats)
{
    return prepare_cliquet(ctx, opt, sim, cliquet, surface, d_samples,
                           [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

int mcamd_price_localvol_greeks(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                const mcamd_localvol_greeks_job *job, const mcamd_localvol_surface *surface,
                                double *d_samples, mcamd_localvol_greeks *out)
{
    if (!out) return fail(MCAMD_ERR_INVALID, "opt, sim, job, surface and out must be non-NULL");
    std::memset(out, 0, sizeof *out);
    return prepare_localvol_greeks(ctx, opt, sim, job, surface, d_samples, [&](const auto &call) {
        return run_sync(ctx, call, out, [&](const double *stats) {
            finalize_localvol_greeks_into(stats, opt->r, opt->T, job->n_vega_buckets, job->gamma_bump > 0.0, out);
        });
    });
}

int mcamd_price_localvol_greeks_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                        const mcamd_localvol_greeks_job *job, const mcamd_localvol_surface *surface,
                                        double *d_samples, double *d_stats)
{
    return prepare_localvol_greeks(ctx, opt, sim, job, surface, d_samples, [&](const auto &call) {
        if (call.n && d_stats) {   // NaN (all-ones bytes) until the kernel has written the record
            HIP_TRY(hipSetDevice(ctx->device));
            HIP_TRY(hipMemsetAsync(d_stats, 0xFF, mcamd::kLvGreeksStats * sizeof(double), ctx->stream));
        }
        return run_enqueue(ctx, call, d_stats);
    });
}

int mcamd_price_autocall_localvol(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                  const mcamd_autocall_localvol *autocall, const mcamd_localvol_surface *const *surfaces,
                                  void *d_samples, mcamd_autocall_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim, autocall, surfaces and res must be non-NULL");
    std::memset(res, 0, sizeof *res);
    return prepare_autocall_localvol(ctx, opt, sim, autocall, surfaces, d_samples, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) {
            fill_autocall_result(rec, sim->n_paths_local, opt->r, opt->T, res);
        });
    });
}

int mcamd_price_autocall_localvol_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                          const mcamd_autocall_localvol *autocall,
                                          const mcamd_localvol_surface *const *surfaces, void *d_samples, double *d_stats)
{
    return prepare_autocall_localvol(ctx, opt, sim, autocall, surfaces, d_samples,
                                     [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

int mcamd_price_localvol_smile(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_smile *smile,
                               const uint32_t *h_expiry_steps, const double *h_strikes,
                               const mcamd_localvol_surface *surface, void *d_spots, double *h_stats, mcamd_result *res)
{
    if (!res || !h_stats) return fail(MCAMD_ERR_INVALID, "h_stats and res must be non-NULL");
    zero_result(res);
    return prepare_smile(ctx, opt, sim, smile, h_expiry_steps, h_strikes, surface, d_spots,
                         [&](const SmileCall &call) { return run_smile_sync(ctx, call, h_stats, res); });
}

int mcamd_price_localvol_smile_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                       const mcamd_smile *smile, const uint32_t *h_expiry_steps, const double *h_strikes,
                                       const mcamd_localvol_surface *surface, void *d_spots, double *d_stats)
{
    if (!d_stats) return fail(MCAMD_ERR_INVALID, "d_stats is NULL");
    return prepare_smile(ctx, opt, sim, smile, h_expiry_steps, h_strikes, surface, d_spots,
                         [&](const SmileCall &call) { return run_smile_enqueue(ctx, call, d_stats); });
}

}  // extern "C"
