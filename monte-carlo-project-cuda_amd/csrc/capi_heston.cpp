// capi_heston.cpp — the calls of the C ABI that walk Heston stochastic-volatility paths under the full-truncation Euler
// scheme: European options and their Greeks (include/mcamd_heston_greeks.h), the strike-by-expiry smile, cliquets and
// single barriers.  Each call is a prepare step (the refusals and the job) and its synchronous and enqueue forms; the
// refusals keep the order of the other families: the request alone, then the context.  The stages the prepare steps share are check_heston_job and check_heston_walk
// here, check_barrier_terms and barrier_form in capi_pathdep.cpp and check_smile_nodes in capi_smile.cpp.
#include "capi_internal.hpp"
#include "heston.hpp"
#include "heston_barrier.hpp"
#include "heston_cliquet.hpp"
#include "heston_greeks.hpp"
#include "heston_smile.hpp"
#include "mcamd_heston_greeks.h"

#include <cstdio>

static_assert(sizeof(mcamd_heston) == 64 && sizeof(mcamd_heston_result) == 96,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_heston_cliquet_result) == 112, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_heston_barrier_result) == 104, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_heston_greeks_job) == 56 && sizeof(mcamd_heston_greeks) == 208,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(MCAMD_HESTON_GREEKS_STATS == mcamd::kHestonGreeksStats && MCAMD_HESTON_GREEKS_STATS <= mcamd_ctx::kRecord &&
                  MCAMD_HESTON_GREEKS == 5 + mcamd::kHestonGreeksMaxParams &&
                  mcamd::heston_greeks_record(mcamd::kHestonGreeksMaxParams) < MCAMD_HESTON_GREEKS_STATS,
              "the Greeks record is the header's");
static_assert(MCAMD_HESTON_FULL_TRUNCATION == mcamd::kHestonFullTruncation, "the kernels' scheme is MCAMD_HESTON_*");

using namespace mcamd::capi;

namespace mcamd::capi {

// What the Heston call and its closed form refuse of the model's parameters.
int check_heston_model(double q, double v0, double kappa, double theta, double xi, double rho)
{
    if (!std::isfinite(q) || !std::isfinite(v0) || !std::isfinite(kappa) || !std::isfinite(theta) || !std::isfinite(xi) ||
        !std::isfinite(rho))
        return fail(MCAMD_ERR_INVALID, "the Heston parameters must be finite: q = %g, v0 = %g, kappa = %g, theta = %g, "
                                       "xi = %g, rho = %g", q, v0, kappa, theta, xi, rho);
    if (v0 < 0.0 || kappa < 0.0 || theta < 0.0 || xi < 0.0)
        return fail(MCAMD_ERR_INVALID, "Heston needs v0, kappa, theta and xi >= 0, got v0 = %g, kappa = %g, theta = %g, "
                                       "xi = %g", v0, kappa, theta, xi);
    if (std::fabs(rho) > 1.0) return fail(MCAMD_ERR_INVALID, "the correlation rho must lie in [-1, 1], got %g", rho);
    return MCAMD_OK;
}

}  // namespace mcamd::capi

namespace {

// What both Heston calls refuse of the job and of the rate, after the NULL pointers: payoff, scheme, reserved, the
// model, r.
int check_heston_job(const mcamd_option *opt, const mcamd_heston *hs)
{
    if (int rc = check_payoff(hs->payoff)) return rc;
    if (hs->scheme != MCAMD_HESTON_FULL_TRUNCATION)
        return fail(MCAMD_ERR_INVALID, "heston->scheme must be MCAMD_HESTON_FULL_TRUNCATION (0), got %d", hs->scheme);
    if (hs->reserved != 0.0) return fail(MCAMD_ERR_INVALID, "heston->reserved must be 0, got %g", hs->reserved);
    if (int rc = check_heston_model(hs->q, hs->v0, hs->kappa, hs->theta, hs->xi, hs->rho)) return rc;
    if (!std::isfinite(opt->r)) return fail(MCAMD_ERR_INVALID, "option parameters must be finite with T > 0");
    return MCAMD_OK;
}

// The walk of every job, read once check_heston_job has passed.  The refusals of sim and opt come after it: until then
// dt may be anything (n_steps == 0 divides by zero, in floating point) and nothing reads it.
mcamd::HestonWalk heston_walk(const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *hs)
{
    return {path_range(sim), opt->r - hs->q, even_dt(opt, sim), hs->v0, hs->kappa, hs->theta, hs->xi, hs->rho, hs->scheme};
}

// The walk stage of the calls that price off the spot (European, smile, barrier), after check_heston_job: the walk,
// then opt and sim at the drift r - q (what: how check_drift_request's messages call the product), then S0 and, with a
// strike of the option's own, K.  The drift check runs as the local-volatility calls' does, on a copy whose ignored
// fields are harmless (the variance is random: no bound on the request can cover it, so the drift stands alone in the
// fp64 exponent-range bound): the level bounds nothing here, and without a strike (the smile, whose nodes carry
// theirs) K does not either.  The cliquet keeps its own order (prepare_heston_cliquet).
int check_heston_walk(const char *what, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *hs,
                      bool with_strike, mcamd::HestonWalk *walk)
{
    *walk = heston_walk(opt, sim, hs);
    mcamd_option seen = *opt;
    seen.B = 0.0;
    if (!with_strike) seen.K = 1.0;
    if (int rc = check_drift_request(what, seen, sim, &walk->mu, 1)) return rc;
    if (!with_strike) {
        if (!(opt->S0 > 0.0)) return fail(MCAMD_ERR_INVALID, "Heston smile options need S0 > 0 (S0 = %g)", opt->S0);
    } else if (!(opt->S0 > 0.0) || !(opt->K > 0.0)) {
        return fail(MCAMD_ERR_INVALID, "Heston options need S0 > 0 and K > 0 (S0 = %g, K = %g)", opt->S0, opt->K);
    }
    return MCAMD_OK;
}

// The Heston calls.  The kernel always finishes its own sum (one_path_per_thread_grid caps the grid); every refusal
// depends on the request alone and comes before the context is looked at.  opt->v and opt->B are ignored.
template <typename Drive>
int prepare_heston(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *hs, void *d_samples,
                   void *d_state, Drive drive)
{
    if (!opt || !sim || !hs) return fail(MCAMD_ERR_INVALID, "opt, sim and heston must be non-NULL");
    if (int rc = check_heston_job(opt, hs)) return rc;
    mcamd::HestonJob job;
    if (int rc = check_heston_walk("Heston", opt, sim, hs, true, &job.walk)) return rc;
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (sim->n_paths_local == 0) return drive(empty_call());
    job.S0 = opt->S0;
    job.K = opt->K;
    job.put = hs->payoff == MCAMD_PAYOFF_PUT;
    job.d_samples = d_samples;
    job.d_state = d_state;
    const uint32_t grid = mcamd::one_path_per_thread_grid(sim->n_paths_local);
    return drive(DeviceCall{sim->n_paths_local, grid, mcamd::kHestonRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_heston(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

// The Heston smile calls: mcamd_price_heston's paths, stopped at the expiry steps, every strike priced at every expiry.
// The refusals: prepare_heston's of the job, the nodes as every smile call refuses them (check_smile_nodes),
// prepare_heston's of sim and opt, S0, then the context.  drive(call) runs the form's driver (run_smile_sync,
// run_smile_enqueue of capi_smile.cpp); call.n == 0 is the empty shard.  opt->K, opt->v and opt->B are ignored.
template <typename Drive>
int prepare_heston_smile(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *hs,
                         uint32_t n_expiries, uint32_t n_strikes, const uint32_t *h_expiry_steps, const double *h_strikes,
                         void *d_state, Drive drive)
{
    if (!opt || !sim || !hs || !h_expiry_steps || !h_strikes)
        return fail(MCAMD_ERR_INVALID, "opt, sim, heston, h_expiry_steps and h_strikes must be non-NULL");
    if (int rc = check_heston_job(opt, hs)) return rc;
    mcamd::HestonSmileJob job;
    if (int rc = check_smile_nodes(n_expiries, n_strikes, h_expiry_steps, sim->n_steps, h_strikes, hs->payoff, &job.nodes))
        return rc;
    if (int rc = check_heston_walk("Heston smile", opt, sim, hs, false, &job.walk)) return rc;
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    job.S0 = opt->S0;
    job.d_state = d_state;
    return drive(make_smile_call(ctx, sim, job.nodes, opt->r, job.walk.dt,
                                 smile_launch<mcamd::HestonSmileJob, mcamd::launch_heston_smile>, &job));
}

// The Heston cliquet calls: mcamd_price_heston's paths with mcamd_price_cliquet's payoff.  The refusals: what
// prepare_cliquet refuses before the surface (the job, then q, r, opt and sim at the drift r - cliquet->q), what
// prepare_heston refuses of the job and the model, the two dividend yields that must be one, then the context.  Once
// the yields agree prepare_heston's refusals of sim are the ones already made.  opt->v, opt->K and opt->B are ignored,
// S0 is read by nothing, and heston->payoff must be in range but is not read.
template <typename Drive>
int prepare_heston_cliquet(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *hs,
                           const mcamd_cliquet *cq, void *d_samples, Drive drive)
{
    if (!opt || !sim || !hs || !cq) return fail(MCAMD_ERR_INVALID, "opt, sim, heston and cliquet must be non-NULL");
    if (int rc = check_cliquet_job(cq, sim->n_steps)) return rc;
    if (!std::isfinite(cq->q)) return fail(MCAMD_ERR_INVALID, "the dividend yield q must be finite, got %g", cq->q);
    if (!std::isfinite(opt->r)) return fail(MCAMD_ERR_INVALID, "option parameters must be finite with T > 0");
    // as prepare_cliquet, on a copy that carries no spot, strike or barrier of its own
    mcamd_option seen = *opt;
    seen.S0 = 1.0;
    seen.K = seen.B = 0.0;
    const double mu = opt->r - cq->q;
    if (int rc = check_drift_request("Heston cliquet", seen, sim, &mu, 1)) return rc;
    if (int rc = check_heston_job(opt, hs)) return rc;
    if (std::memcmp(&cq->q, &hs->q, sizeof(double)) != 0)
        return fail(MCAMD_ERR_INVALID, "cliquet->q = %.17g and heston->q = %.17g must be the same dividend yield, bit for bit",
                    cq->q, hs->q);
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (sim->n_paths_local == 0) return drive(empty_call());
    mcamd::HestonCliquetJob job;
    job.walk = heston_walk(opt, sim, hs);
    job.kind = cq->kind;
    job.reset_every = cq->reset_every;
    job.first_period = cq->first_period;
    const bool compound = cq->kind == MCAMD_CLIQUET_COMPOUND;
    job.local_lo = compound ? std::log(1.0 + cq->local_floor) : cq->local_floor;
    job.local_hi = compound ? std::log(1.0 + cq->local_cap) : cq->local_cap;
    job.global_lo = cq->global_floor;
    job.global_hi = cq->global_cap;
    const double P = static_cast<double>(sim->n_steps / cq->reset_every - cq->first_period + 1);
    job.scale = 1.0 / (P * (static_cast<double>(cq->reset_every) * job.walk.dt));
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(sim->n_paths_local);
    return drive(DeviceCall{sim->n_paths_local, grid, mcamd::kHestonCliquetRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_heston_cliquet(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

// The Heston barrier calls: mcamd_price_heston's paths with mcamd_price_barrier's tests and samples.  The refusals:
// what prepare_barrier refuses of the barrier (monitoring, reserved, then kind, payoff, B and the side of S0), what
// prepare_heston refuses (the job and the model, r, opt's other fields, sim->flags and sim at the drift r - q, S0 and K),
// the two payoffs that must be one, then the context.  opt->v is ignored.
template <typename Drive>
int prepare_heston_barrier(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *hs,
                           const mcamd_barrier *bar, void *d_samples, void *d_state, Drive drive)
{
    if (!opt || !sim || !hs || !bar) return fail(MCAMD_ERR_INVALID, "opt, sim, heston and barrier must be non-NULL");
    if (int rc = check_barrier_terms(bar, opt->S0, opt->B)) return rc;
    if (int rc = check_heston_job(opt, hs)) return rc;
    mcamd::HestonBarrierJob job;
    if (int rc = check_heston_walk("Heston barrier", opt, sim, hs, true, &job.walk)) return rc;
    if (hs->payoff != bar->payoff)
        return fail(MCAMD_ERR_INVALID, "heston->payoff = %d and barrier->payoff = %d must be the same payoff", hs->payoff,
                    bar->payoff);
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (sim->n_paths_local == 0) return drive(empty_call());
    job.S0 = opt->S0;
    job.K = opt->K;
    job.B = opt->B;
    job.form = barrier_form(bar->kind, bar->monitoring, bar->payoff);
    job.d_samples = d_samples;
    job.d_state = d_state;
    const uint32_t grid = mcamd::one_path_per_thread_grid(sim->n_paths_local);
    return drive(DeviceCall{sim->n_paths_local, grid, mcamd::kHestonBarrierRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_heston_barrier(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

// ---- the Heston Greeks (include/mcamd_heston_greeks.h) ---------------------------------------------------------------

const char *const kGreekParam[mcamd::kHestonGreeksMaxParams] = {"v0", "kappa", "theta", "xi", "rho"};

// What the Greeks calls and their finalize refuse of the job alone: reserved, gamma_eta, the bumps.
int check_heston_greeks_job(const mcamd_heston_greeks_job *gj)
{
    if (gj->reserved != 0.0) return fail(MCAMD_ERR_INVALID, "job->reserved must be 0, got %g", gj->reserved);
    if (!std::isfinite(gj->gamma_eta) || gj->gamma_eta < 0.0)
        return fail(MCAMD_ERR_INVALID, "gamma_eta must be finite and >= 0 (0: no gamma), got %g", gj->gamma_eta);
    for (int k = 0; k < mcamd::kHestonGreeksMaxParams; ++k)
        if (!std::isfinite(gj->bump[k]) || gj->bump[k] < 0.0)
            return fail(MCAMD_ERR_INVALID, "bump[%d] (of %s) must be finite and >= 0 (0: not requested), got %g", k,
                        kGreekParam[k], gj->bump[k]);
    return MCAMD_OK;
}

// the model with parameter k (0 .. 4: v0, kappa, theta, xi, rho) moved by delta, formed in double
mcamd_heston bumped_heston(const mcamd_heston &hs, int k, double delta)
{
    mcamd_heston b = hs;
    double *const field[mcamd::kHestonGreeksMaxParams] = {&b.v0, &b.kappa, &b.theta, &b.xi, &b.rho};
    *field[k] = *field[k] + delta;
    return b;
}

// The Greeks calls: prepare_heston's refusals, then the job's own, then every bumped model, then the context.  The
// kernel finishes its own sum into the 32-double statistics record.  opt->v and opt->B are ignored.
template <typename Drive>
int prepare_heston_greeks(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *hs,
                          const mcamd_heston_greeks_job *gj, void *d_samples, Drive drive)
{
    if (!opt || !sim || !hs) return fail(MCAMD_ERR_INVALID, "opt, sim and heston must be non-NULL");
    if (int rc = check_heston_job(opt, hs)) return rc;
    mcamd::HestonGreeksJob job;
    if (int rc = check_heston_walk("Heston Greeks", opt, sim, hs, true, &job.walk[0])) return rc;
    if (!gj) return fail(MCAMD_ERR_INVALID, "job is NULL");
    if (int rc = check_heston_greeks_job(gj)) return rc;
    job.n_params = 0;
    for (int k = 0; k < mcamd::kHestonGreeksMaxParams; ++k) {
        if (!(gj->bump[k] > 0.0)) continue;
        for (int side = 0; side < 2; ++side) {
            const mcamd_heston b = bumped_heston(*hs, k, side == 0 ? gj->bump[k] : -gj->bump[k]);
            if (check_heston_model(b.q, b.v0, b.kappa, b.theta, b.xi, b.rho)) {
                char why[256];
                std::snprintf(why, sizeof why, "%s", mcamd_last_error());
                const double base[mcamd::kHestonGreeksMaxParams] = {hs->v0, hs->kappa, hs->theta, hs->xi, hs->rho};
                return fail(MCAMD_ERR_INVALID, "%s %c bump[%d] = %g %c %g leaves the model: %s", kGreekParam[k],
                            side == 0 ? '+' : '-', k, base[k], side == 0 ? '+' : '-', gj->bump[k], why);
            }
            job.walk[1 + 2 * job.n_params + side] = heston_walk(opt, sim, &b);
        }
        job.n_params++;
    }
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (sim->n_paths_local == 0) return drive(empty_call(mcamd::kHestonGreeksStats));
    job.S0 = opt->S0;
    job.K = opt->K;
    job.put = hs->payoff == MCAMD_PAYOFF_PUT;
    job.gamma_eta = gj->gamma_eta;
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(sim->n_paths_local);
    return drive(DeviceCall{sim->n_paths_local, grid, mcamd::heston_greeks_record(job.n_params), mcamd::kHestonGreeksStats,
                            Finish::kFolded, [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_heston_greeks(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

// value / std_err of a (possibly all-reduced) 32-double Greeks record; S0, r and T of the option, eta and the bumps of
// the job (checked by the caller).  Fills value, std_err, n, truncated_steps and mean_variance.
void finalize_heston_greeks_into(const double stats[MCAMD_HESTON_GREEKS_STATS], double S0, double r, double T,
                                 const mcamd_heston_greeks_job *gj, mcamd_heston_greeks *out)
{
    int P = 0;
    for (int k = 0; k < mcamd::kHestonGreeksMaxParams; ++k) P += gj->bump[k] > 0.0 ? 1 : 0;
    const double disc = std::exp(-r * T);
    const uint64_t n = static_cast<uint64_t>(std::llround(stats[9 + 2 * P]));
    const auto set = [&](int which, double sum, double sumsq, double factor) {
        const Estimate e = estimate(sum, sumsq, n, disc);
        out->value[which] = factor * e.value;
        out->std_err[which] = std::fabs(factor) * e.std_err;
    };
    out->n = n;
    set(MCAMD_HESTON_GREEK_PRICE, stats[0], stats[1], 1.0);
    set(MCAMD_HESTON_GREEK_DELTA, stats[2], stats[3], 1.0 / S0);
    if (gj->gamma_eta > 0.0)
        set(MCAMD_HESTON_GREEK_GAMMA, stats[5], stats[6],
            1.0 / (S0 * S0 * (std::exp(gj->gamma_eta) - std::exp(-gj->gamma_eta))));
    set(MCAMD_HESTON_GREEK_RHO, stats[2] - stats[0], stats[4], T);
    set(MCAMD_HESTON_GREEK_RHO_Q, stats[2], stats[3], -T);
    for (int k = 0, j = 0; k < mcamd::kHestonGreeksMaxParams; ++k) {
        if (!(gj->bump[k] > 0.0)) continue;
        set(MCAMD_HESTON_GREEK_V0 + k, stats[7 + 2 * j], stats[8 + 2 * j], 1.0 / (2.0 * gj->bump[k]));
        ++j;
    }
    out->truncated_steps = stats[7 + 2 * P];
    out->mean_variance = n ? stats[8 + 2 * P] / static_cast<double>(n) : 0.0;
}

}  // namespace

extern "C" {

int mcamd_price_heston_greeks(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *heston,
                              const mcamd_heston_greeks_job *job, void *d_samples, mcamd_heston_greeks *out)
{
    if (!out) return fail(MCAMD_ERR_INVALID, "opt, sim, heston, job and out must be non-NULL");
    std::memset(out, 0, sizeof *out);
    return prepare_heston_greeks(ctx, opt, sim, heston, job, d_samples, [&](const auto &call) {
        return run_sync(ctx, call, out, [&](const double *stats) {
            finalize_heston_greeks_into(stats, opt->S0, opt->r, opt->T, job, out);
            out->work_steps = full_walk_work_steps(sim->n_paths_local, sim->n_steps);
        });
    });
}

int mcamd_price_heston_greeks_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                      const mcamd_heston *heston, const mcamd_heston_greeks_job *job, void *d_samples,
                                      double *d_stats)
{
    return prepare_heston_greeks(ctx, opt, sim, heston, job, d_samples,
                                 [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

int mcamd_finalize_heston_greeks_stats(const double stats[32], const mcamd_option *opt,
                                       const mcamd_heston_greeks_job *job, mcamd_heston_greeks *out)
{
    if (!stats || !opt || !job || !out) return fail(MCAMD_ERR_INVALID, "stats, opt, job and out must be non-NULL");
    std::memset(out, 0, sizeof *out);
    if (int rc = check_heston_greeks_job(job)) return rc;
    if (!(opt->S0 > 0.0) || !std::isfinite(opt->S0) || !std::isfinite(opt->T) || !std::isfinite(opt->r))
        return fail(MCAMD_ERR_INVALID, "the Heston Greeks need S0 > 0 and finite S0, T and r (S0 = %g, T = %g, r = %g)",
                    opt->S0, opt->T, opt->r);
    finalize_heston_greeks_into(stats, opt->S0, opt->r, opt->T, job, out);
    return MCAMD_OK;
}

int mcamd_price_heston(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *heston,
                       void *d_samples, void *d_state, mcamd_heston_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim, heston and res must be non-NULL");
    std::memset(res, 0, sizeof *res);
    return prepare_heston(ctx, opt, sim, heston, d_samples, d_state, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) {
            // {sum, sumsq, lane-steps entered with v < 0, sum of the paths' average variance}
            const uint64_t n = sim->n_paths_local;
            finalize_into(rec[0], rec[1], n, opt->r, opt->T, res);
            res->truncated_steps = rec[2];
            res->mean_variance = rec[3] / static_cast<double>(n);
            res->work_steps = full_walk_work_steps(n, sim->n_steps);
        });
    });
}

int mcamd_price_heston_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *heston,
                               void *d_samples, void *d_state, double *d_stats)
{
    return prepare_heston(ctx, opt, sim, heston, d_samples, d_state,
                          [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

int mcamd_price_heston_smile(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *heston,
                             uint32_t n_expiries, uint32_t n_strikes, const uint32_t *h_expiry_steps,
                             const double *h_strikes, void *d_state, double *h_stats, mcamd_result *res)
{
    if (!res || !h_stats) return fail(MCAMD_ERR_INVALID, "h_stats and res must be non-NULL");
    zero_result(res);
    return prepare_heston_smile(ctx, opt, sim, heston, n_expiries, n_strikes, h_expiry_steps, h_strikes, d_state,
                                [&](const SmileCall &call) { return run_smile_sync(ctx, call, h_stats, res); });
}

int mcamd_price_heston_smile_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                     const mcamd_heston *heston, uint32_t n_expiries, uint32_t n_strikes,
                                     const uint32_t *h_expiry_steps, const double *h_strikes, void *d_state,
                                     double *d_stats)
{
    if (!d_stats) return fail(MCAMD_ERR_INVALID, "d_stats is NULL");
    return prepare_heston_smile(ctx, opt, sim, heston, n_expiries, n_strikes, h_expiry_steps, h_strikes, d_state,
                                [&](const SmileCall &call) { return run_smile_enqueue(ctx, call, d_stats); });
}

int mcamd_price_heston_cliquet(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *heston,
                               const mcamd_cliquet *cliquet, void *d_samples, mcamd_heston_cliquet_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim, heston, cliquet and res must be non-NULL");
    std::memset(res, 0, sizeof *res);
    return prepare_heston_cliquet(ctx, opt, sim, heston, cliquet, d_samples, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) {
            // {sum, sumsq, paths on the global floor, paths on the global cap, sum of the paths' average variance,
            // lane-steps entered with v < 0}
            const uint64_t n = sim->n_paths_local;
            finalize_into(rec[0], rec[1], n, opt->r, opt->T, res);
            res->n_floored = static_cast<uint64_t>(std::llround(rec[2]));
            res->n_capped = static_cast<uint64_t>(std::llround(rec[3]));
            res->mean_variance = rec[4] / static_cast<double>(n);
            res->truncated_steps = rec[5];
            res->work_steps = full_walk_work_steps(n, sim->n_steps);
        });
    });
}

int mcamd_price_heston_cliquet_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                       const mcamd_heston *heston, const mcamd_cliquet *cliquet, void *d_samples,
                                       double *d_stats)
{
    return prepare_heston_cliquet(ctx, opt, sim, heston, cliquet, d_samples,
                                  [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

int mcamd_price_heston_barrier(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *heston,
                               const mcamd_barrier *barrier, void *d_samples, void *d_state,
                               mcamd_heston_barrier_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim, heston, barrier and res must be non-NULL");
    std::memset(res, 0, sizeof *res);
    return prepare_heston_barrier(ctx, opt, sim, heston, barrier, d_samples, d_state, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) {
            // {sum, sumsq, live lane-steps, counted lane-steps entered with v < 0, sum of v+ over the counted
            // lane-steps, wave-steps}
            const uint64_t n = sim->n_paths_local;
            finalize_into(rec[0], rec[1], n, opt->r, opt->T, res);
            res->live_steps = rec[2];
            res->work_steps = 64.0 * rec[5];
            res->truncated_steps = rec[3];
            // the steps that count: a knock-in's all, a knock-out's live ones (every path enters its first step live)
            const double counted = barrier_sides(barrier->kind).out
                                       ? rec[2]
                                       : static_cast<double>(n) * static_cast<double>(sim->n_steps);
            res->mean_variance = rec[4] / counted;
        });
    });
}

int mcamd_price_heston_barrier_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                       const mcamd_heston *heston, const mcamd_barrier *barrier, void *d_samples,
                                       void *d_state, double *d_stats)
{
    return prepare_heston_barrier(ctx, opt, sim, heston, barrier, d_samples, d_state,
                                  [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

}  // extern "C"
