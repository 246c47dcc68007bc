// capi_pathdep.cpp — the path-dependent single-asset calls of the C ABI: barrier, lookback and Asian options, each a
// prepare_* step (the refusals and the job) and its synchronous and enqueue forms.
#include "capi_internal.hpp"
#include "barrier.hpp"
#include "lookback.hpp"
#include "asian.hpp"

static_assert(sizeof(mcamd_barrier) == 16, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_lookback) == 16, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_asian) == 24, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");

using namespace mcamd::capi;

namespace mcamd::capi {

// What the barrier, lookback, local-volatility and Heston barrier calls refuse of a monitoring.
int check_monitoring(int monitoring)
{
    if (monitoring != MCAMD_MONITOR_DISCRETE && monitoring != MCAMD_MONITOR_CONTINUOUS)
        return fail(MCAMD_ERR_INVALID, "monitoring must be MCAMD_MONITOR_DISCRETE (0) or MCAMD_MONITOR_CONTINUOUS (1), "
                                       "got %d", monitoring);
    return MCAMD_OK;
}

// The refusals of the barrier calls that depend on the request's enums and levels alone (shared with the closed form
// and the local-volatility call).
int check_barrier_kind(double S0, double B, int kind, int payoff)
{
    if (kind < MCAMD_BARRIER_DOWN_OUT || kind > MCAMD_BARRIER_UP_IN)
        return fail(MCAMD_ERR_INVALID, "barrier kind must be MCAMD_BARRIER_DOWN_OUT (0) .. MCAMD_BARRIER_UP_IN (3), got %d",
                    kind);
    if (int rc = check_payoff(payoff)) return rc;
    if (!(B > 0.0) || !std::isfinite(B)) return fail(MCAMD_ERR_INVALID, "the barrier level B must be positive, got %g", B);
    const bool up = barrier_sides(kind).up;
    if (!(S0 > 0.0) || !std::isfinite(S0) || !(up ? S0 < B : S0 > B))
        return fail(MCAMD_ERR_INVALID, "the spot must lie strictly on the live side of the barrier: %s (S0 = %g, B = %g)",
                    up ? "an up-barrier needs 0 < S0 < B" : "a down-barrier needs S0 > B", S0, B);
    return MCAMD_OK;
}

int check_barrier_terms(const mcamd_barrier *bar, double S0, double B)
{
    if (int rc = check_monitoring(bar->monitoring)) return rc;
    if (bar->reserved != 0) return fail(MCAMD_ERR_INVALID, "barrier->reserved must be 0, got %d", bar->reserved);
    return check_barrier_kind(S0, B, bar->kind, bar->payoff);
}

mcamd::BarrierForm barrier_form(int kind, int monitoring, int payoff)
{
    const BarrierSides sides = barrier_sides(kind);   // neither up nor out outside MCAMD_BARRIER_*
    const bool barrier = kind >= MCAMD_BARRIER_DOWN_OUT && kind <= MCAMD_BARRIER_UP_IN;
    return {sides.up, sides.out, barrier && monitoring == MCAMD_MONITOR_CONTINUOUS, payoff == MCAMD_PAYOFF_PUT};
}

// The refusals of the lookback calls that depend on the product alone (shared with the closed form).
int check_lookback_kind(double K, int strike, int payoff)
{
    if (strike != MCAMD_LOOKBACK_FLOATING && strike != MCAMD_LOOKBACK_FIXED)
        return fail(MCAMD_ERR_INVALID, "strike must be MCAMD_LOOKBACK_FLOATING (0) or MCAMD_LOOKBACK_FIXED (1), got %d",
                    strike);
    if (int rc = check_payoff(payoff)) return rc;
    if (strike == MCAMD_LOOKBACK_FIXED && (!(K > 0.0) || !std::isfinite(K)))
        return fail(MCAMD_ERR_INVALID, "a fixed-strike lookback needs a finite K > 0, got %g", K);
    return MCAMD_OK;
}

// The refusals of the Asian calls that depend on the product alone (shared with the closed form).
int check_asian_kind(double K, int strike, int payoff, int include_spot)
{
    if (strike != MCAMD_ASIAN_FIXED && strike != MCAMD_ASIAN_FLOATING)
        return fail(MCAMD_ERR_INVALID, "strike must be MCAMD_ASIAN_FIXED (0) or MCAMD_ASIAN_FLOATING (1), got %d", strike);
    if (int rc = check_payoff(payoff)) return rc;
    if (include_spot != 0 && include_spot != 1)
        return fail(MCAMD_ERR_INVALID, "include_spot must be 0 or 1, got %d", include_spot);
    if (strike == MCAMD_ASIAN_FIXED && (!(K > 0.0) || !std::isfinite(K)))
        return fail(MCAMD_ERR_INVALID, "a fixed-strike Asian option needs a finite K > 0, got %g", K);
    return MCAMD_OK;
}

}  // namespace mcamd::capi

namespace {

// The barrier calls.  The kernel always finishes its own sum (one_path_per_thread_grid caps the grid); every refusal
// that depends on the request alone comes before the context is looked at.
template <typename Drive>
int prepare_barrier(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_barrier *bar,
                    void *d_samples, Drive drive)
{
    if (!opt || !sim || !bar) return fail(MCAMD_ERR_INVALID, "opt, sim and barrier must be non-NULL");
    if (int rc = check_barrier_terms(bar, opt->S0, opt->B)) return rc;
    if (int rc = check_spot_start("barrier", false, opt, sim)) return rc;
    if (int rc = check_request(opt, sim)) return rc;
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (sim->n_paths_local == 0) return drive(empty_call());
    mcamd::BarrierJob job;
    job.path = make_plain_job(opt, sim, false, true);
    job.form = barrier_form(bar->kind, bar->monitoring, bar->payoff);
    job.kq = 2.0 / (opt->v * opt->v * even_dt(opt, sim));
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(job.path.n_local);
    return drive(DeviceCall{job.path.n_local, grid, mcamd::kBarrierRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_barrier(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

// The lookback calls.  The kernel always finishes its own sum (one_path_per_thread_grid caps the grid); every refusal
// that depends on the request alone comes before the context is looked at.
template <typename Drive>
int prepare_lookback(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_lookback *lb,
                     void *d_samples, Drive drive)
{
    if (!opt || !sim || !lb) return fail(MCAMD_ERR_INVALID, "opt, sim and lookback must be non-NULL");
    if (int rc = check_monitoring(lb->monitoring)) return rc;
    if (lb->reserved != 0) return fail(MCAMD_ERR_INVALID, "lookback->reserved must be 0, got %d", lb->reserved);
    if (int rc = check_lookback_kind(opt->K, lb->strike, lb->payoff)) return rc;
    if (int rc = check_spot_start("lookback", false, opt, sim)) return rc;
    const bool fixed = lb->strike == MCAMD_LOOKBACK_FIXED;
    mcamd_option seen = *opt;   // a floating strike ignores K, and every lookback ignores B
    if (!fixed) seen.K = 0.0;
    seen.B = 0.0;
    if (int rc = check_request(&seen, sim)) return rc;
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (sim->n_paths_local == 0) return drive(empty_call());
    mcamd::LookbackJob job;
    job.path = make_plain_job(&seen, sim, false, true);
    job.fixed = fixed;
    job.put = lb->payoff == MCAMD_PAYOFF_PUT;
    job.maximum = fixed ? !job.put : job.put;   // fixed call and floating put look at the maximum
    job.continuous = lb->monitoring == MCAMD_MONITOR_CONTINUOUS;
    job.K = seen.K;
    job.v2dt = opt->v * opt->v * even_dt(opt, sim);
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(job.path.n_local);
    return drive(DeviceCall{job.path.n_local, grid, mcamd::kLookbackRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_lookback(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

// The Asian calls.  The kernel always finishes its own sum (one_path_per_thread_grid caps the grid); every refusal
// that depends on the request alone comes before the context is looked at.
template <typename Drive>
int prepare_asian(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_asian *as, void *d_samples,
                  Drive drive)
{
    if (!opt || !sim || !as) return fail(MCAMD_ERR_INVALID, "opt, sim and asian must be non-NULL");
    if (as->average != MCAMD_ASIAN_ARITHMETIC && as->average != MCAMD_ASIAN_GEOMETRIC)
        return fail(MCAMD_ERR_INVALID, "average must be MCAMD_ASIAN_ARITHMETIC (0) or MCAMD_ASIAN_GEOMETRIC (1), got %d",
                    as->average);
    if (as->control != MCAMD_ASIAN_CONTROL_NONE && as->control != MCAMD_ASIAN_CONTROL_GEOMETRIC)
        return fail(MCAMD_ERR_INVALID, "control must be MCAMD_ASIAN_CONTROL_NONE (0) or MCAMD_ASIAN_CONTROL_GEOMETRIC "
                                       "(1), got %d", as->control);
    if (as->reserved != 0) return fail(MCAMD_ERR_INVALID, "asian->reserved must be 0, got %d", as->reserved);
    if (int rc = check_asian_kind(opt->K, as->strike, as->payoff, as->include_spot)) return rc;
    const bool arithmetic = as->average == MCAMD_ASIAN_ARITHMETIC;
    const bool control = as->control == MCAMD_ASIAN_CONTROL_GEOMETRIC;
    if (control && !arithmetic)
        return fail(MCAMD_ERR_INVALID, "the geometric control variate serves arithmetic jobs only: a geometric job takes "
                                       "control = MCAMD_ASIAN_CONTROL_NONE");
    if (int rc = check_spot_start("Asian", false, opt, sim)) return rc;
    const bool floating = as->strike == MCAMD_ASIAN_FLOATING;
    mcamd_option seen = *opt;   // a floating strike ignores K, and every Asian option ignores B
    if (floating) seen.K = 0.0;
    seen.B = 0.0;
    if (int rc = check_request(&seen, sim)) return rc;
    double control_mean = 0.0;
    if (control) {
        double geo;
        if (int rc = asian_geometric_price(opt->S0, seen.K, opt->T, opt->r, opt->v, sim->n_steps, as->include_spot,
                                           as->strike, as->payoff, &geo))
            return rc;
        control_mean = std::exp(opt->r * opt->T) * geo;
    }
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (sim->n_paths_local == 0) return drive(empty_call());
    mcamd::AsianJob job;
    job.path = make_plain_job(&seen, sim, false, true);
    job.arithmetic = arithmetic;
    job.control = control;
    job.floating = floating;
    job.put = as->payoff == MCAMD_PAYOFF_PUT;
    job.include_spot = as->include_spot != 0;
    job.K = seen.K;
    job.control_mean = control_mean;
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(job.path.n_local);
    return drive(DeviceCall{job.path.n_local, grid, mcamd::kAsianRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_asian(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

}  // namespace

extern "C" {

int mcamd_price_barrier(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_barrier *barrier,
                        void *d_samples, mcamd_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim, barrier and res must be non-NULL");
    zero_result(res);
    return prepare_barrier(ctx, opt, sim, barrier, d_samples, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) {
            finalize_counted_into(rec, sim->n_paths_local, opt->r, opt->T, res);
        });
    });
}

int mcamd_price_barrier_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                const mcamd_barrier *barrier, void *d_samples, double *d_stats)
{
    return prepare_barrier(ctx, opt, sim, barrier, d_samples,
                           [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

int mcamd_price_lookback(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_lookback *lookback,
                         void *d_samples, mcamd_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim, lookback and res must be non-NULL");
    zero_result(res);
    return prepare_lookback(ctx, opt, sim, lookback, d_samples, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) {
            finalize_counted_into(rec, sim->n_paths_local, opt->r, opt->T, res);
        });
    });
}

int mcamd_price_lookback_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                 const mcamd_lookback *lookback, void *d_samples, double *d_stats)
{
    return prepare_lookback(ctx, opt, sim, lookback, d_samples,
                            [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

int mcamd_price_asian(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_asian *asian,
                      void *d_samples, mcamd_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim, asian and res must be non-NULL");
    zero_result(res);
    return prepare_asian(ctx, opt, sim, asian, d_samples, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) {
            // {sum y, sum y^2, sum c, sum c^2, sum y c, wave-steps}
            finalize_record(rec, asian->control == MCAMD_ASIAN_CONTROL_GEOMETRIC, sim->n_paths_local, opt->r, opt->T, res);
            res->work_steps = 64.0 * rec[mcamd::kAsianRecord - 1];   // wave-steps x 64 lanes
        });
    });
}

int mcamd_price_asian_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_asian *asian,
                              void *d_samples, double *d_stats)
{
    return prepare_asian(ctx, opt, sim, asian, d_samples,
                         [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

}  // extern "C"
