// capi_multi.cpp — the multi-asset calls of the C ABI under constant volatilities: basket (spread, rainbow) options
// and worst-of autocallable notes, each a prepare_* step (the refusals and the job) and its synchronous and enqueue
// forms.  The autocallable under local-volatility surfaces is capi_localvol.cpp's.
#include "capi_internal.hpp"
#include "basket.hpp"
#include "autocall.hpp"

static_assert(sizeof(mcamd_basket) == 728, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_autocall) == 632 && sizeof(mcamd_autocall_result) == 112,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(MCAMD_AUTOCALL_MAX_DATES == mcamd::kAutocallMaxDates, "the kernel's date tables hold MCAMD_AUTOCALL_MAX_DATES");

using namespace mcamd::capi;

namespace mcamd::capi {

// The refusals of the basket calls that depend on the assets alone (shared with the geometric closed form and both
// autocall calls).  Leaves the lower Cholesky factor of corr[:d, :d] in L (row-major, stride 8; entries above the
// diagonal 0).
int check_basket_assets(const mcamd_basket *b, bool positive_weights, double L[64])
{
    const int d = b->n_assets;
    if (d < 1 || d > MCAMD_BASKET_MAX_ASSETS)
        return fail(MCAMD_ERR_INVALID, "n_assets must be 1..%d, got %d", MCAMD_BASKET_MAX_ASSETS, d);
    if (int rc = check_payoff(b->payoff)) return rc;
    bool any_weight = false;
    for (int j = 0; j < d; ++j) {
        if (!(b->S0[j] > 0.0) || !std::isfinite(b->S0[j]) || !(b->v[j] > 0.0) || !std::isfinite(b->v[j]))
            return fail(MCAMD_ERR_INVALID, "basket assets need finite S0 > 0 and v > 0 (asset %d: S0 = %g, v = %g)", j,
                        b->S0[j], b->v[j]);
        if (!std::isfinite(b->w[j])) return fail(MCAMD_ERR_INVALID, "basket weight %d is not finite", j);
        if (positive_weights && !(b->w[j] > 0.0))
            return fail(MCAMD_ERR_INVALID, "best-of and worst-of need every weight > 0 (w[%d] = %g)", j, b->w[j]);
        any_weight = any_weight || b->w[j] != 0.0;
    }
    if (!any_weight) return fail(MCAMD_ERR_INVALID, "every basket weight is 0");
    for (int j = 0; j < d; ++j) {
        if (b->corr[8 * j + j] != 1.0)
            return fail(MCAMD_ERR_INVALID, "corr[%d][%d] must be exactly 1, got %g", j, j, b->corr[8 * j + j]);
        for (int k = 0; k < j; ++k) {
            const double rho = b->corr[8 * j + k];
            if (rho != b->corr[8 * k + j])
                return fail(MCAMD_ERR_INVALID, "corr must be exactly symmetric: [%d][%d] = %g, [%d][%d] = %g", j, k, rho,
                            k, j, b->corr[8 * k + j]);
            if (!(rho >= -1.0 && rho <= 1.0))
                return fail(MCAMD_ERR_INVALID, "corr[%d][%d] = %g lies beyond +-1", j, k, rho);
        }
    }
    std::memset(L, 0, 64 * sizeof(double));
    for (int j = 0; j < d; ++j) {
        for (int k = 0; k <= j; ++k) {
            double s = b->corr[8 * j + k];
            for (int q = 0; q < k; ++q) s -= L[8 * j + q] * L[8 * k + q];
            if (k < j) {
                L[8 * j + k] = s / L[8 * k + k];
            } else {
                if (!(s > 1e-12))
                    return fail(MCAMD_ERR_INVALID, "corr is not positive definite: Cholesky pivot %d is %g (must exceed "
                                                   "1e-12; a correlation of +-1 is refused: use fewer assets)", j, s);
                L[8 * j + j] = std::sqrt(s);
            }
        }
    }
    return MCAMD_OK;
}

// The refusals of the autocall calls that depend on the note's terms alone (shared with the closed form); L_last is the
// autocall level of the last date.
int check_autocall_terms(double coupon, double call_level, double call_step_down, double L_last, int ki_monitoring,
                         double ki_level)
{
    if (ki_monitoring < MCAMD_AUTOCALL_KI_NONE || ki_monitoring > MCAMD_AUTOCALL_KI_EVERY_STEP)
        return fail(MCAMD_ERR_INVALID, "ki_monitoring must be MCAMD_AUTOCALL_KI_NONE (0) .. MCAMD_AUTOCALL_KI_EVERY_STEP "
                                       "(2), got %d", ki_monitoring);
    if (!std::isfinite(coupon) || !(coupon >= 0.0))
        return fail(MCAMD_ERR_INVALID, "the coupon must be finite and >= 0, got %g", coupon);
    if (!std::isfinite(call_level)) return fail(MCAMD_ERR_INVALID, "call_level must be finite, got %g", call_level);
    if (!std::isfinite(call_step_down) || !(call_step_down >= 0.0))
        return fail(MCAMD_ERR_INVALID, "call_step_down must be finite and >= 0, got %g", call_step_down);
    if (!(L_last > 0.0))
        return fail(MCAMD_ERR_INVALID, "the autocall level of the last date must be positive, got %g", L_last);
    if (ki_monitoring != MCAMD_AUTOCALL_KI_NONE && (!(ki_level > 0.0) || !(ki_level <= 1.0) || !(ki_level < L_last)))
        return fail(MCAMD_ERR_INVALID, "ki_level must lie in (0, 1] and below the autocall level of the last date "
                                       "(ki_level = %g, last level = %g)", ki_level, L_last);
    return MCAMD_OK;
}

int check_autocall_assets(int n_assets, const double *v, const double corr[64], double L[64])
{
    mcamd_basket assets{};
    assets.n_assets = n_assets;
    assets.payoff = MCAMD_PAYOFF_PUT;
    for (int j = 0; j < MCAMD_BASKET_MAX_ASSETS; ++j) {
        assets.S0[j] = assets.w[j] = 1.0;
        assets.v[j] = v ? v[j] : 1.0;
    }
    std::memcpy(assets.corr, corr, sizeof assets.corr);
    return check_basket_assets(&assets, true, L);
}

int check_autocall_schedule(const AutocallTerms &t, uint32_t n_steps, uint32_t *M_out)
{
    if (t.observe_every == 0 || n_steps % t.observe_every != 0)
        return fail(MCAMD_ERR_INVALID, "observe_every must be >= 1 and divide n_steps (observe_every = %u, n_steps = %u)",
                    t.observe_every, n_steps);
    const uint32_t M = *M_out = n_steps / t.observe_every;
    if (M > MCAMD_AUTOCALL_MAX_DATES)   // M == 0 is n_steps == 0, which check_request refuses later
        return fail(MCAMD_ERR_INVALID, "n_steps / observe_every = %u observation dates exceed MCAMD_AUTOCALL_MAX_DATES = %d",
                    M, MCAMD_AUTOCALL_MAX_DATES);
    if (M != 0 && (t.first_call_date < 1 || t.first_call_date > M))
        return fail(MCAMD_ERR_INVALID, "first_call_date must be 1..%u (the observation dates), got %u", M,
                    t.first_call_date);
    const double L_last = t.call_level - (static_cast<double>(M) - 1.0) * t.call_step_down;
    return check_autocall_terms(t.coupon, t.call_level, t.call_step_down, M ? L_last : t.call_level, t.ki_monitoring,
                                t.ki_level);
}

void make_autocall_schedule(const AutocallTerms &t, uint32_t M, double r, double T, double dt,
                            mcamd::AutocallSchedule *schedule)
{
    mcamd::AutocallSchedule &s = *schedule;
    s.observe_every = t.observe_every;
    s.n_dates = M;
    s.first_call_date = t.first_call_date;
    for (uint32_t q = 1; q <= M; ++q) {
        const double t_q = static_cast<double>(q * t.observe_every) * dt;
        s.log_level[q - 1] = std::log(t.call_level - (static_cast<double>(q) - 1.0) * t.call_step_down);
        s.pay[q - 1] = (1.0 + static_cast<double>(q) * t.coupon) * std::exp(r * (T - t_q));
    }
    s.dt = dt;
    s.ki = t.ki_monitoring != MCAMD_AUTOCALL_KI_NONE;
    s.ki_every_step = t.ki_monitoring == MCAMD_AUTOCALL_KI_EVERY_STEP;
    s.log_ki = s.ki ? std::log(t.ki_level) : 0.0;
}

void fill_autocall_result(const double *rec, uint64_t n, double r, double T, mcamd_autocall_result *res)
{
    finalize_into(rec[0], rec[1], n, r, T, res);
    res->n_called = static_cast<uint64_t>(std::llround(rec[2]));
    res->sum_t_call = rec[3];
    res->n_knocked_in = static_cast<uint64_t>(std::llround(rec[4]));
    res->work_steps = 64.0 * rec[5];   // wave-steps x 64 lanes
    res->live_steps = rec[6];
}

}  // namespace mcamd::capi

namespace {

// The basket calls.  The kernel always finishes its own sum (one_path_per_thread_grid caps the grid); every refusal
// that depends on the request alone comes before the context is looked at.
template <typename Drive>
int prepare_basket(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_basket *bk,
                   void *d_samples, Drive drive)
{
    if (!opt || !sim || !bk) return fail(MCAMD_ERR_INVALID, "opt, sim and basket must be non-NULL");
    if (bk->kind < MCAMD_BASKET_ARITHMETIC || bk->kind > MCAMD_BASKET_WORST_OF)
        return fail(MCAMD_ERR_INVALID, "basket kind must be MCAMD_BASKET_ARITHMETIC (0) .. MCAMD_BASKET_WORST_OF (3), "
                                       "got %d", bk->kind);
    if (bk->barrier < MCAMD_BASKET_NO_BARRIER || bk->barrier > MCAMD_BASKET_UP_IN)
        return fail(MCAMD_ERR_INVALID, "basket barrier must be MCAMD_BASKET_NO_BARRIER (0) .. MCAMD_BASKET_UP_IN (4), "
                                       "got %d", bk->barrier);
    if (bk->reserved[0] != 0 || bk->reserved[1] != 0)
        return fail(MCAMD_ERR_INVALID, "basket->reserved must be 0, got {%d, %d}", bk->reserved[0], bk->reserved[1]);
    const bool extreme = bk->kind == MCAMD_BASKET_BEST_OF || bk->kind == MCAMD_BASKET_WORST_OF;
    double L[64];
    if (int rc = check_basket_assets(bk, extreme, L)) return rc;
    if (!std::isfinite(opt->K) || !(opt->K >= 0.0))
        return fail(MCAMD_ERR_INVALID, "a basket option needs a finite K >= 0, got %g", opt->K);
    const int d = bk->n_assets;
    const bool monitored = bk->barrier != MCAMD_BASKET_NO_BARRIER;
    const bool up = bk->barrier == MCAMD_BASKET_UP_OUT || bk->barrier == MCAMD_BASKET_UP_IN;
    if (monitored) {
        if (!extreme)
            return fail(MCAMD_ERR_INVALID, "a basket barrier needs MCAMD_BASKET_BEST_OF or MCAMD_BASKET_WORST_OF, got "
                                           "kind %d", bk->kind);
        if (!(opt->B > 0.0) || !std::isfinite(opt->B))
            return fail(MCAMD_ERR_INVALID, "the barrier level B must be positive, got %g", opt->B);
        double A0 = bk->w[0] * bk->S0[0];
        for (int j = 1; j < d; ++j)
            A0 = bk->kind == MCAMD_BASKET_BEST_OF ? std::fmax(A0, bk->w[j] * bk->S0[j]) : std::fmin(A0, bk->w[j] * bk->S0[j]);
        if (!std::isfinite(A0) || !(up ? A0 < opt->B : A0 > opt->B))
            return fail(MCAMD_ERR_INVALID, "the aggregate must start strictly on the live side of the barrier: %s "
                                           "(A_0 = %g, B = %g)", up ? "an up-barrier needs A_0 < B" : "a down-barrier needs A_0 > B",
                        A0, opt->B);
    }
    // what the option itself contributes is r, T, K and B: the spot-start rules and those of mcamd_price_paths see the
    // first asset in the place of opt->S0 and opt->v, which are ignored
    mcamd_option seen = *opt;
    seen.S0 = bk->S0[0];
    seen.v = bk->v[0];
    if (!monitored) seen.B = 0.0;
    if (int rc = check_spot_start("basket", false, &seen, sim)) return rc;
    for (int j = 0; j < d; ++j) {   // the fp64 exponent range, asset by asset: |x_j| <= |drift_j| + v_j sqrt(dt) sqrt(d) max_k |z_k|
                                    // (a row of L has unit length)
        seen.v = bk->v[j] * std::sqrt(static_cast<double>(d));
        if (int rc = check_request(&seen, sim)) return rc;
        seen.v = bk->v[j];
        if (int rc = check_request(&seen, sim)) return rc;
    }
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (sim->n_paths_local == 0) return drive(empty_call());
    mcamd::BasketJob job{};
    job.path = make_plain_job(&seen, sim, false, true);
    job.d = d;
    job.kind = bk->kind;
    job.put = bk->payoff == MCAMD_PAYOFF_PUT;
    job.monitored = monitored;
    job.up = up;
    job.out = bk->barrier == MCAMD_BASKET_DOWN_OUT || bk->barrier == MCAMD_BASKET_UP_OUT;
    const double dt = even_dt(opt, sim), sqdt = std::sqrt(dt);
    double log_sum = 0.0;
    for (int j = 0; j < d; ++j) {
        job.drift[j] = (opt->r - 0.5 * bk->v[j] * bk->v[j]) * dt;
        for (int k = 0; k <= j; ++k) job.coef[j * (j + 1) / 2 + k] = bk->v[j] * sqdt * L[8 * j + k];
        job.S0[j] = bk->S0[j];
        job.w[j] = bk->w[j];
        job.log_w[j] = extreme ? std::log(bk->w[j] * bk->S0[j]) : 0.0;
        log_sum += bk->w[j] * std::log(bk->S0[j]);
    }
    if (bk->kind == MCAMD_BASKET_GEOMETRIC) job.log_w[0] = log_sum;
    job.K = opt->K;
    job.logB = monitored ? std::log(opt->B) : 0.0;
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(job.path.n_local);
    return drive(DeviceCall{job.path.n_local, grid, mcamd::kBasketRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_basket(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

// The autocall calls.  The kernel always finishes its own sum (one_path_per_thread_grid caps the grid); every refusal
// that depends on the request alone comes before the context is looked at.
template <typename Drive>
int prepare_autocall(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_autocall *ac,
                     void *d_samples, Drive drive)
{
    if (!opt || !sim || !ac) return fail(MCAMD_ERR_INVALID, "opt, sim and autocall must be non-NULL");
    if (ac->reserved[0] != 0 || ac->reserved[1] != 0)
        return fail(MCAMD_ERR_INVALID, "autocall->reserved must be 0, got {%d, %d}", ac->reserved[0], ac->reserved[1]);
    // the assets through the basket's own checks and Cholesky factor
    double L[64];
    if (int rc = check_autocall_assets(ac->n_assets, ac->v, ac->corr, L)) return rc;
    const int d = ac->n_assets;
    const AutocallTerms terms = autocall_terms(ac);
    uint32_t M;
    if (int rc = check_autocall_schedule(terms, sim->n_steps, &M)) return rc;
    // what the option itself contributes is r and T: the spot-start rules and those of mcamd_price_paths see a
    // performance (spot 1) with each asset's volatility in the place of opt->S0 and opt->v; K and B are ignored
    mcamd_option seen = *opt;
    seen.S0 = 1.0;
    seen.v = ac->v[0];
    seen.K = seen.B = 0.0;
    if (int rc = check_spot_start("autocallable", false, &seen, sim)) return rc;
    for (int j = 0; j < d; ++j) {   // the fp64 exponent range, asset by asset, as prepare_basket bounds it
        seen.v = ac->v[j] * std::sqrt(static_cast<double>(d));
        if (int rc = check_request(&seen, sim)) return rc;
        seen.v = ac->v[j];
        if (int rc = check_request(&seen, sim)) return rc;
    }
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (sim->n_paths_local == 0) return drive(empty_call());
    mcamd::AutocallJob job{};
    job.path = make_plain_job(&seen, sim, false, true);
    job.d = d;
    const double dt = even_dt(opt, sim), sqdt = std::sqrt(dt);
    for (int j = 0; j < d; ++j) {
        job.drift[j] = (opt->r - 0.5 * ac->v[j] * ac->v[j]) * dt;
        for (int k = 0; k <= j; ++k) job.coef[j * (j + 1) / 2 + k] = ac->v[j] * sqdt * L[8 * j + k];
    }
    make_autocall_schedule(terms, M, opt->r, opt->T, dt, &job.schedule);
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(job.path.n_local);
    return drive(DeviceCall{job.path.n_local, grid, mcamd::kAutocallRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_autocall(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

}  // namespace

extern "C" {

int mcamd_price_basket(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_basket *basket,
                       void *d_samples, mcamd_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim, basket and res must be non-NULL");
    zero_result(res);
    return prepare_basket(ctx, opt, sim, basket, d_samples, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) {
            finalize_counted_into(rec, sim->n_paths_local, opt->r, opt->T, res);
        });
    });
}

int mcamd_price_basket_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                               const mcamd_basket *basket, void *d_samples, double *d_stats)
{
    return prepare_basket(ctx, opt, sim, basket, d_samples,
                          [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

int mcamd_price_autocall(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_autocall *autocall,
                         void *d_samples, mcamd_autocall_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim, autocall and res must be non-NULL");
    std::memset(res, 0, sizeof *res);
    return prepare_autocall(ctx, opt, sim, autocall, d_samples, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) {
            fill_autocall_result(rec, sim->n_paths_local, opt->r, opt->T, res);
        });
    });
}

int mcamd_price_autocall_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                 const mcamd_autocall *autocall, void *d_samples, double *d_stats)
{
    return prepare_autocall(ctx, opt, sim, autocall, d_samples,
                            [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

}  // extern "C"
