// capi.cpp — the core of the C ABI declared in include/mcamd.h: the error string, context/scratch ownership, the
// request checks and host statistics every family shares (capi_internal.hpp), and the calls on plain paths: pricing,
// trajectories, nested MC, the array-driven pricer, reductions and Greeks.  The product families live in capi_*.cpp,
// the host formulas in closed_forms.cpp.  All device work is enqueued through the launchers of launch.hpp on the
// context's stream; there is no CPU fallback of any kind — a call either runs the gfx950 kernels or returns an error.
#include "capi_internal.hpp"
#include "greeks.hpp"

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

static_assert(sizeof(mcamd_option) == 88 && sizeof(mcamd_sim) == 48 && sizeof(mcamd_result) == 128 &&
                  sizeof(mcamd_device_info) == 384,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_greeks) == 224, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");

using namespace mcamd::capi;

namespace {

thread_local std::string g_last_error;

}  // namespace

// used by group.cpp: records the calling thread's last error message
int mcamd_set_error_(int code, const char *msg)
{
    g_last_error = msg ? msg : "";
    return code;
}

namespace mcamd::capi {

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

int check_payoff(int payoff)
{
    if (payoff != MCAMD_PAYOFF_CALL && payoff != MCAMD_PAYOFF_PUT)
        return fail(MCAMD_ERR_INVALID, "payoff must be MCAMD_PAYOFF_CALL (0) or MCAMD_PAYOFF_PUT (1), got %d", payoff);
    return MCAMD_OK;
}

int check_precision_steps(const mcamd_sim *sim)
{
    if (sim->precision != MCAMD_F32 && sim->precision != MCAMD_F64)
        return fail(MCAMD_ERR_INVALID, "precision must be MCAMD_F32 (32) or MCAMD_F64 (64), got %d", sim->precision);
    if (sim->n_steps == 0) return fail(MCAMD_ERR_INVALID, "n_steps must be >= 1");
    return MCAMD_OK;
}

int ensure_partials(mcamd_ctx *ctx, uint32_t records, int record_doubles)
{
    const uint64_t need = static_cast<uint64_t>(records) * record_doubles;
    if (need <= ctx->partial_capacity) return MCAMD_OK;
    if (ctx->d_partials) HIP_TRY(hipFree(ctx->d_partials));
    ctx->d_partials = nullptr;
    ctx->partial_capacity = 0;
    HIP_TRY(hipMalloc(&ctx->d_partials, need * sizeof(double)));
    ctx->partial_capacity = need;
    return MCAMD_OK;
}

int enqueue_empty_shard(mcamd_ctx *ctx, double *d_stats, uint32_t n)
{
    const uint32_t slot = static_cast<uint32_t>(ctx->n_enqueued % mcamd_ctx::kRing);
    HIP_TRY(hipMemsetAsync(d_stats, 0, n * sizeof(double), ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ring0[slot], ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ring1[slot], ctx->stream));
    ctx->n_enqueued++;
    return MCAMD_OK;
}

int ensure_partials_enqueued(mcamd_ctx *ctx, uint32_t records, int record_doubles)
{
    // wait for work that may still read the old buffer
    if (static_cast<uint64_t>(records) * record_doubles > ctx->partial_capacity) HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ensure_partials(ctx, records, record_doubles);
}

int overlap_failed(mcamd_ctx *ctx, int rc)
{
    ctx->overlap = false;
    return rc;
}

int overlap_begin(mcamd_ctx *ctx, uint32_t records, int record_doubles, int *lane)
{
    *lane = -1;
    // a capture records the caller's stream alone: the in-order path keeps the whole job inside it
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &capturing) != hipSuccess || capturing != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return MCAMD_OK;
    }
    if (!ctx->overlap_ready) {
        hipError_t e = hipSuccess;
        for (int l = 0; l < 2 && e == hipSuccess; ++l) {
            e = hipStreamCreateWithFlags(&ctx->lane_stream[l], hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->lane_reduced[l], hipEventDisableTiming);
        }
        if (e != hipSuccess) {   // mcamd_ctx_destroy frees what was created
            (void)hipGetLastError();
            return overlap_failed(ctx, MCAMD_OK);
        }
        ctx->overlap_ready = true;
    }
    const int l = static_cast<int>(ctx->n_overlapped % 2);
    const uint64_t need = static_cast<uint64_t>(records) * record_doubles;
    if (need > ctx->lane_capacity[l]) {
        // the old buffer may still be written by the lane's last kernel and read by its reduction on the caller's stream
        HIP_TRY(hipStreamSynchronize(ctx->lane_stream[0]));
        HIP_TRY(hipStreamSynchronize(ctx->lane_stream[1]));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->lane_partials[l]) HIP_TRY(hipFree(ctx->lane_partials[l]));
        ctx->lane_partials[l] = nullptr;
        ctx->lane_capacity[l] = 0;
        HIP_TRY(hipMalloc(&ctx->lane_partials[l], need * sizeof(double)));
        ctx->lane_capacity[l] = need;
    }
    const uint32_t slot = ring_slot(ctx->n_enqueued);
    hipError_t e = ctx->lane_read[l] ? hipStreamWaitEvent(ctx->lane_stream[l], ctx->lane_reduced[l], 0) : hipSuccess;
    if (e == hipSuccess) e = hipEventRecord(ctx->ring0[slot], ctx->lane_stream[l]);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return overlap_failed(ctx, fail(MCAMD_ERR_HIP, "internal stream %d: %s", l, hipGetErrorString(e)));
    }
    *lane = l;
    return MCAMD_OK;
}

int overlap_finish(mcamd_ctx *ctx, int lane, uint32_t records, int record_doubles, double *d_stats, double n_value)
{
    const uint32_t slot = ring_slot(ctx->n_enqueued);
    hipError_t e = hipEventRecord(ctx->ring1[slot], ctx->lane_stream[lane]);
    // the reduction, and with it everything the caller enqueues later, waits for the kernel
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->ring1[slot], 0);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return overlap_failed(ctx, fail(MCAMD_ERR_HIP, "internal stream %d: %s", lane, hipGetErrorString(e)));
    }
    HIP_TRY(launch_final_reduce(ctx->lane_partials[lane], records, record_doubles, d_stats, ctx->stream, n_value));
    HIP_TRY(hipEventRecord(ctx->lane_reduced[lane], ctx->stream));
    ctx->lane_read[lane] = true;
    OverlapSlot &s = ctx->ring_overlap[slot];
    s.chained = ctx->n_enqueued > 0 && slot_overlapped(ctx->ring_overlap, ctx->n_enqueued - 1);
    s.call = ctx->n_enqueued + 1;
    s.lane = static_cast<uint8_t>(lane);
    ctx->n_overlapped++;
    ctx->n_enqueued++;
    return MCAMD_OK;
}

int check_request(const mcamd_option *opt, const mcamd_sim *sim)
{
    if (int rc = check_precision_steps(sim)) return rc;
    if (opt->Tk < 0 || static_cast<uint32_t>(opt->Tk) >= sim->n_steps)
        return fail(MCAMD_ERR_INVALID, "restart Tk=%d must satisfy 0 <= Tk < n_steps=%u", opt->Tk, sim->n_steps);
    if (!(opt->T > 0.0) || !(opt->v >= 0.0) || !std::isfinite(opt->S0) || !std::isfinite(opt->K) ||
        !std::isfinite(opt->r) || !std::isfinite(opt->T) || !std::isfinite(opt->v))
        return fail(MCAMD_ERR_INVALID, "option parameters must be finite with T > 0 and v >= 0");
    if (!(opt->dt >= 0.0) || !std::isfinite(opt->dt))
        return fail(MCAMD_ERR_INVALID, "dt must be 0 (= T / n_steps) or a positive finite step, got %g", opt->dt);
    if (sim->flags & ~(MCAMD_FLAG_LOG_SPACE | MCAMD_FLAG_ANTITHETIC | MCAMD_FLAG_CONTROL_VARIATE | MCAMD_FLAG_SEPARATE_REDUCE |
                       MCAMD_FLAG_PRODUCT_FORM))
        return fail(MCAMD_ERR_INVALID, "unknown bits in flags: %d", sim->flags);
    if ((sim->flags & MCAMD_FLAG_LOG_SPACE) && (sim->flags & MCAMD_FLAG_PRODUCT_FORM))
        return fail(MCAMD_ERR_INVALID, "MCAMD_FLAG_LOG_SPACE and MCAMD_FLAG_PRODUCT_FORM exclude each other");
    if (sim->path_offset + sim->n_paths_local < sim->path_offset)
        return fail(MCAMD_ERR_INVALID, "path_offset + n_paths_local overflows 64 bits");
    if (sim->precision == MCAMD_F64) {
        // fp64 keeps a path's exponent as an int32 count of 2^-16 octaves (fast64.hpp ExpAcc): bound the largest
        // log-return a path can reach (|z| <= 8.6 for the 53-bit Box-Muller uniform).  A job beyond this has prices
        // outside the range of a double anyway (e^709); the fp32 path saturates in hardware.
        const double dt = step_dt(opt, sim);
        const double per_step = std::fabs((opt->r - 0.5 * opt->v * opt->v) * dt) + 8.6 * opt->v * std::sqrt(dt);
        if (!(per_step < 700.0) || !(per_step * static_cast<double>(sim->n_steps) < 20000.0))
            return fail(MCAMD_ERR_INVALID,
                        "fp64 path: |drift| + 8.6 vol = %.3g per step over %u steps exceeds the exponent range "
                        "(per step < 700, per path < 20000)", per_step, sim->n_steps);
    }
    return MCAMD_OK;
}

int check_common(const mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim)
{
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (!opt || !sim) return fail(MCAMD_ERR_INVALID, "opt and sim must be non-NULL");
    return check_request(opt, sim);
}

int check_plain(const mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int layout)
{
    if (int rc = check_common(ctx, opt, sim)) return rc;
    if (sim->flags & (MCAMD_FLAG_ANTITHETIC | MCAMD_FLAG_CONTROL_VARIATE))
        return fail(MCAMD_ERR_INVALID, "variance-reduction flags apply to mcamd_price_paths only");
    if (layout != MCAMD_STEP_MAJOR && layout != MCAMD_PATH_MAJOR)
        return fail(MCAMD_ERR_INVALID, "layout must be MCAMD_STEP_MAJOR or MCAMD_PATH_MAJOR");
    return MCAMD_OK;
}

PathJob make_job(const mcamd_option *opt, const mcamd_sim *sim)
{
    PathJob j;
    const double dt = step_dt(opt, sim);
    j.drift = (opt->r - 0.5 * opt->v * opt->v) * dt;
    j.vol = opt->v * std::sqrt(dt);
    j.K = opt->K;
    j.B = opt->B;
    j.S_start = (opt->Sk == 0.0) ? opt->S0 : opt->Sk;
    j.P1 = opt->P1;
    j.P2 = opt->P2;
    j.Ik = opt->Ik;
    j.n_sim = sim->n_steps - static_cast<uint32_t>(opt->Tk);
    j.n_steps = sim->n_steps;
    j.seed = sim->seed;
    j.path_offset = sim->path_offset;
    j.n_local = sim->n_paths_local;
    j.window = opt->use_window != 0;
    // the in-register kernels (pricing with or without a window, nested-MC inner stage) carry ln(St / S0) unless the
    // caller asks for the product form; the kernels that must produce St at every step ignore this
    j.logspace = (sim->flags & MCAMD_FLAG_PRODUCT_FORM) == 0;
    j.vr = ((sim->flags & MCAMD_FLAG_ANTITHETIC) ? 1 : 0) | ((sim->flags & MCAMD_FLAG_CONTROL_VARIATE) ? 2 : 0);
    // E[S_T] under the simulated dynamics: S_start exp(r * remaining time)
    j.control_mean = j.S_start * std::exp(opt->r * dt * static_cast<double>(j.n_sim));
    j.precision = sim->precision;
    return j;
}

PathJob make_plain_job(const mcamd_option *opt, const mcamd_sim *sim, bool window, bool logspace)
{
    PathJob j = make_job(opt, sim);
    j.window = window;
    j.logspace = logspace;
    j.vr = 0;
    return j;
}

int check_spot_start(const char *name, bool american, const mcamd_option *opt, const mcamd_sim *sim)
{
    const int allowed_flags = american ? MCAMD_FLAG_LOG_SPACE | MCAMD_FLAG_PRODUCT_FORM : MCAMD_FLAG_LOG_SPACE;
    if (american) {
        if (opt->use_window)
            return fail(MCAMD_ERR_INVALID, "%s options take no bullet window: use_window must be 0", name);
    } else if (opt->use_window || opt->P1 != 0 || opt->P2 != 0 || opt->Ik != 0) {
        return fail(MCAMD_ERR_INVALID, "%s options take no bullet window: use_window, P1, P2 and Ik must be 0", name);
    }
    if (opt->Tk != 0 || opt->Sk != 0.0)
        return fail(MCAMD_ERR_INVALID, "%s options start at t = 0: Tk and Sk must be 0 (Tk = %d, Sk = %g)", name,
                    opt->Tk, opt->Sk);
    if (opt->dt != 0.0) return fail(MCAMD_ERR_INVALID, "%s options step dt = T / n_steps: opt->dt must be 0", name);
    if (american) {
        if (!(opt->v > 0.0) || !(opt->S0 > 0.0) || !(opt->K > 0.0))
            return fail(MCAMD_ERR_INVALID, "%s options need v > 0, S0 > 0 and K > 0 (v = %g, S0 = %g, K = %g)", name,
                        opt->v, opt->S0, opt->K);
    } else if (!(opt->v > 0.0)) {
        return fail(MCAMD_ERR_INVALID, "%s options need v > 0 (v = %g)", name, opt->v);
    }
    if ((sim->flags & ~allowed_flags) || sim->flags == (MCAMD_FLAG_LOG_SPACE | MCAMD_FLAG_PRODUCT_FORM))
        return fail(MCAMD_ERR_INVALID, american ? "%s options take flags 0, MCAMD_FLAG_LOG_SPACE or "
                                                  "MCAMD_FLAG_PRODUCT_FORM, got %d"
                                                : "%s options take flags 0 or MCAMD_FLAG_LOG_SPACE only, got %d",
                    name, sim->flags);
    return MCAMD_OK;
}

int check_drift_request(const char *name, mcamd_option seen, const mcamd_sim *sim, const double *mu, int n_mu)
{
    seen.v = 1.0;
    if (int rc = check_spot_start(name, false, &seen, sim)) return rc;
    seen.v = 0.0;
    for (int j = 0; j < n_mu; ++j) {
        seen.r = mu[j];
        if (int rc = check_request(&seen, sim)) return rc;
    }
    return MCAMD_OK;
}

void zero_result(mcamd_result *res)
{
    std::memset(res, 0, sizeof *res);
}

void arm_record(double *rec, int n)
{
    std::memset(rec, 0xFF, n * sizeof(double));
}

bool record_unwritten(const double *rec, int n)
{
    for (int k = 0; k < n; ++k) {
        uint64_t bits;
        std::memcpy(&bits, rec + k, sizeof bits);
        if (bits == ~0ull) return true;
    }
    return false;
}

Estimate estimate(double sum, double sumsq, uint64_t n, double disc)
{
    const double N = static_cast<double>(n);
    const double mean = n ? sum / N : 0.0;
    double var = n > 1 ? (sumsq - N * mean * mean) / (N - 1.0) : 0.0;
    if (var < 0.0) var = 0.0;
    return {disc * mean, n ? disc * std::sqrt(var / N) : 0.0};
}

void finalize_cv_into(const double s[5], uint64_t n, double r, double T, mcamd_result *res)
{
    const double disc = std::exp(-r * T);
    const double N = static_cast<double>(n);
    res->sum = s[0]; res->sumsq = s[1]; res->sum_c = s[2]; res->sum_cc = s[3]; res->sum_yc = s[4];
    res->n = n;
    if (n < 2) {
        res->price = n ? disc * s[0] : 0.0;
        res->std_err = 0.0;
        res->ci_lo = res->ci_hi = res->price;
        return;
    }
    const double ybar = s[0] / N, cbar = s[2] / N;
    const double var_y = std::fmax((s[1] - N * ybar * ybar) / (N - 1.0), 0.0);
    const double var_c = std::fmax((s[3] - N * cbar * cbar) / (N - 1.0), 0.0);
    const double cov = (s[4] - N * ybar * cbar) / (N - 1.0);
    const double beta = var_c > 0.0 ? cov / var_c : 0.0;
    const double rho = (var_c > 0.0 && var_y > 0.0) ? cov / std::sqrt(var_c * var_y) : 0.0;
    const double var_res = std::fmax(var_y - beta * cov, 0.0);
    res->cv_beta = beta;
    res->cv_rho = rho;
    res->price = disc * (ybar - beta * cbar);
    res->std_err = disc * std::sqrt(var_res / N);
    set_ci(res);
}

void finalize_counted_into(const double rec[4], uint64_t n, double r, double T, mcamd_result *res)
{
    finalize_into(rec[0], rec[1], n, r, T, res);
    res->work_steps = 64.0 * rec[2];   // wave-steps x 64 lanes
    res->live_steps = rec[3];
}

void finalize_record(const double *rec, bool control_variate, uint64_t n, double r, double T, mcamd_result *res)
{
    if (control_variate) finalize_cv_into(rec, n, r, T, res);
    else finalize_into(rec[0], rec[1], n, r, T, res);
}

// the mean point price is the scalar diagnostic of the wrappers (inc/wrappers.cuh:185-189,316-321)
void finalize_nmc_into(const double rec[kNmcRecord], uint64_t n, mcamd_result *res)
{
    res->sum = rec[0];
    res->sumsq = rec[1];
    res->work_steps = 64.0 * rec[2];   // wave-steps x 64 lanes
    res->live_steps = rec[3];
    res->n = n;
    res->price = n ? res->sum / static_cast<double>(n) : 0.0;
}

void finalize_greeks_into(const double stats[16], double r, double T, int theta_defined, mcamd_greeks *out)
{
    const double disc = std::exp(-r * T);
    const uint64_t n = static_cast<uint64_t>(std::llround(stats[kGreeksRecord]));
    out->n = n;
    for (int k = 0; k < kGreeks; ++k) {
        const Estimate e = estimate(stats[2 * k], stats[2 * k + 1], n, disc);
        out->sum[k] = stats[2 * k];
        out->sumsq[k] = stats[2 * k + 1];
        out->value[k] = e.value;
        out->std_err[k] = e.std_err;
    }
    if (!theta_defined) out->value[MCAMD_GREEK_THETA] = out->std_err[MCAMD_GREEK_THETA] = std::nan("");
}

}  // namespace mcamd::capi

namespace {

// The prepare_* steps below (and those of capi_*.cpp) hold the argument checks and the job of a call with a
// synchronous and an enqueue form.  Once every check has passed they hand the DeviceCall to drive (the form's driver)
// and return what it returns.

// The pricing kernel's launch: on the context's stream into its scratch buffer, as every DeviceCall launches, or where
// run_enqueue aims it (an overlapped job).  A job that run_enqueue aims elsewhere is a kReduce one, of more
// than kFoldMaxRecords workgroups, and so not one of the lane-compacting kernel's (4 workgroups per CU), the only
// pricing kernel that uses d_queue.
struct PriceLaunch {
    const mcamd::PathJob &job;
    mcamd_ctx *ctx;
    uint32_t grid;
    hipError_t operator()(const mcamd::FinishSpec &fs) const { return (*this)(fs, ctx->d_partials, ctx->stream); }
    hipError_t operator()(const mcamd::FinishSpec &fs, double *d_partials, hipStream_t stream) const
    {
        return mcamd::launch_price(job, ctx->compute_units, d_partials, ctx->d_queue, grid, fs, stream);
    }
};

template <typename Drive>
int prepare_paths(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, Drive drive)
{
    if (int rc = check_common(ctx, opt, sim)) return rc;
    if (sim->n_paths_local == 0) return drive(empty_call());
    const mcamd::PathJob job = make_job(opt, sim);
    const uint32_t grid = mcamd::price_grid(job, ctx->compute_units);
    // few records: the kernel's last workgroup sums them and writes the result itself — one launch and no copy per
    // call (the reference's shape, inc/trajectories.cuh:77-111 + one cudaMemcpy)
    const Finish how = grid > mcamd::kFoldMaxRecords ? Finish::kReduce
                       : (sim->flags & MCAMD_FLAG_SEPARATE_REDUCE) ? Finish::kSmall : Finish::kFolded;
    return drive(DeviceCall{job.n_local, grid, (job.vr & 2) ? 5 : 2, 6, how, PriceLaunch{job, ctx, grid}});
}

template <typename Drive>
int prepare_store(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int layout, void *d_traj,
                  int32_t *d_counts, void *d_payoffs, Drive drive)
{
    if (int rc = check_plain(ctx, opt, sim, layout)) return rc;
    if (sim->n_paths_local == 0) return drive(empty_call());
    if (!d_traj) return fail(MCAMD_ERR_INVALID, "d_traj is NULL");
    mcamd::PathJob job = make_job(opt, sim);
    if (d_counts && !job.window) {
        // counts requested for a European payoff: count against B but let every count pay
        job.window = true;
        job.P1 = INT32_MIN;
        job.P2 = INT32_MAX;
    }
    const uint32_t grid = mcamd::store_grid(job.n_local, job.precision);
    return drive(DeviceCall{job.n_local, grid, 2, 6, Finish::kReduce, [&](const mcamd::FinishSpec &) {
        return mcamd::launch_store(job, layout, d_traj, d_counts, d_payoffs, ctx->d_partials, grid, ctx->stream);
    }});
}

// The nested-MC calls: the inner stage (variant) and the fused one (outer_seed, which must differ from the inner seed;
// d_prices / d_counts are its outputs: the fused entry points pass them non-const).
template <typename Drive>
int prepare_nmc(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int layout, int variant, bool fused,
                uint64_t outer_seed, const void *d_prices, const int32_t *d_counts, void *d_point_prices, Drive drive)
{
    if (int rc = check_plain(ctx, opt, sim, layout)) return rc;
    if (!fused && variant != MCAMD_NMC_WAVE_PER_POINT && variant != MCAMD_NMC_BLOCK_PER_POINT &&
        variant != MCAMD_NMC_BLOCK_PER_POINT_PLAIN)
        return fail(MCAMD_ERR_INVALID, "unknown nested-MC variant %d", variant);
    if (opt->Tk != 0) return fail(MCAMD_ERR_INVALID, "nested MC expects outer trajectories stored from step 0 (Tk = 0)");
    if (fused && outer_seed == sim->seed)
        return fail(MCAMD_ERR_INVALID, "outer_seed must differ from the inner seed (sim->seed): equal seeds would make "
                                       "outer path p and inner path p draw the same Philox stream");
    if (sim->n_paths_inner == 0) return fail(MCAMD_ERR_INVALID, "n_paths_inner must be >= 1");
    // inner path j of point q draws Philox subsequence q * n_paths_inner + j, q = global_path * n_steps + step: the
    // largest one of the shard must fit 64 bits
    const long double top = static_cast<long double>(sim->path_offset + sim->n_paths_local) * sim->n_steps * sim->n_paths_inner;
    if (top >= 18446744073709551615.0L)
        return fail(MCAMD_ERR_INVALID, "(path_offset + n_paths_local) * n_steps * n_paths_inner overflows the 64-bit "
                                       "Philox subsequence");
    if (sim->n_paths_local == 0) return drive(empty_call());
    if (!d_prices || !d_point_prices) return fail(MCAMD_ERR_INVALID, "d_prices and d_point_prices must be non-NULL");
    if (opt->use_window && !d_counts) return fail(MCAMD_ERR_INVALID, "bullet window needs d_counts");
    const uint64_t n_points = sim->n_paths_local * static_cast<uint64_t>(sim->n_steps);
    if (n_points / sim->n_steps != sim->n_paths_local) return fail(MCAMD_ERR_INVALID, "point count overflows");
    mcamd::NmcJob job;
    job.path = make_job(opt, sim);
    job.n_inner = sim->n_paths_inner;
    job.discount = std::exp(-opt->r * opt->T);
    job.n_points = n_points;
    job.compute_units = ctx->compute_units;
    if (fused) {
        const uint32_t grid = mcamd::nmc_fused_grid(job);
        return drive(DeviceCall{n_points, grid, mcamd::kNmcRecord, 6, Finish::kReduce, [&](const mcamd::FinishSpec &) {
            return mcamd::launch_nmc_fused(job, outer_seed, layout, const_cast<void *>(d_prices),
                                           const_cast<int32_t *>(d_counts), d_point_prices, ctx->d_partials, ctx->d_queue,
                                           grid, ctx->stream);
        }});
    }
    const uint32_t grid = mcamd::nmc_grid(job, variant);
    return drive(DeviceCall{n_points, grid, mcamd::kNmcRecord, 6, Finish::kReduce, [&](const mcamd::FinishSpec &) {
        return mcamd::launch_nmc_inner(job, layout, variant, d_prices, d_counts, d_point_prices, ctx->d_partials,
                                       ctx->d_queue, grid, ctx->stream);
    }});
}

// The Greeks calls.  The kernel always finishes its own sum (greeks_grid caps the grid) into the 16-double statistics
// record; the request-only refusals come before the context is looked at.
template <typename Drive>
int prepare_greeks(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int method, Drive drive)
{
    if (!opt || !sim) return fail(MCAMD_ERR_INVALID, "opt and sim must be non-NULL");
    if (sim->flags & ~MCAMD_FLAG_LOG_SPACE)
        return fail(MCAMD_ERR_INVALID, "Greeks take flags 0 or MCAMD_FLAG_LOG_SPACE only, got %d", sim->flags);
    const mcamd::GreeksRule rule = mcamd::greeks_rule(*opt, method);
    if (rule.method == 0)
        return fail(MCAMD_ERR_INVALID, method == MCAMD_GREEKS_PATHWISE
                                           ? "pathwise Greeks are wrong for the bullet window's discontinuous payoff: use "
                                             "MCAMD_GREEKS_LIKELIHOOD_RATIO (or AUTO) with use_window = 1"
                                           : "unknown Greeks method %d", method);
    const double S_s = (opt->Sk == 0.0) ? opt->S0 : opt->Sk;
    if (!(opt->v > 0.0) || !(S_s > 0.0))
        return fail(MCAMD_ERR_INVALID, "Greeks need v > 0 and a positive start price (v = %g, S = %g)", opt->v, S_s);
    if (int rc = check_common(ctx, opt, sim)) return rc;
    if (sim->n_paths_local == 0) return drive(empty_call(mcamd::kGreeksStats));
    mcamd::GreeksJob job;
    job.path = make_plain_job(opt, sim, opt->use_window != 0, true);
    job.lr = rule.method == MCAMD_GREEKS_LIKELIHOOD_RATIO;
    const double dt = step_dt(opt, sim);
    const double v = opt->v, r = opt->r, T = opt->T, T_h = dt * static_cast<double>(job.path.n_sim);
    mcamd::GreeksConsts &g = job.g;
    g.K = opt->K;
    g.S_s = S_s;
    g.T = T;
    g.r = r;
    g.v = v;
    g.T_h = T_h;
    g.mu_h = (r - 0.5 * v * v) * T_h;
    g.nu_h = (r + 0.5 * v * v) * T_h;
    g.gamma_pw = 1.0 / (S_s * S_s * v * v * T_h);
    g.theta_mu = r - 0.5 * v * v;
    g.theta_mu_T = g.theta_mu * T;
    g.inv_2T = 0.5 / T;
    g.inv_scale = 0.0;   // set by the launcher: the unit of the path precision's exponent
    g.sqrt_dt = std::sqrt(dt);
    g.delta_lr = 1.0 / (S_s * v * g.sqrt_dt);
    g.gamma_lr1 = 1.0 / (S_s * S_s * v * v * dt);
    g.gamma_lr2 = 1.0 / (S_s * S_s * v * g.sqrt_dt);
    g.theta_on = rule.theta_defined;
    const uint32_t grid = mcamd::greeks_grid(job);
    return drive(DeviceCall{job.path.n_local, grid, mcamd::kGreeksRecord, mcamd::kGreeksStats, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_greeks(job, ctx->d_partials, grid, fs.out, fs.ticket, ctx->stream);
                            }});
}

}  // namespace

extern "C" {

int mcamd_abi_version(void)
{
    return MCAMD_ABI_VERSION;
}

const char *mcamd_last_error(void)
{
    return g_last_error.c_str();
}

#ifndef MCAMD_BUILD_ID
#define MCAMD_BUILD_ID "unknown"
#endif
const char *mcamd_build_id(void)
{
    return MCAMD_BUILD_ID;
}

int mcamd_device_count(int *count)
{
    if (!count) return fail(MCAMD_ERR_INVALID, "count is NULL");
    *count = 0;
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *count = 0;
        return fail(MCAMD_ERR_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    return MCAMD_OK;
}

int mcamd_ctx_create(int device, void *hip_stream, mcamd_ctx **out)
{
    if (!out) return fail(MCAMD_ERR_INVALID, "ctx out-pointer is NULL");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
        (void)hipGetLastError();
        return fail(MCAMD_ERR_NODEVICE, "no HIP device visible: this engine has no CPU fallback");
    }
    if (device < 0 || device >= count) return fail(MCAMD_ERR_INVALID, "device %d out of range [0, %d)", device, count);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MCAMD_ERR_NODEVICE, "device %d is %s; the kernels are built for gfx950 only", device,
                    prop.gcnArchName);
    mcamd_ctx *ctx = new (std::nothrow) mcamd_ctx;
    if (!ctx) return fail(MCAMD_ERR_NOMEM, "out of host memory");
    ctx->device = device;
    static std::atomic<uint64_t> next_id{0};
    ctx->id = ++next_id;
    if (hip_stream) {
        ctx->stream = static_cast<hipStream_t>(hip_stream);
    } else {
        hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete ctx;
            return fail(MCAMD_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
        }
        ctx->own_stream = true;
    }
    hipError_t e = hipEventCreate(&ctx->ev0);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev1);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev2);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev3);
    for (uint32_t i = 0; i < mcamd_ctx::kRing && e == hipSuccess; ++i) {
        e = hipEventCreate(&ctx->ring0[i]);
        if (e == hipSuccess) e = hipEventCreate(&ctx->ring1[i]);
    }
    if (e == hipSuccess) e = hipMalloc(&ctx->d_out, 8 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&ctx->d_queue, 64);
    // the ticket must be zero at a kernel's first launch: zeroed on the context's stream, so that the zeroing is
    // ordered before that launch also on a caller's non-blocking stream
    if (e == hipSuccess) e = hipMemsetAsync(ctx->d_queue, 0, 64, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) ctx->d_ticket = reinterpret_cast<unsigned int *>(ctx->d_queue + 2);
    ctx->compute_units = static_cast<uint32_t>(prop.multiProcessorCount);
    // read once, here: MCAMD_ENQUEUE_OVERLAP=0 keeps every enqueue of this context in order on its stream.  A device on
    // which the lane-compacting kernel's grid (4 workgroups per CU) could need the separate reduction does the same.
    const char *overlap_env = std::getenv("MCAMD_ENQUEUE_OVERLAP");
    ctx->overlap = !(overlap_env && std::strcmp(overlap_env, "0") == 0) && ctx->compute_units * 4 <= mcamd::kFoldMaxRecords;
    if (e == hipSuccess) e = hipHostMalloc(&ctx->h_rec, mcamd_ctx::kRecord * sizeof(double), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void **>(&ctx->h_rec_dev), ctx->h_rec, 0);
    if (e != hipSuccess) {
        mcamd_ctx_destroy(ctx);
        return fail(MCAMD_ERR_HIP, "context setup: %s", hipGetErrorString(e));
    }
    *out = ctx;
    return MCAMD_OK;
}

int mcamd_ctx_destroy(mcamd_ctx *ctx)
{
    if (!ctx) return MCAMD_OK;
    (void)hipSetDevice(ctx->device);
    for (int l = 0; l < 2; ++l)
        if (ctx->lane_stream[l]) (void)hipStreamSynchronize(ctx->lane_stream[l]);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (int l = 0; l < 2; ++l) {
        if (ctx->lane_partials[l]) (void)hipFree(ctx->lane_partials[l]);
        if (ctx->lane_reduced[l]) (void)hipEventDestroy(ctx->lane_reduced[l]);
        if (ctx->lane_stream[l]) (void)hipStreamDestroy(ctx->lane_stream[l]);
    }
    if (ctx->d_partials) (void)hipFree(ctx->d_partials);
    if (ctx->d_out) (void)hipFree(ctx->d_out);
    if (ctx->d_queue) (void)hipFree(ctx->d_queue);
    if (ctx->h_rec) (void)hipHostFree(ctx->h_rec);
    if (ctx->h_smile) (void)hipHostFree(ctx->h_smile);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->ev2) (void)hipEventDestroy(ctx->ev2);
    if (ctx->ev3) (void)hipEventDestroy(ctx->ev3);
    for (uint32_t i = 0; i < mcamd_ctx::kRing; ++i) {
        if (ctx->ring0[i]) (void)hipEventDestroy(ctx->ring0[i]);
        if (ctx->ring1[i]) (void)hipEventDestroy(ctx->ring1[i]);
    }
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return MCAMD_OK;
}

int mcamd_get_device_info(mcamd_ctx *ctx, mcamd_device_info *info)
{
    if (!ctx || !info) return fail(MCAMD_ERR_INVALID, "ctx and info must be non-NULL");
    std::memset(info, 0, sizeof *info);
    HIP_TRY(hipSetDevice(ctx->device));
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, ctx->device));
    std::snprintf(info->name, sizeof info->name, "%s", p.name);
    std::snprintf(info->arch, sizeof info->arch, "%s", p.gcnArchName);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    info->total_mem = total_b;
    info->free_mem = free_b;
    info->compute_units = p.multiProcessorCount;
    info->wavefront_size = p.warpSize;
    info->max_threads_per_block = p.maxThreadsPerBlock;
    info->clock_khz = p.clockRate;
    info->mem_clock_khz = p.memoryClockRate;
    info->mem_bus_bits = p.memoryBusWidth;
    info->lds_per_block = static_cast<int32_t>(p.sharedMemPerBlock);
    info->regs_per_block = p.regsPerBlock;
    info->l2_bytes = p.l2CacheSize;
    info->device_index = ctx->device;
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    info->device_count = count;
    return MCAMD_OK;
}

int mcamd_device_malloc(mcamd_ctx *ctx, uint64_t bytes, void **d_ptr)
{
    if (!ctx || !d_ptr) return fail(MCAMD_ERR_INVALID, "ctx and d_ptr must be non-NULL");
    *d_ptr = nullptr;
    if (bytes == 0) return MCAMD_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMalloc(d_ptr, bytes));
    return MCAMD_OK;
}

int mcamd_device_free(mcamd_ctx *ctx, void *d_ptr)
{
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (!d_ptr) return MCAMD_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipFree(d_ptr));
    return MCAMD_OK;
}

int mcamd_memcpy_to_host(mcamd_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes)
{
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (bytes == 0) return MCAMD_OK;
    if (!h_dst || !d_src) return fail(MCAMD_ERR_INVALID, "copy pointers must be non-NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MCAMD_OK;
}

int mcamd_memcpy_to_device(mcamd_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes)
{
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (bytes == 0) return MCAMD_OK;
    if (!d_dst || !h_src) return fail(MCAMD_ERR_INVALID, "copy pointers must be non-NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MCAMD_OK;
}

int mcamd_price_paths(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, mcamd_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim and res must be non-NULL");
    zero_result(res);
    return prepare_paths(ctx, opt, sim, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) {
            finalize_record(rec, call.rec == 5, sim->n_paths_local, opt->r, opt->T, res);
        });
    });
}

int mcamd_price_paths_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, double *d_stats)
{
    return prepare_paths(ctx, opt, sim, [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

int mcamd_simulate_trajectories_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int layout,
                                        void *d_traj, int32_t *d_counts, void *d_payoffs, double *d_stats)
{
    return prepare_store(ctx, opt, sim, layout, d_traj, d_counts, d_payoffs,
                         [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

int mcamd_nmc_inner_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int layout, int variant,
                            const void *d_prices, const int32_t *d_counts, void *d_point_prices, double *d_stats)
{
    return prepare_nmc(ctx, opt, sim, layout, variant, false, 0, d_prices, d_counts, d_point_prices,
                       [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

int mcamd_nmc_fused_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, uint64_t outer_seed, int layout,
                            void *d_prices, int32_t *d_counts, void *d_point_prices, double *d_stats)
{
    return prepare_nmc(ctx, opt, sim, layout, 0, true, outer_seed, d_prices, d_counts, d_point_prices,
                       [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

int mcamd_finalize_nmc_stats(const double stats[6], mcamd_result *res)
{
    if (!stats || !res) return fail(MCAMD_ERR_INVALID, "stats and res must be non-NULL");
    zero_result(res);
    finalize_nmc_into(stats, static_cast<uint64_t>(std::llround(stats[5])), res);
    return MCAMD_OK;
}

int mcamd_enqueued_kernel_ms(mcamd_ctx *ctx, uint32_t n_last, float *ms)
{
    if (!ctx || !ms) return fail(MCAMD_ERR_INVALID, "ctx and ms must be non-NULL");
    if (n_last > mcamd_ctx::kRing || n_last > ctx->n_enqueued)
        return fail(MCAMD_ERR_INVALID, "only the last min(%u, enqueued) calls are kept", mcamd_ctx::kRing);
    HIP_TRY(hipSetDevice(ctx->device));
    for (int l = 0; l < 2; ++l)
        if (ctx->lane_stream[l]) HIP_TRY(hipStreamSynchronize(ctx->lane_stream[l]));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint64_t first = ctx->n_enqueued - n_last;
    for (uint32_t i = 0; i < n_last; ++i) {
        const uint32_t slot = ring_slot(first + i);
        HIP_TRY(hipEventElapsedTime(&ms[i], ctx->ring0[slot], ctx->ring1[slot]));
    }
    // Runs of overlapped jobs [b, e): each job is charged the part of its interval that enqueue_intervals.hpp gives it,
    // on the clock that starts at the run's first start event.  A run may reach back past the calls asked for.
    const OverlapSlot *ring = ctx->ring_overlap;
    for (uint64_t call = first; call < ctx->n_enqueued;) {
        uint64_t b = call, e = call + 1;
        while (continues_run(ring, b, ctx->n_enqueued)) --b;
        while (continues_run(ring, e, ctx->n_enqueued)) ++e;
        call = e;
        if (e - b < 2) continue;
        double start[mcamd_ctx::kRing], end[mcamd_ctx::kRing], charged[mcamd_ctx::kRing];
        const uint32_t n = static_cast<uint32_t>(e - b);
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t slot = ring_slot(b + k);
            float since_base = 0.0f, own = 0.0f;
            if (k) HIP_TRY(hipEventElapsedTime(&since_base, ctx->ring0[ring_slot(b)], ctx->ring0[slot]));
            HIP_TRY(hipEventElapsedTime(&own, ctx->ring0[slot], ctx->ring1[slot]));
            start[k] = since_base;
            end[k] = static_cast<double>(since_base) + own;
        }
        exclusive_run_ms(start, end, n, charged);
        for (uint32_t k = 0; k < n; ++k)
            if (b + k >= first) ms[b + k - first] = static_cast<float>(charged[k]);
    }
    return MCAMD_OK;
}

int mcamd_finalize_stats(const double stats[6], double r, double T, int control_variate, mcamd_result *res)
{
    if (!stats || !res) return fail(MCAMD_ERR_INVALID, "stats and res must be non-NULL");
    zero_result(res);
    finalize_record(stats, control_variate != 0, static_cast<uint64_t>(std::llround(stats[5])), r, T, res);
    return MCAMD_OK;
}

int mcamd_simulate_trajectories(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int layout,
                                void *d_traj, int32_t *d_counts, void *d_payoffs, mcamd_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim and res must be non-NULL");
    zero_result(res);
    return prepare_store(ctx, opt, sim, layout, d_traj, d_counts, d_payoffs, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) {
            finalize_into(rec[0], rec[1], sim->n_paths_local, opt->r, opt->T, res);
        });
    });
}

int mcamd_diag_store_pattern(mcamd_ctx *ctx, uint64_t n_paths_local, uint32_t n_steps, int precision, void *d_traj,
                             void *d_payoffs, float *kernel_ms)
{
    if (!ctx || !kernel_ms) return fail(MCAMD_ERR_INVALID, "ctx and kernel_ms must be non-NULL");
    if (precision != MCAMD_F32 && precision != MCAMD_F64) return fail(MCAMD_ERR_INVALID, "bad precision %d", precision);
    *kernel_ms = 0.0f;
    const uint64_t v = precision == MCAMD_F32 ? 4 : 2;
    if (n_paths_local == 0 || n_steps == 0) return MCAMD_OK;
    if (!d_traj) return fail(MCAMD_ERR_INVALID, "d_traj is NULL");
    if (n_paths_local % v != 0 || reinterpret_cast<uintptr_t>(d_traj) % 16 != 0 || reinterpret_cast<uintptr_t>(d_payoffs) % 16 != 0 ||
        n_paths_local + v > 0xffffffffull / 8)
        return fail(MCAMD_ERR_INVALID, "the store pattern is the vector store path's: n_paths_local a multiple of %llu (< 2^29), "
                                       "16-byte aligned buffers", static_cast<unsigned long long>(v));
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t grid = mcamd::store_grid(n_paths_local, precision);
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    HIP_TRY(mcamd::launch_store_pattern(n_paths_local, n_steps, precision, d_traj, d_payoffs, grid, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipEventElapsedTime(kernel_ms, ctx->ev0, ctx->ev1));
    return MCAMD_OK;
}

int mcamd_price_from_normals(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const void *d_normals,
                             void *d_payoffs, mcamd_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim and res must be non-NULL");
    if (int rc = check_plain(ctx, opt, sim)) return rc;
    zero_result(res);
    if (sim->n_paths_local == 0) return MCAMD_OK;
    if (!d_normals) return fail(MCAMD_ERR_INVALID, "d_normals is NULL");
    const mcamd::PathJob job = make_job(opt, sim);
    const uint32_t grid = mcamd::array_grid(job.n_local);
    const DeviceCall call{job.n_local, grid, 2, 6, Finish::kReduce, [&](const mcamd::FinishSpec &) {
        return mcamd::launch_from_normals(job, d_normals, d_payoffs, ctx->d_partials, grid, ctx->stream);
    }};
    return run_sync(ctx, call, res, [&](const double *rec) {
        finalize_into(rec[0], rec[1], sim->n_paths_local, opt->r, opt->T, res);
    });
}

int mcamd_generate_normals(mcamd_ctx *ctx, uint64_t seed, uint64_t n, int precision, void *d_out, float *kernel_ms)
{
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (precision != MCAMD_F32 && precision != MCAMD_F64) return fail(MCAMD_ERR_INVALID, "bad precision %d", precision);
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n == 0) return MCAMD_OK;
    if (!d_out) return fail(MCAMD_ERR_INVALID, "d_out is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    HIP_TRY(mcamd::launch_generate_normals(seed, n, precision, d_out, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, ctx->ev0, ctx->ev1));
    return MCAMD_OK;
}

int mcamd_reduce_sum(mcamd_ctx *ctx, const void *d_in, uint64_t n, int precision, int variant, double *sum,
                     float *kernel_ms)
{
    if (!ctx || !sum) return fail(MCAMD_ERR_INVALID, "ctx and sum must be non-NULL");
    if (precision != MCAMD_F32 && precision != MCAMD_F64) return fail(MCAMD_ERR_INVALID, "bad precision %d", precision);
    if (variant < MCAMD_REDUCE_SEQUENTIAL || variant > MCAMD_REDUCE_GRID_STRIDE)
        return fail(MCAMD_ERR_INVALID, "reduce variant must be 3..6 (ReductionType), got %d", variant);
    *sum = 0.0;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n == 0) return MCAMD_OK;
    if (!d_in) return fail(MCAMD_ERR_INVALID, "d_in is NULL");
    const uint32_t grid = mcamd::reduce_grid(n, variant);
    const DeviceCall call{n, grid, 2, 6, Finish::kReduce, [&](const mcamd::FinishSpec &) {
        return mcamd::launch_reduce(d_in, n, precision, variant, ctx->d_partials, grid, ctx->stream);
    }};
    mcamd_result tmp;
    zero_result(&tmp);
    if (int rc = run_sync(ctx, call, &tmp, [&](const double *rec) { *sum = rec[0]; })) return rc;
    if (kernel_ms) *kernel_ms = tmp.kernel_ms;
    return MCAMD_OK;
}

int mcamd_nmc_inner(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int layout, int variant,
                    const void *d_prices, const int32_t *d_counts, void *d_point_prices, mcamd_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim and res must be non-NULL");
    zero_result(res);
    return prepare_nmc(ctx, opt, sim, layout, variant, false, 0, d_prices, d_counts, d_point_prices, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) { finalize_nmc_into(rec, call.n, res); });
    });
}

int mcamd_nmc_fused(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, uint64_t outer_seed, int layout,
                    void *d_prices, int32_t *d_counts, void *d_point_prices, mcamd_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim and res must be non-NULL");
    zero_result(res);
    return prepare_nmc(ctx, opt, sim, layout, 0, true, outer_seed, d_prices, d_counts, d_point_prices, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) { finalize_nmc_into(rec, call.n, res); });
    });
}

int mcamd_reduce_partials(mcamd_ctx *ctx, const void *d_in, uint64_t n, int precision, int variant, uint32_t n_blocks,
                          double *h_partials, float *kernel_ms)
{
    if (!ctx || !h_partials) return fail(MCAMD_ERR_INVALID, "ctx and h_partials must be non-NULL");
    if (precision != MCAMD_F32 && precision != MCAMD_F64) return fail(MCAMD_ERR_INVALID, "bad precision %d", precision);
    if (variant < MCAMD_REDUCE_SEQUENTIAL || variant > MCAMD_REDUCE_GRID_STRIDE)
        return fail(MCAMD_ERR_INVALID, "reduce variant must be 3..6 (ReductionType), got %d", variant);
    if (n_blocks == 0 || n_blocks > mcamd::kMaxGrid) return fail(MCAMD_ERR_INVALID, "n_blocks must be in [1, 2^20]");
    if (kernel_ms) *kernel_ms = 0.0f;
    for (uint32_t b = 0; b < n_blocks; ++b) h_partials[b] = 0.0;
    if (n == 0) return MCAMD_OK;
    if (!d_in) return fail(MCAMD_ERR_INVALID, "d_in is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = ensure_partials(ctx, n_blocks)) return rc;
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    HIP_TRY(mcamd::launch_reduce(d_in, n, precision, variant, ctx->d_partials, n_blocks, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    // the kernels leave records of two doubles {partial, 0}: strided copy of the first of each
    HIP_TRY(hipMemcpy2DAsync(h_partials, sizeof(double), ctx->d_partials, 2 * sizeof(double), sizeof(double), n_blocks,
                             hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, ctx->ev0, ctx->ev1));
    return MCAMD_OK;
}

int mcamd_cpu_mc_f32(const mcamd_option *opt, uint64_t n_paths, uint32_t n_steps, uint64_t seed, int from_random_device,
                     float *price, float *payoff_sum)
{
    if (!opt || !price) return fail(MCAMD_ERR_INVALID, "opt and price must be non-NULL");
    if (n_steps == 0) return fail(MCAMD_ERR_INVALID, "n_steps must be >= 1");
    *price = 0.0f;
    if (payoff_sum) *payoff_sum = 0.0f;
    if (n_paths == 0) return MCAMD_OK;
    // fp32 throughout, the operation order of inc/tool.cuh:104-173
    const float K = static_cast<float>(opt->K), r = static_cast<float>(opt->r), sigma = static_cast<float>(opt->v);
    const float S0 = static_cast<float>(opt->S0), T = static_cast<float>(opt->T), B = static_cast<float>(opt->B);
    const float dt = opt->dt > 0.0 ? static_cast<float>(opt->dt) : T / static_cast<float>(n_steps);
    const float sqrdt = sqrtf(dt);
    const float P1 = static_cast<float>(opt->P1), P2 = static_cast<float>(opt->P2);   // the reference compares as floats
    std::mt19937 generator(from_random_device ? std::random_device{}() : static_cast<std::mt19937::result_type>(seed));
    std::normal_distribution<float> distribution(0.0f, 1.0f);
    float sum = 0.0f;
    for (uint64_t i = 0; i < n_paths; ++i) {
        float St = S0;
        int count = 0;
        for (uint32_t j = 0; j < n_steps; ++j) {
            const float G = distribution(generator);
            St *= expf((r - (sigma * sigma) / 2) * dt + sigma * sqrdt * G);
            if (opt->use_window && St < B) count++;
        }
        if (!opt->use_window || (count >= P1 && count <= P2)) sum += std::fmax(St - K, 0.0f);
    }
    if (payoff_sum) *payoff_sum = sum;
    *price = expf(-r * T) * sum / static_cast<float>(n_paths);
    return MCAMD_OK;
}

int mcamd_price_greeks(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int method, mcamd_greeks *out)
{
    if (!out) return fail(MCAMD_ERR_INVALID, "out is NULL");
    std::memset(out, 0, sizeof *out);
    return prepare_greeks(ctx, opt, sim, method, [&](const auto &call) {
        const mcamd::GreeksRule rule = mcamd::greeks_rule(*opt, method);
        out->method = rule.method;
        return run_sync(ctx, call, out, [&](const double *stats) {
            finalize_greeks_into(stats, opt->r, opt->T, rule.theta_defined, out);
        });
    });
}

int mcamd_price_greeks_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int method,
                               double *d_stats)
{
    return prepare_greeks(ctx, opt, sim, method, [&](const auto &call) {
        if (call.n && d_stats) {   // NaN (all-ones bytes) until the kernel has written the record
            HIP_TRY(hipSetDevice(ctx->device));
            HIP_TRY(hipMemsetAsync(d_stats, 0xFF, mcamd::kGreeksStats * sizeof(double), ctx->stream));
        }
        return run_enqueue(ctx, call, d_stats);
    });
}

int mcamd_finalize_greeks_stats(const double stats[16], double r, double T, int theta_defined, mcamd_greeks *out)
{
    if (!stats || !out) return fail(MCAMD_ERR_INVALID, "stats and out must be non-NULL");
    std::memset(out, 0, sizeof *out);
    finalize_greeks_into(stats, r, T, theta_defined, out);
    return MCAMD_OK;
}

int mcamd_finalize_localvol_greeks_stats(const double stats[32], double r, double T, uint32_t n_vega_buckets,
                                         int gamma_defined, mcamd_localvol_greeks *out)
{
    if (!stats || !out) return fail(MCAMD_ERR_INVALID, "stats and out must be non-NULL");
    if (n_vega_buckets > MCAMD_LOCALVOL_GREEKS_MAX_BUCKETS)
        return fail(MCAMD_ERR_INVALID, "n_vega_buckets must lie in 0 .. %d, got %u", MCAMD_LOCALVOL_GREEKS_MAX_BUCKETS,
                    n_vega_buckets);
    std::memset(out, 0, sizeof *out);
    finalize_localvol_greeks_into(stats, r, T, n_vega_buckets, gamma_defined, out);
    return MCAMD_OK;
}

int mcamd_finalize(double sum, double sumsq, uint64_t n, double r, double T, mcamd_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "res is NULL");
    zero_result(res);
    finalize_into(sum, sumsq, n, r, T, res);
    return MCAMD_OK;
}

int mcamd_finalize_cv(const double sums[5], uint64_t n, double r, double T, mcamd_result *res)
{
    if (!res || !sums) return fail(MCAMD_ERR_INVALID, "sums and res must be non-NULL");
    zero_result(res);
    finalize_cv_into(sums, n, r, T, res);
    return MCAMD_OK;
}

}  // extern "C"
