// capi.cpp — the C ABI declared in include/mcamd.h: argument checking, context/scratch
// ownership, HIP-event timing, final host-side statistics.  All device work is enqueued through
// the launchers of launch.hpp on the context's stream; there is no CPU fallback of any kind — a
// call either runs the gfx950 kernels or returns an error.
#include "launch.hpp"
#include "greeks.hpp"
#include "american.hpp"
#include "american_dual.hpp"
#include "barrier.hpp"
#include "lookback.hpp"
#include "basket.hpp"
#include "asian.hpp"
#include "autocall.hpp"
#include "autocall_localvol.hpp"
#include "cliquet.hpp"
#include "localvol.hpp"
#include "localvol_greeks.hpp"
#include "localvol_smile.hpp"

#include "mcamd.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static_assert(sizeof(mcamd_option) == 88 && sizeof(mcamd_sim) == 48 && sizeof(mcamd_result) == 128 &&
                  sizeof(mcamd_device_info) == 384,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_greeks) == 224, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_american) == 32 && sizeof(mcamd_american_result) == 152,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_american_dual) == 16 && sizeof(mcamd_american_dual_result) == 104,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_barrier) == 16, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_lookback) == 16, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_basket) == 728, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_asian) == 24, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_autocall) == 632 && sizeof(mcamd_autocall_result) == 112,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_autocall_localvol) == 632, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_localvol_grid) == 24 && sizeof(mcamd_localvol) == 24,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_smile) == 24, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(MCAMD_SMILE_MAX_STRIKES == mcamd::kSmileMaxStrikes && MCAMD_SMILE_MAX_EXPIRIES == mcamd::kSmileMaxExpiries,
              "the smile kernel takes one strike per lane and MCAMD_SMILE_MAX_EXPIRIES expiry steps");
static_assert(sizeof(mcamd_localvol_greeks_job) == 24 && sizeof(mcamd_localvol_greeks) == 472,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(MCAMD_LOCALVOL_GREEKS_MAX_BUCKETS == mcamd::kLvGreeksMaxBuckets && MCAMD_LOCALVOL_GREEK_RHO_Q + 1 == mcamd::kLvGreeks,
              "the kernel's record holds six estimators and MCAMD_LOCALVOL_GREEKS_MAX_BUCKETS buckets");
static_assert(sizeof(mcamd_cliquet) == 56 && sizeof(mcamd_cliquet_result) == 96,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(MCAMD_CLIQUET_SUM == mcamd::kCliquetSum && MCAMD_CLIQUET_COMPOUND == mcamd::kCliquetCompound &&
                  MCAMD_CLIQUET_VARIANCE == mcamd::kCliquetVariance,
              "the kernels' kinds are MCAMD_CLIQUET_*");
static_assert(MCAMD_LOCALVOL_MAX_NODES == mcamd::kLocalVolMaxNodes, "the kernel's LDS budget holds MCAMD_LOCALVOL_MAX_NODES");
static_assert(MCAMD_AUTOCALL_MAX_DATES == mcamd::kAutocallMaxDates, "the kernel's date tables hold MCAMD_AUTOCALL_MAX_DATES");

namespace {

thread_local std::string g_last_error;

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

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            (void)hipGetLastError();                                                                   \
            return fail(e_ == hipErrorOutOfMemory ? MCAMD_ERR_NOMEM : MCAMD_ERR_HIP, "%s: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                             \
        }                                                                                              \
    } while (0)

}  // namespace

// used by group.cpp: records the calling thread's last error message
int mcamd_set_error_(int code, const char *msg)
{
    g_last_error = msg ? msg : "";
    return code;
}

struct mcamd_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    double *d_partials = nullptr;  // one record (2 or 5 doubles) per block
    uint64_t partial_capacity = 0; // in doubles
    double *d_out = nullptr;       // 8 doubles
    unsigned long long *d_queue = nullptr;  // task counter of the wave-per-point nested-MC kernel
    unsigned int *d_ticket = nullptr;       // arrival counter of kernels that finish their own sum (in d_queue's allocation)
    uint32_t compute_units = 0;
    static constexpr int kRecord = 32;      // doubles of h_rec: the widest final record (the local-volatility Greeks' statistics layout)
    double *h_rec = nullptr;                // pinned: the final record of a synchronous call
    double *h_rec_dev = nullptr;            // h_rec as the device addresses it (a self-finishing kernel writes there)
    // asynchronous calls: a ring of event pairs around the simulation kernel of the last kRing enqueues
    static constexpr uint32_t kRing = 64;
    hipEvent_t ring0[kRing] = {}, ring1[kRing] = {};
    uint64_t n_enqueued = 0;
    uint64_t id = 0;   // unique per context of the process: what a local-volatility surface remembers of its owner
    // pinned: the node sums of a synchronous smile call (allocated by the first one, at the largest smile's size)
    static constexpr uint32_t kSmileStats = 2 * MCAMD_SMILE_MAX_EXPIRIES * MCAMD_SMILE_MAX_STRIKES;
    double *h_smile = nullptr;
    double *h_smile_dev = nullptr;   // h_smile as the device addresses it
};

// An immutable local-volatility surface: the grid, the largest entry, and the two pair tables in device memory.
struct mcamd_localvol_surface {
    const mcamd_ctx *ctx = nullptr;
    uint64_t ctx_id = 0;
    int device = 0;
    mcamd_localvol_grid grid = {};
    double sigma_max = 0.0;
    void *d_tables = nullptr;   // one allocation: n fp64 pairs, then n fp32 pairs
    void *d_tab64 = nullptr, *d_tab32 = nullptr;
};

namespace {

constexpr double kZ95 = 1.959963984540054;   // two-sided 95 % quantile of the standard normal

int ensure_partials(mcamd_ctx *ctx, uint32_t records, int record_doubles = 2)
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

// what every path call refuses on the request alone (opt and sim non-NULL)
int check_request(const mcamd_option *opt, const mcamd_sim *sim)
{
    if (sim->precision != MCAMD_F32 && sim->precision != MCAMD_F64)
        return fail(MCAMD_ERR_INVALID, "precision must be MCAMD_F32 (32) or MCAMD_F64 (64), got %d", sim->precision);
    if (sim->n_steps == 0) return fail(MCAMD_ERR_INVALID, "n_steps must be >= 1");
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
        const double dt = opt->dt > 0.0 ? opt->dt : opt->T / static_cast<double>(sim->n_steps);
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

// check_common plus the refusals of the calls that run plain paths (no variance reduction) and, but for
// mcamd_price_from_normals, take a trajectory layout
int check_plain(const mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int layout = MCAMD_STEP_MAJOR)
{
    if (int rc = check_common(ctx, opt, sim)) return rc;
    if (sim->flags & (MCAMD_FLAG_ANTITHETIC | MCAMD_FLAG_CONTROL_VARIATE))
        return fail(MCAMD_ERR_INVALID, "variance-reduction flags apply to mcamd_price_paths only");
    if (layout != MCAMD_STEP_MAJOR && layout != MCAMD_PATH_MAJOR)
        return fail(MCAMD_ERR_INVALID, "layout must be MCAMD_STEP_MAJOR or MCAMD_PATH_MAJOR");
    return MCAMD_OK;
}
mcamd::PathJob make_job(const mcamd_option *opt, const mcamd_sim *sim)
{
    mcamd::PathJob j;
    const double dt = opt->dt > 0.0 ? opt->dt : opt->T / static_cast<double>(sim->n_steps);
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

// The job of a call that runs plain paths whatever the flags say: no variance reduction, the given window and form.
mcamd::PathJob make_plain_job(const mcamd_option *opt, const mcamd_sim *sim, bool window, bool logspace)
{
    mcamd::PathJob j = make_job(opt, sim);
    j.window = window;
    j.logspace = logspace;
    j.vr = 0;
    return j;
}

// What a plain product that starts at the spot ("American", "barrier", "lookback" options) refuses of the option and
// the flags.  american: the rules of the two American calls, which read only use_window of the window fields, price
// off S0 and K as well, and take the product form; the others allow MCAMD_FLAG_LOG_SPACE alone.
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

void zero_result(mcamd_result *res)
{
    std::memset(res, 0, sizeof *res);
}

// How the block records of a call's simulation kernel reach the host.
enum class Finish {
    kFolded,    // the kernel sums them itself and writes the final record where FinishSpec::out points
    kSmall,     // separate launch of the same sum (launch_small_final)
    kReduce     // separate 1024-thread reduction (launch_final_reduce)
};

// One device call as both drivers (run_sync, run_enqueue) see it.  launch(fs) enqueues the simulation kernel on
// ctx->stream; fs.out and fs.ticket are set when how == kFolded.
template <typename Launch>
struct DeviceCall {
    uint64_t n;      // paths (nested MC: points) of the shard, the statistics layout's n; 0: empty shard, nothing runs
    uint32_t grid;   // block records the kernel writes
    int rec;         // doubles per block record
    int stats;       // doubles of the statistics layout an enqueue leaves in d_stats: 6, 16 for Greeks, 32 for the
                     // local-volatility Greeks
    Finish how;
    Launch launch;
};
template <typename Launch>
DeviceCall(uint64_t, uint32_t, int, int, Finish, Launch) -> DeviceCall<Launch>;

struct NoLaunch {
    hipError_t operator()(const mcamd::FinishSpec &) const { return hipSuccess; }
};
DeviceCall<NoLaunch> empty_call(int stats = 6)
{
    return {0, 0, 2, stats, Finish::kReduce, {}};
}

// A self-finishing kernel's final record is filled with all-ones bits before the launch.  No finished sum has that
// pattern (a NaN the arithmetic makes is the canonical one), so finding it after the sync means the kernel's last
// workgroup never wrote the record, e.g. because the arrival ticket was not zero at launch.  Bits, not isnan: an fp32
// job that saturates can sum to a genuine NaN, and that is a result.
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

// disc x the mean of n samples and its standard error, from their sum and sum of squares
struct Estimate {
    double value, std_err;
};
Estimate estimate(double sum, double sumsq, uint64_t n, double disc)
{
    const double N = static_cast<double>(n);
    const double mean = n ? sum / N : 0.0;
    double var = n > 1 ? (sumsq - N * mean * mean) / (N - 1.0) : 0.0;
    if (var < 0.0) var = 0.0;
    return {disc * mean, n ? disc * std::sqrt(var / N) : 0.0};
}

template <typename Result>   // mcamd_result, mcamd_american_result
void set_ci(Result *res)
{
    res->ci_lo = res->price - kZ95 * res->std_err;
    res->ci_hi = res->price + kZ95 * res->std_err;
}

void finalize_into(double sum, double sumsq, uint64_t n, double r, double T, mcamd_result *res)
{
    const Estimate e = estimate(sum, sumsq, n, std::exp(-r * T));
    res->sum = sum;
    res->sumsq = sumsq;
    res->n = n;
    res->price = e.value;
    res->std_err = e.std_err;
    set_ci(res);
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

// a price record with the work counters behind it: {sum, sumsq, wave-steps, live lane-steps}
void finalize_counted_into(const double rec[4], uint64_t n, double r, double T, mcamd_result *res)
{
    finalize_into(rec[0], rec[1], n, r, T, res);
    res->work_steps = 64.0 * rec[2];   // wave-steps x 64 lanes
    res->live_steps = rec[3];
}

// price / SE / CI of a pricing record: {sum, sumsq} or, with the control variate, the five sums
void finalize_record(const double *rec, bool control_variate, uint64_t n, double r, double T, mcamd_result *res)
{
    if (control_variate) finalize_cv_into(rec, n, r, T, res);
    else finalize_into(rec[0], rec[1], n, r, T, res);
}

// a nested-MC record over n points: the mean point price is the scalar diagnostic of the wrappers
// (inc/wrappers.cuh:185-189,316-321)
void finalize_nmc_into(const double rec[mcamd::kNmcRecord], uint64_t n, mcamd_result *res)
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
    const uint64_t n = static_cast<uint64_t>(std::llround(stats[mcamd::kGreeksRecord]));
    out->n = n;
    for (int k = 0; k < mcamd::kGreeks; ++k) {
        const Estimate e = estimate(stats[2 * k], stats[2 * k + 1], n, disc);
        out->sum[k] = stats[2 * k];
        out->sumsq[k] = stats[2 * k + 1];
        out->value[k] = e.value;
        out->std_err[k] = e.std_err;
    }
    if (!theta_defined) out->value[MCAMD_GREEK_THETA] = out->std_err[MCAMD_GREEK_THETA] = std::nan("");
}

// Synchronous driver.  The kernel runs between ev0 and ev1 and finishes into the pinned record (kFolded: one launch is
// the whole call, total_ms = kernel_ms), or a separate sum into d_out and one copy run up to ev2.  After the wait,
// fill(record) fills *res from the final record; then the timings and the launch shape.  res must be zeroed by the
// caller: an empty shard leaves it so.
template <typename Launch, typename Result, typename Fill>
int run_sync(mcamd_ctx *ctx, const DeviceCall<Launch> &call, Result *res, Fill fill)
{
    if (call.n == 0) return MCAMD_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = ensure_partials(ctx, call.grid, call.rec)) return rc;
    const bool folded = call.how == Finish::kFolded;
    mcamd::FinishSpec fs;
    if (folded) {
        fs.out = ctx->h_rec_dev;
        fs.ticket = ctx->d_ticket;
        arm_record(ctx->h_rec, mcamd_ctx::kRecord);
    }
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    HIP_TRY(call.launch(fs));
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    if (!folded) {
        if (call.how == Finish::kSmall)
            HIP_TRY(mcamd::launch_small_final(ctx->d_partials, call.grid, call.rec, ctx->d_out, ctx->stream));
        else
            HIP_TRY(mcamd::launch_final_reduce(ctx->d_partials, call.grid, call.rec, ctx->d_out, ctx->stream));
        HIP_TRY(hipMemcpyAsync(ctx->h_rec, ctx->d_out, call.rec * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipEventRecord(ctx->ev2, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    float kernel_ms = 0.0f, total_ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&kernel_ms, ctx->ev0, ctx->ev1));
    if (folded) total_ms = kernel_ms;
    else HIP_TRY(hipEventElapsedTime(&total_ms, ctx->ev0, ctx->ev2));
    double record[mcamd_ctx::kRecord];
    std::memcpy(record, ctx->h_rec, sizeof record);
    if (folded && record_unwritten(record, call.rec))
        return fail(MCAMD_ERR_HIP, "the kernel left no result (its last workgroup did not finish the sum)");
    fill(static_cast<const double *>(record));
    res->kernel_ms = kernel_ms;
    res->total_ms = total_ms;
    res->grid = call.grid;
    res->block = mcamd::kBlockThreads;
    return MCAMD_OK;
}

// Asynchronous driver: the kernel runs between a pair of ring events, and its record reaches d_stats in the statistics
// layout with n_value = n, from the kernel itself (kFolded) or from the separate sum.  Nothing waits on the host but the
// growth of the scratch buffer.  An empty shard leaves all-zero statistics, still ordered on the stream.
template <typename Launch>
int run_enqueue(mcamd_ctx *ctx, const DeviceCall<Launch> &call, double *d_stats)
{
    if (!d_stats) return fail(MCAMD_ERR_INVALID, "d_stats is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t slot = static_cast<uint32_t>(ctx->n_enqueued % mcamd_ctx::kRing);
    if (call.n == 0) {
        HIP_TRY(hipMemsetAsync(d_stats, 0, call.stats * sizeof(double), ctx->stream));
        HIP_TRY(hipEventRecord(ctx->ring0[slot], ctx->stream));
        HIP_TRY(hipEventRecord(ctx->ring1[slot], ctx->stream));
        ctx->n_enqueued++;
        return MCAMD_OK;
    }
    const double n_value = static_cast<double>(call.n);
    // growing the scratch buffer frees the old one: wait for work that may still read it
    if (static_cast<uint64_t>(call.grid) * call.rec > ctx->partial_capacity) HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (int rc = ensure_partials(ctx, call.grid, call.rec)) return rc;
    mcamd::FinishSpec fs;
    if (call.how == Finish::kFolded) {
        fs.out = d_stats;
        fs.ticket = ctx->d_ticket;
        fs.n_value = n_value;
    }
    HIP_TRY(hipEventRecord(ctx->ring0[slot], ctx->stream));
    HIP_TRY(call.launch(fs));
    HIP_TRY(hipEventRecord(ctx->ring1[slot], ctx->stream));
    if (call.how == Finish::kSmall)
        HIP_TRY(mcamd::launch_small_final(ctx->d_partials, call.grid, call.rec, d_stats, ctx->stream, n_value));
    else if (call.how == Finish::kReduce)
        HIP_TRY(mcamd::launch_final_reduce(ctx->d_partials, call.grid, call.rec, d_stats, ctx->stream, n_value));
    ctx->n_enqueued++;
    return MCAMD_OK;
}

// The prepare_* steps below hold the argument checks and the job of a call with a synchronous and an enqueue form.
// Once every check has passed they hand the DeviceCall to drive (the form's driver) and return what it returns.

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
    return drive(DeviceCall{job.n_local, grid, (job.vr & 2) ? 5 : 2, 6, how, [&](const mcamd::FinishSpec &fs) {
        return mcamd::launch_price(job, ctx->compute_units, ctx->d_partials, ctx->d_queue, grid, fs, ctx->stream);
    }});
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
    const double dt = opt->dt > 0.0 ? opt->dt : opt->T / static_cast<double>(sim->n_steps);
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
// The refusals of the American calls that depend on the request's shape alone (shared with the workspace-size query):
// dates and basis size on success.
int check_american_shape(const mcamd_sim *sim, const mcamd_american *am, uint32_t *M, int *n_basis)
{
    if (am->payoff != MCAMD_PAYOFF_CALL && am->payoff != MCAMD_PAYOFF_PUT)
        return fail(MCAMD_ERR_INVALID, "payoff must be MCAMD_PAYOFF_CALL (0) or MCAMD_PAYOFF_PUT (1), got %d", am->payoff);
    if (am->n_basis != 0 && (am->n_basis < 2 || am->n_basis > static_cast<uint32_t>(mcamd::kAmMaxBasis)))
        return fail(MCAMD_ERR_INVALID, "n_basis must be 2, 3 or 4 (0 = 3), got %u", am->n_basis);
    if (am->reserved != 0) return fail(MCAMD_ERR_INVALID, "am->reserved must be 0, got %u", am->reserved);
    if (sim->precision != MCAMD_F32 && sim->precision != MCAMD_F64)
        return fail(MCAMD_ERR_INVALID, "precision must be MCAMD_F32 (32) or MCAMD_F64 (64), got %d", sim->precision);
    if (sim->n_steps == 0) return fail(MCAMD_ERR_INVALID, "n_steps must be >= 1");
    if (am->exercise_every == 0 || sim->n_steps % am->exercise_every != 0)
        return fail(MCAMD_ERR_INVALID, "exercise_every = %u must be >= 1 and divide n_steps = %u", am->exercise_every,
                    sim->n_steps);
    if (am->n_train == 0) return fail(MCAMD_ERR_INVALID, "n_train must be >= 1");
    const uint32_t dates = sim->n_steps / am->exercise_every;
    if (dates > mcamd::kAmMaxDates)
        return fail(MCAMD_ERR_INVALID, "n_steps / exercise_every = %u exercise dates; at most %u are supported", dates,
                    mcamd::kAmMaxDates);
    if (static_cast<long double>(am->n_train) * sim->n_steps * 8.0L >= 9.2e18L)
        return fail(MCAMD_ERR_INVALID, "n_train * n_steps overflows the training workspace's 64-bit size");
    *M = dates;
    *n_basis = am->n_basis ? static_cast<int>(am->n_basis) : 3;
    return MCAMD_OK;
}

// The refusals of the dual-bound calls that depend on the request's shape alone (shared with the workspace-size query).
// am->n_train and am->train_seed play no part: the rule comes in as a table.
int check_dual_shape(const mcamd_sim *sim, const mcamd_american *am, const mcamd_american_dual *dual, uint32_t *M,
                     int *n_basis)
{
    mcamd_american shape = *am;
    shape.n_train = 1;
    if (int rc = check_american_shape(sim, &shape, M, n_basis)) return rc;
    if (dual->n_inner == 0) return fail(MCAMD_ERR_INVALID, "n_inner must be >= 1");
    if (dual->reserved != 0) return fail(MCAMD_ERR_INVALID, "dual->reserved must be 0, got %u", dual->reserved);
    if (sim->path_offset + sim->n_paths_local < sim->path_offset)
        return fail(MCAMD_ERR_INVALID, "path_offset + n_paths_local overflows 64 bits");
    // continuation path i of point (g, j) draws Philox subsequence (g M + j) n_inner + i: the shard's largest one
    // must fit 64 bits
    const long double top = static_cast<long double>(sim->path_offset + sim->n_paths_local) * *M * dual->n_inner;
    if (top >= 18446744073709551615.0L)
        return fail(MCAMD_ERR_INVALID, "(path_offset + n_paths_local) * dates * n_inner overflows the 64-bit Philox "
                                       "subsequence");
    if (static_cast<long double>(sim->n_paths_local) * sim->n_steps * 8.0L >= 9.2e18L)
        return fail(MCAMD_ERR_INVALID, "n_paths_local * n_steps overflows the workspace's 64-bit size");
    return MCAMD_OK;
}

// The refusals of the barrier calls that depend on the request's enums and levels alone (shared with the closed form).
int check_barrier_kind(double S0, double B, int kind, int payoff)
{
    if (kind < MCAMD_BARRIER_DOWN_OUT || kind > MCAMD_BARRIER_UP_IN)
        return fail(MCAMD_ERR_INVALID, "barrier kind must be MCAMD_BARRIER_DOWN_OUT (0) .. MCAMD_BARRIER_UP_IN (3), got %d",
                    kind);
    if (payoff != MCAMD_PAYOFF_CALL && payoff != MCAMD_PAYOFF_PUT)
        return fail(MCAMD_ERR_INVALID, "payoff must be MCAMD_PAYOFF_CALL (0) or MCAMD_PAYOFF_PUT (1), got %d", payoff);
    if (!(B > 0.0) || !std::isfinite(B)) return fail(MCAMD_ERR_INVALID, "the barrier level B must be positive, got %g", B);
    const bool up = kind == MCAMD_BARRIER_UP_OUT || kind == MCAMD_BARRIER_UP_IN;
    if (!(S0 > 0.0) || !std::isfinite(S0) || !(up ? S0 < B : S0 > B))
        return fail(MCAMD_ERR_INVALID, "the spot must lie strictly on the live side of the barrier: %s (S0 = %g, B = %g)",
                    up ? "an up-barrier needs 0 < S0 < B" : "a down-barrier needs S0 > B", S0, B);
    return MCAMD_OK;
}

// The barrier calls.  The kernel always finishes its own sum (one_path_per_thread_grid caps the grid); every refusal
// that depends on the request alone comes before the context is looked at.
template <typename Drive>
int prepare_barrier(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_barrier *bar,
                    void *d_samples, Drive drive)
{
    if (!opt || !sim || !bar) return fail(MCAMD_ERR_INVALID, "opt, sim and barrier must be non-NULL");
    if (bar->monitoring != MCAMD_MONITOR_DISCRETE && bar->monitoring != MCAMD_MONITOR_CONTINUOUS)
        return fail(MCAMD_ERR_INVALID, "monitoring must be MCAMD_MONITOR_DISCRETE (0) or MCAMD_MONITOR_CONTINUOUS (1), "
                                       "got %d", bar->monitoring);
    if (bar->reserved != 0) return fail(MCAMD_ERR_INVALID, "barrier->reserved must be 0, got %d", bar->reserved);
    if (int rc = check_barrier_kind(opt->S0, opt->B, bar->kind, bar->payoff)) return rc;
    if (int rc = check_spot_start("barrier", false, opt, sim)) return rc;
    if (int rc = check_request(opt, sim)) return rc;
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (sim->n_paths_local == 0) return drive(empty_call());
    mcamd::BarrierJob job;
    job.path = make_plain_job(opt, sim, false, true);
    job.up = bar->kind == MCAMD_BARRIER_UP_OUT || bar->kind == MCAMD_BARRIER_UP_IN;
    job.out = bar->kind == MCAMD_BARRIER_DOWN_OUT || bar->kind == MCAMD_BARRIER_UP_OUT;
    job.continuous = bar->monitoring == MCAMD_MONITOR_CONTINUOUS;
    job.put = bar->payoff == MCAMD_PAYOFF_PUT;
    job.kq = 2.0 / (opt->v * opt->v * (opt->T / static_cast<double>(sim->n_steps)));
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(job.path.n_local);
    return drive(DeviceCall{job.path.n_local, grid, mcamd::kBarrierRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_barrier(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

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

// What the local-volatility calls (name: how the messages call the product) refuse of the option, the flags and sim
// through the checks shared with the other calls.  seen: the caller's copy of the option with every field it does not
// read made harmless; it carries no volatility of its own, so check_spot_start sees v = 1 and check_request v = 0,
// which leaves each drift mu[j] = r - q_j alone in the fp64 exponent-range bound.
int check_localvol_request(const char *name, mcamd_option seen, const mcamd_sim *sim, const double *mu, int n_mu)
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

// The local-volatility calls.  The kernel always finishes its own sum (one_path_per_thread_grid caps the grid); every
// refusal that depends on the request alone comes before the context is looked at, and all that do not need the
// surface before the surface is.  opt->v is ignored.
template <typename Drive>
int prepare_localvol(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_localvol *lv,
                     const mcamd_localvol_surface *surface, void *d_samples, Drive drive)
{
    if (!opt || !sim || !lv) return fail(MCAMD_ERR_INVALID, "opt, sim, localvol and surface must be non-NULL");
    if (lv->payoff != MCAMD_PAYOFF_CALL && lv->payoff != MCAMD_PAYOFF_PUT)
        return fail(MCAMD_ERR_INVALID, "payoff must be MCAMD_PAYOFF_CALL (0) or MCAMD_PAYOFF_PUT (1), got %d", lv->payoff);
    if (lv->barrier != MCAMD_LOCALVOL_NO_BARRIER && (lv->barrier < MCAMD_BARRIER_DOWN_OUT || lv->barrier > MCAMD_BARRIER_UP_IN))
        return fail(MCAMD_ERR_INVALID, "localvol->barrier must be MCAMD_LOCALVOL_NO_BARRIER (-1) or MCAMD_BARRIER_DOWN_OUT (0) "
                                       ".. MCAMD_BARRIER_UP_IN (3), got %d", lv->barrier);
    if (lv->monitoring != MCAMD_MONITOR_DISCRETE && lv->monitoring != MCAMD_MONITOR_CONTINUOUS)
        return fail(MCAMD_ERR_INVALID, "monitoring must be MCAMD_MONITOR_DISCRETE (0) or MCAMD_MONITOR_CONTINUOUS (1), "
                                       "got %d", lv->monitoring);
    if (lv->reserved != 0) return fail(MCAMD_ERR_INVALID, "localvol->reserved must be 0, got %d", lv->reserved);
    if (!std::isfinite(lv->q)) return fail(MCAMD_ERR_INVALID, "the dividend yield q must be finite, got %g", lv->q);
    const bool barrier = lv->barrier != MCAMD_LOCALVOL_NO_BARRIER;
    if (barrier) {
        if (int rc = check_barrier_kind(opt->S0, opt->B, lv->barrier, lv->payoff)) return rc;
    }
    if (!std::isfinite(opt->r)) return fail(MCAMD_ERR_INVALID, "option parameters must be finite with T > 0");
    const double mu = opt->r - lv->q;
    if (int rc = check_localvol_request("local-volatility", *opt, sim, &mu, 1)) return rc;
    if (!(opt->S0 > 0.0)) return fail(MCAMD_ERR_INVALID, "local-volatility options need S0 > 0 (S0 = %g)", opt->S0);
    if (!surface) return fail(MCAMD_ERR_INVALID, "opt, sim, localvol and surface must be non-NULL");
    const double dt = opt->T / static_cast<double>(sim->n_steps);
    if (sim->precision == MCAMD_F64)
        if (int rc = check_localvol_exponent_range(mu, surface->sigma_max, dt, sim->n_steps)) return rc;
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (!surface_belongs(surface, ctx)) return fail(MCAMD_ERR_INVALID, "the surface was created on another context");
    if (sim->n_paths_local == 0) return drive(empty_call());
    mcamd::LocalVolJob job;
    job.seed = sim->seed;
    job.path_offset = sim->path_offset;
    job.n_local = sim->n_paths_local;
    job.n_steps = sim->n_steps;
    job.precision = sim->precision;
    job.S0 = opt->S0;
    job.K = opt->K;
    job.B = opt->B;
    job.mu = mu;
    job.dt = dt;
    job.barrier = barrier;
    job.up = lv->barrier == MCAMD_BARRIER_UP_OUT || lv->barrier == MCAMD_BARRIER_UP_IN;
    job.out = lv->barrier == MCAMD_BARRIER_DOWN_OUT || lv->barrier == MCAMD_BARRIER_UP_OUT;
    job.continuous = barrier && lv->monitoring == MCAMD_MONITOR_CONTINUOUS;
    job.put = lv->payoff == MCAMD_PAYOFF_PUT;
    job.surface = job_surface(surface, sim->precision);
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(job.n_local);
    return drive(DeviceCall{job.n_local, grid, mcamd::kLocalVolRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_localvol(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
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

// The cliquet calls: mcamd_price_localvol's paths without a barrier.  The refusals follow prepare_localvol's order: the
// request alone, then the surface, then the context.  opt->v, opt->K and opt->B are ignored, and S0 is read by nothing.
template <typename Drive>
int prepare_cliquet(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_cliquet *cq,
                    const mcamd_localvol_surface *surface, void *d_samples, Drive drive)
{
    if (!opt || !sim || !cq) return fail(MCAMD_ERR_INVALID, "opt, sim, cliquet and surface must be non-NULL");
    if (int rc = check_cliquet_kind(cq->kind)) return rc;
    if (cq->reserved != 0) return fail(MCAMD_ERR_INVALID, "cliquet->reserved must be 0, got %d", cq->reserved);
    if (cq->reset_every == 0 || sim->n_steps % cq->reset_every != 0)
        return fail(MCAMD_ERR_INVALID, "reset_every must be >= 1 and divide n_steps (reset_every = %u, n_steps = %u)",
                    cq->reset_every, sim->n_steps);
    const uint32_t M = sim->n_steps / cq->reset_every;
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
    if (!std::isfinite(cq->q)) return fail(MCAMD_ERR_INVALID, "the dividend yield q must be finite, got %g", cq->q);
    if (!std::isfinite(opt->r)) return fail(MCAMD_ERR_INVALID, "option parameters must be finite with T > 0");
    const double mu = opt->r - cq->q;
    // as prepare_localvol, on a copy that carries no spot, strike or barrier of its own either
    mcamd_option seen = *opt;
    seen.S0 = 1.0;
    seen.K = seen.B = 0.0;
    if (int rc = check_localvol_request("cliquet", seen, sim, &mu, 1)) return rc;
    if (!surface) return fail(MCAMD_ERR_INVALID, "opt, sim, cliquet and surface must be non-NULL");
    const double dt = opt->T / static_cast<double>(sim->n_steps);
    if (sim->precision == MCAMD_F64)
        if (int rc = check_localvol_exponent_range(mu, surface->sigma_max, dt, sim->n_steps)) return rc;
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (!surface_belongs(surface, ctx)) return fail(MCAMD_ERR_INVALID, "the surface was created on another context");
    if (sim->n_paths_local == 0) return drive(empty_call());
    mcamd::CliquetJob job;
    job.seed = sim->seed;
    job.path_offset = sim->path_offset;
    job.n_local = sim->n_paths_local;
    job.n_steps = sim->n_steps;
    job.precision = sim->precision;
    job.kind = cq->kind;
    job.reset_every = cq->reset_every;
    job.first_period = cq->first_period;
    job.mu = mu;
    job.dt = dt;
    const bool compound = cq->kind == MCAMD_CLIQUET_COMPOUND;
    job.local_lo = compound ? std::log(1.0 + cq->local_floor) : cq->local_floor;
    job.local_hi = compound ? std::log(1.0 + cq->local_cap) : cq->local_cap;
    job.global_lo = cq->global_floor;
    job.global_hi = cq->global_cap;
    const double P = static_cast<double>(M - cq->first_period + 1);
    job.scale = 1.0 / (P * (static_cast<double>(cq->reset_every) * dt));
    job.surface = job_surface(surface, sim->precision);
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(job.n_local);
    return drive(DeviceCall{job.n_local, grid, mcamd::kCliquetRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_cliquet(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

// value / std_err / sums of a (possibly all-reduced) 32-double local-volatility Greeks record
void finalize_localvol_greeks_into(const double stats[32], double r, double T, uint32_t n_buckets, int gamma_defined,
                                   mcamd_localvol_greeks *out)
{
    const double disc = std::exp(-r * T);
    const uint64_t n = static_cast<uint64_t>(std::llround(stats[mcamd::kLvGreeksRecord]));
    out->n = n;
    for (int k = 0; k < mcamd::kLvGreeks; ++k) {
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
        const double *pair = stats + 2 * (mcamd::kLvGreeks + b);
        const Estimate e = estimate(pair[0], pair[1], n, disc);
        out->bucket_sum[b] = pair[0];
        out->bucket_sumsq[b] = pair[1];
        out->bucket_value[b] = e.value;
        out->bucket_std_err[b] = e.std_err;
    }
}

// The local-volatility Greeks calls: prepare_localvol's refusals for a barrier-less job, in its order, with the
// job's own in between.  The kernel finishes its own sum into the 32-double statistics record.  opt->v is ignored.
template <typename Drive>
int prepare_localvol_greeks(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                            const mcamd_localvol_greeks_job *gj, const mcamd_localvol_surface *surface, double *d_samples,
                            Drive drive)
{
    if (!opt || !sim || !gj) return fail(MCAMD_ERR_INVALID, "opt, sim, job and surface must be non-NULL");
    if (gj->payoff != MCAMD_PAYOFF_CALL && gj->payoff != MCAMD_PAYOFF_PUT)
        return fail(MCAMD_ERR_INVALID, "payoff must be MCAMD_PAYOFF_CALL (0) or MCAMD_PAYOFF_PUT (1), got %d", gj->payoff);
    if (gj->n_vega_buckets > MCAMD_LOCALVOL_GREEKS_MAX_BUCKETS)
        return fail(MCAMD_ERR_INVALID, "n_vega_buckets must lie in 0 .. %d, got %u", MCAMD_LOCALVOL_GREEKS_MAX_BUCKETS,
                    gj->n_vega_buckets);
    if (!std::isfinite(gj->gamma_bump) || gj->gamma_bump < 0.0 || gj->gamma_bump > 0.1)
        return fail(MCAMD_ERR_INVALID, "gamma_bump must be finite and lie in 0 .. 0.1, got %g", gj->gamma_bump);
    if (!std::isfinite(gj->q)) return fail(MCAMD_ERR_INVALID, "the dividend yield q must be finite, got %g", gj->q);
    if (!std::isfinite(opt->r)) return fail(MCAMD_ERR_INVALID, "option parameters must be finite with T > 0");
    const double mu = opt->r - gj->q;
    if (int rc = check_localvol_request("local-volatility Greeks", *opt, sim, &mu, 1)) return rc;
    if (!(opt->S0 > 0.0)) return fail(MCAMD_ERR_INVALID, "local-volatility Greeks need S0 > 0 (S0 = %g)", opt->S0);
    if (!surface) return fail(MCAMD_ERR_INVALID, "opt, sim, job and surface must be non-NULL");
    const double dt = opt->T / static_cast<double>(sim->n_steps);
    if (sim->precision == MCAMD_F64)
        if (int rc = check_localvol_exponent_range(mu, surface->sigma_max, dt, sim->n_steps, -1, gj->gamma_bump)) return rc;
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (!surface_belongs(surface, ctx)) return fail(MCAMD_ERR_INVALID, "the surface was created on another context");
    if (sim->n_paths_local == 0) return drive(empty_call(mcamd::kLvGreeksStats));
    mcamd::LocalVolGreeksJob job;
    job.seed = sim->seed;
    job.path_offset = sim->path_offset;
    job.n_local = sim->n_paths_local;
    job.n_steps = sim->n_steps;
    job.precision = sim->precision;
    job.S0 = opt->S0;
    job.K = opt->K;
    job.mu = mu;
    job.dt = dt;
    job.T = opt->T;
    job.put = gj->payoff == MCAMD_PAYOFF_PUT;
    job.n_buckets = gj->n_vega_buckets;
    job.gamma_bump = gj->gamma_bump;
    job.surface = job_surface(surface, sim->precision);
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(job.n_local);
    return drive(DeviceCall{job.n_local, grid, mcamd::kLvGreeksRecord, mcamd::kLvGreeksStats, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_localvol_greeks(job, ctx->d_partials, grid, fs.out, fs.ticket,
                                                                     ctx->stream);
                            }});
}

// The smile calls: mcamd_price_localvol's paths without a barrier, stopped at the expiry steps, every strike priced at
// every expiry.  The refusals follow prepare_localvol's order: the request alone, then the surface, then the context.
// drive(job, grid) runs the form's driver; grid == 0 is the empty shard.  opt->v and opt->K are ignored.
template <typename Drive>
int prepare_smile(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_smile *sm,
                  const uint32_t *h_expiry_steps, const double *h_strikes, const mcamd_localvol_surface *surface,
                  void *d_spots, Drive drive)
{
    if (!opt || !sim || !sm || !h_expiry_steps || !h_strikes)
        return fail(MCAMD_ERR_INVALID, "opt, sim, smile, h_expiry_steps, h_strikes and surface must be non-NULL");
    if (sm->payoff != MCAMD_PAYOFF_CALL && sm->payoff != MCAMD_PAYOFF_PUT)
        return fail(MCAMD_ERR_INVALID, "payoff must be MCAMD_PAYOFF_CALL (0) or MCAMD_PAYOFF_PUT (1), got %d", sm->payoff);
    if (sm->reserved != 0) return fail(MCAMD_ERR_INVALID, "smile->reserved must be 0, got %d", sm->reserved);
    if (sm->n_expiries < 1 || sm->n_expiries > MCAMD_SMILE_MAX_EXPIRIES)
        return fail(MCAMD_ERR_INVALID, "n_expiries must lie in 1 .. %d, got %u", MCAMD_SMILE_MAX_EXPIRIES, sm->n_expiries);
    if (sm->n_strikes < 1 || sm->n_strikes > MCAMD_SMILE_MAX_STRIKES)
        return fail(MCAMD_ERR_INVALID, "n_strikes must lie in 1 .. %d, got %u", MCAMD_SMILE_MAX_STRIKES, sm->n_strikes);
    for (uint32_t m = 0; m < sm->n_expiries; ++m) {
        const uint32_t before = m ? h_expiry_steps[m - 1] : 0;
        if (h_expiry_steps[m] <= before || h_expiry_steps[m] > sim->n_steps)
            return fail(MCAMD_ERR_INVALID, "expiry steps must be strictly ascending in 1 .. n_steps = %u: "
                                           "h_expiry_steps[%u] = %u", sim->n_steps, m, h_expiry_steps[m]);
    }
    for (uint32_t k = 0; k < sm->n_strikes; ++k)
        if (!std::isfinite(h_strikes[k]) || !(h_strikes[k] > 0.0))
            return fail(MCAMD_ERR_INVALID, "every strike must be finite and > 0: h_strikes[%u] = %g", k, h_strikes[k]);
    if (!std::isfinite(sm->q)) return fail(MCAMD_ERR_INVALID, "the dividend yield q must be finite, got %g", sm->q);
    if (!std::isfinite(opt->r)) return fail(MCAMD_ERR_INVALID, "option parameters must be finite with T > 0");
    // as prepare_localvol, on a copy that carries no strike of its own either
    const double mu = opt->r - sm->q;
    mcamd_option seen = *opt;
    seen.K = 1.0;
    if (int rc = check_localvol_request("local-volatility smile", seen, sim, &mu, 1)) return rc;
    if (!(opt->S0 > 0.0)) return fail(MCAMD_ERR_INVALID, "local-volatility smile options need S0 > 0 (S0 = %g)", opt->S0);
    if (!surface)
        return fail(MCAMD_ERR_INVALID, "opt, sim, smile, h_expiry_steps, h_strikes and surface must be non-NULL");
    const double dt = opt->T / static_cast<double>(sim->n_steps);
    if (sim->precision == MCAMD_F64)
        if (int rc = check_localvol_exponent_range(mu, surface->sigma_max, dt, sim->n_steps)) return rc;
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (!surface_belongs(surface, ctx)) return fail(MCAMD_ERR_INVALID, "the surface was created on another context");
    mcamd::SmileJob job = {};
    job.seed = sim->seed;
    job.path_offset = sim->path_offset;
    job.n_local = sim->n_paths_local;
    job.n_steps = sim->n_steps;
    job.precision = sim->precision;
    job.S0 = opt->S0;
    job.mu = mu;
    job.dt = dt;
    job.put = sm->payoff == MCAMD_PAYOFF_PUT;
    job.surface = job_surface(surface, sim->precision);
    job.n_expiries = sm->n_expiries;
    job.n_strikes = sm->n_strikes;
    std::copy(h_expiry_steps, h_expiry_steps + sm->n_expiries, job.expiry_steps);
    std::copy(h_strikes, h_strikes + sm->n_strikes, job.strikes);
    job.d_spots = d_spots;
    const uint32_t grid = job.n_local ? mcamd::smile_grid(job.n_local, job.n_expiries, job.n_strikes, ctx->compute_units) : 0;
    return drive(job, grid);
}

// price and standard error of every node of a smile from its 2 n_e n_K sums, each discounted to its own expiry
void finalize_smile_into(const double *stats, uint64_t n, double r, double T, uint32_t n_steps, uint32_t n_e, uint32_t n_K,
                         const uint32_t *expiry_steps, double *price, double *std_err)
{
    const uint32_t nodes = n_e * n_K;
    const double dt = T / static_cast<double>(n_steps);
    for (uint32_t m = 0; m < n_e; ++m) {
        const double disc = std::exp(-r * (static_cast<double>(expiry_steps[m]) * dt));
        for (uint32_t k = 0; k < n_K; ++k) {
            const Estimate e = estimate(stats[m * n_K + k], stats[nodes + m * n_K + k], n, disc);
            if (price) price[m * n_K + k] = e.value;
            if (std_err) std_err[m * n_K + k] = e.std_err;
        }
    }
}

// Black-Scholes with a dividend yield at volatility v > 0 and its vega; every argument checked by the caller
double bs_value(double S0, double K, double T, double r, double q, double v, bool call, double *vega)
{
    const double sqrtT = std::sqrt(T);
    const double d1 = (std::log(S0 / K) + (r - q + 0.5 * v * v) * T) / (v * sqrtT), d2 = d1 - v * sqrtT;
    const auto N = [](double x) { return 0.5 * std::erfc(-x / std::sqrt(2.0)); };
    const double Sd = S0 * std::exp(-q * T), Kd = K * std::exp(-r * T);
    if (vega) *vega = Sd * sqrtT * std::exp(-0.5 * d1 * d1) * 0.3989422804014327;
    return call ? Sd * N(d1) - Kd * N(d2) : Kd * N(-d2) - Sd * N(-d1);
}

// The refusals of the lookback calls that depend on the product alone (shared with the closed form).
int check_lookback_kind(double K, int strike, int payoff)
{
    if (strike != MCAMD_LOOKBACK_FLOATING && strike != MCAMD_LOOKBACK_FIXED)
        return fail(MCAMD_ERR_INVALID, "strike must be MCAMD_LOOKBACK_FLOATING (0) or MCAMD_LOOKBACK_FIXED (1), got %d",
                    strike);
    if (payoff != MCAMD_PAYOFF_CALL && payoff != MCAMD_PAYOFF_PUT)
        return fail(MCAMD_ERR_INVALID, "payoff must be MCAMD_PAYOFF_CALL (0) or MCAMD_PAYOFF_PUT (1), got %d", payoff);
    if (strike == MCAMD_LOOKBACK_FIXED && (!(K > 0.0) || !std::isfinite(K)))
        return fail(MCAMD_ERR_INVALID, "a fixed-strike lookback needs a finite K > 0, got %g", K);
    return MCAMD_OK;
}

// The lookback calls.  The kernel always finishes its own sum (one_path_per_thread_grid caps the grid); every refusal
// that depends on the request alone comes before the context is looked at.
template <typename Drive>
int prepare_lookback(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_lookback *lb,
                     void *d_samples, Drive drive)
{
    if (!opt || !sim || !lb) return fail(MCAMD_ERR_INVALID, "opt, sim and lookback must be non-NULL");
    if (lb->monitoring != MCAMD_MONITOR_DISCRETE && lb->monitoring != MCAMD_MONITOR_CONTINUOUS)
        return fail(MCAMD_ERR_INVALID, "monitoring must be MCAMD_MONITOR_DISCRETE (0) or MCAMD_MONITOR_CONTINUOUS (1), "
                                       "got %d", lb->monitoring);
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
    job.v2dt = opt->v * opt->v * (opt->T / static_cast<double>(sim->n_steps));
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(job.path.n_local);
    return drive(DeviceCall{job.path.n_local, grid, mcamd::kLookbackRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_lookback(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

// The refusals of the Asian calls that depend on the product alone (shared with the closed form).
int check_asian_kind(double K, int strike, int payoff, int include_spot)
{
    if (strike != MCAMD_ASIAN_FIXED && strike != MCAMD_ASIAN_FLOATING)
        return fail(MCAMD_ERR_INVALID, "strike must be MCAMD_ASIAN_FIXED (0) or MCAMD_ASIAN_FLOATING (1), got %d", strike);
    if (payoff != MCAMD_PAYOFF_CALL && payoff != MCAMD_PAYOFF_PUT)
        return fail(MCAMD_ERR_INVALID, "payoff must be MCAMD_PAYOFF_CALL (0) or MCAMD_PAYOFF_PUT (1), got %d", payoff);
    if (include_spot != 0 && include_spot != 1)
        return fail(MCAMD_ERR_INVALID, "include_spot must be 0 or 1, got %d", include_spot);
    if (strike == MCAMD_ASIAN_FIXED && (!(K > 0.0) || !std::isfinite(K)))
        return fail(MCAMD_ERR_INVALID, "a fixed-strike Asian option needs a finite K > 0, got %g", K);
    return MCAMD_OK;
}

// The discrete geometric average of geometric Brownian motion over the step ends i = 1..n (and t = 0 with
// include_spot; m dates in all) is lognormal: ln G ~ N(M, s^2) with M = ln S0 + mu dt n(n+1) / (2m) and
// s^2 = v^2 dt n(n+1)(2n+1) / (6 m^2), mu = r - v^2/2.  The floating strike exchanges G for S_T, two lognormals with
// covariance v^2 dt n(n+1) / (2m) of their logarithms (Margrabe's form on the forwards).
int asian_geometric_price(double S0, double K, double T, double r, double v, uint32_t n_steps, int include_spot,
                          int strike, int payoff, double *price)
{
    *price = 0.0;
    if (!(S0 > 0.0) || !(T > 0.0) || !(v > 0.0) || !std::isfinite(S0) || !std::isfinite(T) || !std::isfinite(r) ||
        !std::isfinite(v))
        return fail(MCAMD_ERR_INVALID, "the geometric Asian closed form needs finite S0, T, v > 0 and a finite r");
    if (n_steps == 0) return fail(MCAMD_ERR_INVALID, "n_steps must be >= 1");
    if (int rc = check_asian_kind(K, strike, payoff, include_spot)) return rc;
    const double n = static_cast<double>(n_steps), m = n + include_spot, dt = T / n;
    const double mu = r - 0.5 * v * v, D = std::exp(-r * T);
    const double M = std::log(S0) + mu * dt * n * (n + 1.0) / (2.0 * m);
    const double s2 = v * v * dt * n * (n + 1.0) * (2.0 * n + 1.0) / (6.0 * m * m);
    const double F = std::exp(M + 0.5 * s2);   // E[G]
    const auto N = [](double x) { return 0.5 * std::erfc(-x / std::sqrt(2.0)); };
    const bool put = payoff == MCAMD_PAYOFF_PUT;
    if (strike == MCAMD_ASIAN_FIXED) {
        const double s = std::sqrt(s2);
        const double d1 = (M - std::log(K)) / s + s;
        const double call = D * (F * N(d1) - K * N(d1 - s));
        *price = put ? call - D * (F - K) : call;
        return MCAMD_OK;
    }
    const double sf2 = v * v * T + s2 - v * v * dt * n * (n + 1.0) / m;
    // one step without the spot: the average IS S_T, and the option pays nothing
    if ((n_steps == 1 && !include_spot) || !(sf2 > 0.0)) return MCAMD_OK;
    const double F1 = S0 * std::exp(r * T), sf = std::sqrt(sf2);
    const double d1 = (std::log(F1 / F) + 0.5 * sf2) / sf;
    const double call = D * (F1 * N(d1) - F * N(d1 - sf));
    *price = put ? call - D * (F1 - F) : call;
    return MCAMD_OK;
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

// The refusals of the basket calls that depend on the assets alone (shared with the geometric closed form).  Leaves the
// lower Cholesky factor of corr[:d, :d] in L (row-major, stride 8; entries above the diagonal 0).
int check_basket_assets(const mcamd_basket *b, bool positive_weights, double L[64])
{
    const int d = b->n_assets;
    if (d < 1 || d > MCAMD_BASKET_MAX_ASSETS)
        return fail(MCAMD_ERR_INVALID, "n_assets must be 1..%d, got %d", MCAMD_BASKET_MAX_ASSETS, d);
    if (b->payoff != MCAMD_PAYOFF_CALL && b->payoff != MCAMD_PAYOFF_PUT)
        return fail(MCAMD_ERR_INVALID, "payoff must be MCAMD_PAYOFF_CALL (0) or MCAMD_PAYOFF_PUT (1), got %d", b->payoff);
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
    const double dt = opt->T / static_cast<double>(sim->n_steps), sqdt = std::sqrt(dt);
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

// The autocall calls.  The kernel always finishes its own sum (one_path_per_thread_grid caps the grid); every refusal
// that depends on the request alone comes before the context is looked at.
template <typename Drive>
int prepare_autocall(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_autocall *ac,
                     void *d_samples, Drive drive)
{
    if (!opt || !sim || !ac) return fail(MCAMD_ERR_INVALID, "opt, sim and autocall must be non-NULL");
    if (ac->reserved[0] != 0 || ac->reserved[1] != 0)
        return fail(MCAMD_ERR_INVALID, "autocall->reserved must be 0, got {%d, %d}", ac->reserved[0], ac->reserved[1]);
    // the assets through the basket's own checks and Cholesky factor: performances have spot 1 and weight 1
    mcamd_basket assets{};
    assets.n_assets = ac->n_assets;
    assets.payoff = MCAMD_PAYOFF_PUT;
    for (int j = 0; j < MCAMD_BASKET_MAX_ASSETS; ++j) {
        assets.S0[j] = assets.w[j] = 1.0;
        assets.v[j] = ac->v[j];
    }
    std::memcpy(assets.corr, ac->corr, sizeof assets.corr);
    double L[64];
    if (int rc = check_basket_assets(&assets, true, L)) return rc;
    const int d = ac->n_assets;
    if (ac->observe_every == 0 || sim->n_steps % ac->observe_every != 0)
        return fail(MCAMD_ERR_INVALID, "observe_every must be >= 1 and divide n_steps (observe_every = %u, n_steps = %u)",
                    ac->observe_every, sim->n_steps);
    const uint32_t M = sim->n_steps / ac->observe_every;
    if (M > MCAMD_AUTOCALL_MAX_DATES)   // M == 0 is n_steps == 0, which check_request refuses below
        return fail(MCAMD_ERR_INVALID, "n_steps / observe_every = %u observation dates exceed MCAMD_AUTOCALL_MAX_DATES = %d",
                    M, MCAMD_AUTOCALL_MAX_DATES);
    if (M != 0 && (ac->first_call_date < 1 || ac->first_call_date > M))
        return fail(MCAMD_ERR_INVALID, "first_call_date must be 1..%u (the observation dates), got %u", M,
                    ac->first_call_date);
    const double L_last = ac->call_level - (static_cast<double>(M) - 1.0) * ac->call_step_down;
    if (int rc = check_autocall_terms(ac->coupon, ac->call_level, ac->call_step_down, M ? L_last : ac->call_level,
                                      ac->ki_monitoring, ac->ki_level))
        return rc;
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
    const double dt = opt->T / static_cast<double>(sim->n_steps), sqdt = std::sqrt(dt);
    for (int j = 0; j < d; ++j) {
        job.drift[j] = (opt->r - 0.5 * ac->v[j] * ac->v[j]) * dt;
        for (int k = 0; k <= j; ++k) job.coef[j * (j + 1) / 2 + k] = ac->v[j] * sqdt * L[8 * j + k];
    }
    job.observe_every = ac->observe_every;
    job.n_dates = M;
    job.first_call_date = ac->first_call_date;
    for (uint32_t q = 1; q <= M; ++q) {
        const double t_q = static_cast<double>(q * ac->observe_every) * dt;
        job.log_level[q - 1] = std::log(ac->call_level - (static_cast<double>(q) - 1.0) * ac->call_step_down);
        job.pay[q - 1] = (1.0 + static_cast<double>(q) * ac->coupon) * std::exp(opt->r * (opt->T - t_q));
    }
    job.dt = dt;
    job.ki = ac->ki_monitoring != MCAMD_AUTOCALL_KI_NONE;
    job.ki_every_step = ac->ki_monitoring == MCAMD_AUTOCALL_KI_EVERY_STEP;
    job.log_ki = job.ki ? std::log(ac->ki_level) : 0.0;
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(job.path.n_local);
    return drive(DeviceCall{job.path.n_local, grid, mcamd::kAutocallRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_autocall(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
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
    // n_assets and corr through the basket's own checks and Cholesky factor: unit spots, weights and volatilities
    mcamd_basket assets{};
    assets.n_assets = ac->n_assets;
    assets.payoff = MCAMD_PAYOFF_PUT;
    for (int j = 0; j < MCAMD_BASKET_MAX_ASSETS; ++j) assets.S0[j] = assets.w[j] = assets.v[j] = 1.0;
    std::memcpy(assets.corr, ac->corr, sizeof assets.corr);
    double L[64];
    if (int rc = check_basket_assets(&assets, true, L)) return rc;
    const int d = ac->n_assets;
    for (int j = 0; j < d; ++j)
        if (!std::isfinite(ac->q[j]))
            return fail(MCAMD_ERR_INVALID, "every dividend yield q must be finite, got q[%d] = %g", j, ac->q[j]);
    if (ac->observe_every == 0 || sim->n_steps % ac->observe_every != 0)
        return fail(MCAMD_ERR_INVALID, "observe_every must be >= 1 and divide n_steps (observe_every = %u, n_steps = %u)",
                    ac->observe_every, sim->n_steps);
    const uint32_t M = sim->n_steps / ac->observe_every;
    if (M > MCAMD_AUTOCALL_MAX_DATES)   // M == 0 is n_steps == 0, which check_request refuses below
        return fail(MCAMD_ERR_INVALID, "n_steps / observe_every = %u observation dates exceed MCAMD_AUTOCALL_MAX_DATES = %d",
                    M, MCAMD_AUTOCALL_MAX_DATES);
    if (M != 0 && (ac->first_call_date < 1 || ac->first_call_date > M))
        return fail(MCAMD_ERR_INVALID, "first_call_date must be 1..%u (the observation dates), got %u", M,
                    ac->first_call_date);
    const double L_last = ac->call_level - (static_cast<double>(M) - 1.0) * ac->call_step_down;
    if (int rc = check_autocall_terms(ac->coupon, ac->call_level, ac->call_step_down, M ? L_last : ac->call_level,
                                      ac->ki_monitoring, ac->ki_level))
        return rc;
    if (!std::isfinite(opt->r)) return fail(MCAMD_ERR_INVALID, "option parameters must be finite with T > 0");
    // as prepare_localvol, asset by asset, on a copy that carries no spot, strike or barrier of its own either
    double mu[MCAMD_BASKET_MAX_ASSETS];
    for (int j = 0; j < d; ++j) mu[j] = opt->r - ac->q[j];
    mcamd_option seen = *opt;
    seen.S0 = 1.0;
    seen.K = seen.B = 0.0;
    if (int rc = check_localvol_request("local-volatility autocallable", seen, sim, mu, d)) return rc;
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
    const double dt = opt->T / static_cast<double>(sim->n_steps);
    if (sim->precision == MCAMD_F64)
        for (int j = 0; j < d; ++j)
            if (int rc = check_localvol_exponent_range(mu[j], surfaces[j]->sigma_max, dt, sim->n_steps, j)) return rc;
    if (!ctx) return fail(MCAMD_ERR_INVALID, "ctx is NULL");
    if (sim->n_paths_local == 0) return drive(empty_call());
    mcamd::AutocallLocalVolJob job{};
    job.seed = sim->seed;
    job.path_offset = sim->path_offset;
    job.n_local = sim->n_paths_local;
    job.n_steps = sim->n_steps;
    job.precision = sim->precision;
    job.d = d;
    job.dt = dt;
    for (int j = 0; j < d; ++j) {
        job.mu[j] = mu[j];
        for (int k = 0; k <= j; ++k) job.chol[j * (j + 1) / 2 + k] = L[8 * j + k];
        job.surface[j] = job_surface(surfaces[j], sim->precision);
    }
    job.observe_every = ac->observe_every;
    job.n_dates = M;
    job.first_call_date = ac->first_call_date;
    for (uint32_t q = 1; q <= M; ++q) {
        const double t_q = static_cast<double>(q * ac->observe_every) * dt;
        job.log_level[q - 1] = std::log(ac->call_level - (static_cast<double>(q) - 1.0) * ac->call_step_down);
        job.pay[q - 1] = (1.0 + static_cast<double>(q) * ac->coupon) * std::exp(opt->r * (opt->T - t_q));
    }
    job.ki = ac->ki_monitoring != MCAMD_AUTOCALL_KI_NONE;
    job.ki_every_step = ac->ki_monitoring == MCAMD_AUTOCALL_KI_EVERY_STEP;
    job.log_ki = job.ki ? std::log(ac->ki_level) : 0.0;
    job.d_samples = d_samples;
    const uint32_t grid = mcamd::one_path_per_thread_grid(job.n_local);
    return drive(DeviceCall{job.n_local, grid, mcamd::kAutocallRecord, 6, Finish::kFolded,
                            [&](const mcamd::FinishSpec &fs) {
                                return mcamd::launch_autocall_localvol(job, ctx->d_partials, grid, fs, ctx->stream);
                            }});
}

// h(S0) replaces an estimate it exceeds (exercise at t = 0); returns whether it did
bool floor_at_immediate(double h0, double *price, double *std_err)
{
    if (!(h0 > *price)) return false;
    *price = h0;
    *std_err = 0.0;
    return true;
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
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
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
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (uint32_t i = 0; i < n_last; ++i) {
        const uint32_t slot = static_cast<uint32_t>((ctx->n_enqueued - n_last + i) % mcamd_ctx::kRing);
        HIP_TRY(hipEventElapsedTime(&ms[i], ctx->ring0[slot], ctx->ring1[slot]));
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

int mcamd_bs_greeks_f64(double S0, double K, double T, double r, double v, double out[6])
{
    if (!out) return fail(MCAMD_ERR_INVALID, "out is NULL");
    if (!(S0 > 0.0) || !(K > 0.0) || !(T > 0.0) || !(v > 0.0) || !std::isfinite(S0) || !std::isfinite(K) ||
        !std::isfinite(T) || !std::isfinite(r) || !std::isfinite(v))
        return fail(MCAMD_ERR_INVALID, "closed-form Greeks need finite S0, K, T, v > 0 and a finite r");
    const double sqrtT = std::sqrt(T);
    const double d1 = (std::log(S0 / K) + (r + 0.5 * v * v) * T) / (v * sqrtT);
    const double d2 = d1 - v * sqrtT;
    const double Nd1 = 0.5 * std::erfc(-d1 / std::sqrt(2.0)), Nd2 = 0.5 * std::erfc(-d2 / std::sqrt(2.0));
    const double phi = std::exp(-0.5 * d1 * d1) / std::sqrt(2.0 * M_PI);
    const double Kdisc = K * std::exp(-r * T);
    out[MCAMD_GREEK_PRICE] = mcamd_bs_call_f64(S0, K, T, r, v);
    out[MCAMD_GREEK_DELTA] = Nd1;
    out[MCAMD_GREEK_GAMMA] = phi / (S0 * v * sqrtT);
    out[MCAMD_GREEK_VEGA] = S0 * phi * sqrtT;
    out[MCAMD_GREEK_RHO] = Kdisc * T * Nd2;
    out[MCAMD_GREEK_THETA] = -S0 * phi * v / (2.0 * sqrtT) - r * Kdisc * Nd2;
    return MCAMD_OK;
}

int mcamd_american_workspace_bytes(const mcamd_american *am, const mcamd_sim *sim, uint64_t *bytes)
{
    if (!am || !sim || !bytes) return fail(MCAMD_ERR_INVALID, "am, sim and bytes must be non-NULL");
    *bytes = 0;
    uint32_t M = 0;
    int n_basis = 0;
    if (int rc = check_american_shape(sim, am, &M, &n_basis)) return rc;
    *bytes = mcamd::american_layout(am->n_train, sim->n_steps, M, sim->precision).total;
    return MCAMD_OK;
}

int mcamd_price_american(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_american *am,
                         void *d_work, uint64_t work_bytes, double *h_coeffs, mcamd_american_result *res)
{
    // every refusal that depends on the request alone comes before the context is looked at
    if (!opt || !sim || !am || !res) return fail(MCAMD_ERR_INVALID, "opt, sim, am and res must be non-NULL");
    std::memset(res, 0, sizeof *res);
    uint32_t M = 0;
    int n_basis = 0;
    if (int rc = check_american_shape(sim, am, &M, &n_basis)) return rc;
    if (int rc = check_spot_start("American", true, opt, sim)) return rc;
    if (!d_work) return fail(MCAMD_ERR_INVALID, "d_work is NULL");
    const mcamd::AmLayout lay = mcamd::american_layout(am->n_train, sim->n_steps, M, sim->precision);
    if (work_bytes < lay.total)
        return fail(MCAMD_ERR_INVALID, "work_bytes = %llu is below the %llu bytes the workspace needs "
                                       "(mcamd_american_workspace_bytes)",
                    static_cast<unsigned long long>(work_bytes), static_cast<unsigned long long>(lay.total));
    if (int rc = check_common(ctx, opt, sim)) return rc;

    HIP_TRY(hipSetDevice(ctx->device));
    char *base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(d_work) + 255) & ~static_cast<uintptr_t>(255));
    void *traj = base + lay.traj;
    double *V = reinterpret_cast<double *>(base + lay.V);
    double *table = reinterpret_cast<double *>(base + lay.table);
    double *records = table + static_cast<uint64_t>(mcamd::kAmRow) * (M + 1);
    double *w_partials = reinterpret_cast<double *>(base + lay.partials);

    mcamd::AmJob job;
    // the product form: St at every date, the same bits as the stored rows
    job.path = make_plain_job(opt, sim, false, false);
    job.put = am->payoff == MCAMD_PAYOFF_PUT ? 1 : 0;
    job.n_basis = n_basis;
    job.k = am->exercise_every;
    job.M = M;
    job.r = opt->r;
    job.dt = opt->T / static_cast<double>(sim->n_steps);
    job.n_train = am->n_train;
    mcamd::PathJob train = job.path;
    train.seed = am->train_seed;
    train.path_offset = 0;
    train.n_local = am->n_train;

    const uint64_t n_local = sim->n_paths_local;
    const uint32_t store_grid = mcamd::store_grid(am->n_train, sim->precision);
    const uint32_t sweep_grid = mcamd::one_path_per_thread_grid(am->n_train);
    const uint32_t price_grid = mcamd::one_path_per_thread_grid(n_local);
    if (n_local)
        if (int rc = ensure_partials(ctx, price_grid, mcamd::kAmPriceRecord)) return rc;
    // all-ones bits in the record slots and the pinned record until a kernel has written the record: a sum that never
    // finished cannot pass as an earlier call's
    HIP_TRY(hipMemsetAsync(records, 0xFF, 2 * mcamd::kAmRecordSlot * sizeof(double), ctx->stream));
    arm_record(ctx->h_rec, mcamd::kAmPriceRecord);
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    HIP_TRY(mcamd::launch_store(train, MCAMD_STEP_MAJOR, traj, nullptr, nullptr, w_partials, store_grid, ctx->stream));
    HIP_TRY(mcamd::launch_american_sweep(job, traj, V, table, records, w_partials, sweep_grid, ctx->d_ticket,
                                         ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    if (n_local)
        HIP_TRY(mcamd::launch_american_price(job, table, ctx->d_partials, price_grid, ctx->h_rec_dev, ctx->d_ticket,
                                             ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev2, ctx->stream));
    std::vector<double> host(static_cast<size_t>(mcamd::kAmRow) * (M + 1) + 2 * mcamd::kAmRecordSlot);
    HIP_TRY(hipMemcpyAsync(host.data(), table, host.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipEventElapsedTime(&res->train_ms, ctx->ev0, ctx->ev1));
    HIP_TRY(hipEventElapsedTime(&res->price_ms, ctx->ev1, ctx->ev2));
    HIP_TRY(hipEventElapsedTime(&res->total_ms, ctx->ev0, ctx->ev2));

    const double *in_rec = host.data() + static_cast<size_t>(mcamd::kAmRow) * (M + 1);   // launch 0's slot
    if (record_unwritten(in_rec, 2))
        return fail(MCAMD_ERR_HIP, "backward sweep left no in-sample record (its last workgroup did not finish the sum)");
    double rec[mcamd::kAmPriceRecord] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (n_local) {
        std::memcpy(rec, ctx->h_rec, sizeof rec);
        if (record_unwritten(rec, mcamd::kAmPriceRecord))
            return fail(MCAMD_ERR_HIP, "American pricing kernel left no result (its last workgroup did not finish "
                                       "the sum)");
    }
    const Estimate out = estimate(rec[0], rec[1], n_local, 1.0);   // samples are discounted where paid: D = 1
    const Estimate in = estimate(in_rec[0], in_rec[1], am->n_train, 1.0);
    res->price = out.value;
    res->std_err = out.std_err;
    res->sum = rec[0];
    res->sumsq = rec[1];
    res->n = n_local;
    res->n_early = static_cast<uint64_t>(std::llround(rec[2]));
    res->sum_t_exercise = rec[3];
    res->in_sample_price = in.value;
    res->in_sample_std_err = in.std_err;
    res->in_sample_sum = in_rec[0];
    res->in_sample_sumsq = in_rec[1];
    res->n_train = am->n_train;
    const double h0 = std::fmax(job.put ? opt->K - opt->S0 : opt->S0 - opt->K, 0.0);
    bool immediate = floor_at_immediate(h0, &res->in_sample_price, &res->in_sample_std_err);
    if (n_local) immediate = floor_at_immediate(h0, &res->price, &res->std_err) || immediate;
    res->immediate_exercise = immediate ? 1 : 0;
    set_ci(res);
    res->n_dates = M;
    for (uint32_t j = 1; j < M; ++j) res->n_regressed += host[static_cast<size_t>(j) * mcamd::kAmRow + 4] != 0.0 ? 1 : 0;
    if (h_coeffs) {
        for (uint32_t j = 1; j <= M; ++j) {
            const double *row = host.data() + static_cast<size_t>(j) * mcamd::kAmRow;
            double *dst = h_coeffs + static_cast<size_t>(j - 1) * (n_basis + 1);
            for (int q = 0; q < n_basis; ++q) dst[q] = row[4] != 0.0 ? row[q] : std::nan("");
            dst[n_basis] = row[4];
        }
    }
    res->grid = n_local ? price_grid : 0;
    res->block = mcamd::kBlockThreads;
    res->train_grid = sweep_grid;
    return MCAMD_OK;
}

int mcamd_american_dual_workspace_bytes(const mcamd_american *am, const mcamd_sim *sim,
                                        const mcamd_american_dual *dual, uint64_t *bytes)
{
    if (!am || !sim || !dual || !bytes) return fail(MCAMD_ERR_INVALID, "am, sim, dual and bytes must be non-NULL");
    *bytes = 0;
    uint32_t M = 0;
    int n_basis = 0;
    if (int rc = check_dual_shape(sim, am, dual, &M, &n_basis)) return rc;
    *bytes = mcamd::american_dual_layout(sim->n_paths_local, sim->n_steps, M, sim->precision).total;
    return MCAMD_OK;
}

int mcamd_american_upper_bound(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_american *am,
                               const mcamd_american_dual *dual, const double *h_coeffs, void *d_work,
                               uint64_t work_bytes, double *d_cont, mcamd_american_dual_result *res)
{
    // every refusal that depends on the request alone comes before the context is looked at
    if (!opt || !sim || !am || !dual || !res)
        return fail(MCAMD_ERR_INVALID, "opt, sim, am, dual and res must be non-NULL");
    std::memset(res, 0, sizeof *res);
    uint32_t M = 0;
    int n_basis = 0;
    if (int rc = check_dual_shape(sim, am, dual, &M, &n_basis)) return rc;
    if (int rc = check_spot_start("American", true, opt, sim)) return rc;
    if (!h_coeffs) return fail(MCAMD_ERR_INVALID, "h_coeffs is NULL: the rule is what mcamd_price_american wrote");
    for (uint32_t j = 1; j <= M; ++j) {
        const double *row = h_coeffs + static_cast<size_t>(j - 1) * (n_basis + 1);
        if (row[n_basis] != 0.0 && row[n_basis] != 1.0)
            return fail(MCAMD_ERR_INVALID, "h_coeffs: the regressed flag of date %u must be 0 or 1, got %g", j, row[n_basis]);
        if (row[n_basis] == 1.0)
            for (int q = 0; q < n_basis; ++q)
                if (!std::isfinite(row[q]))
                    return fail(MCAMD_ERR_INVALID, "h_coeffs: date %u is flagged regressed but coefficient %d is not "
                                                   "finite", j, q);
    }
    if (!d_work) return fail(MCAMD_ERR_INVALID, "d_work is NULL");
    const uint64_t n_local = sim->n_paths_local;
    const mcamd::AmDualLayout lay = mcamd::american_dual_layout(n_local, sim->n_steps, M, sim->precision);
    if (work_bytes < lay.total)
        return fail(MCAMD_ERR_INVALID, "work_bytes = %llu is below the %llu bytes the workspace needs "
                                       "(mcamd_american_dual_workspace_bytes)",
                    static_cast<unsigned long long>(work_bytes), static_cast<unsigned long long>(lay.total));
    if (int rc = check_common(ctx, opt, sim)) return rc;
    res->n_dates = M;
    res->block = mcamd::kBlockThreads;
    if (n_local == 0) return MCAMD_OK;

    HIP_TRY(hipSetDevice(ctx->device));
    char *base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(d_work) + 255) & ~static_cast<uintptr_t>(255));
    void *traj = base + lay.traj;
    double *Q = d_cont ? d_cont : reinterpret_cast<double *>(base + lay.cont);
    double *table = reinterpret_cast<double *>(base + lay.table);
    double *w_partials = reinterpret_cast<double *>(base + lay.partials);

    mcamd::AmDualJob job;
    // the product form: St at every date, the same bits as the stored rows
    job.path = make_plain_job(opt, sim, false, false);
    job.put = am->payoff == MCAMD_PAYOFF_PUT ? 1 : 0;
    job.n_basis = n_basis;
    job.k = am->exercise_every;
    job.M = M;
    job.n_inner = dual->n_inner;
    job.inner_seed = dual->inner_seed;

    // the device table in the layout (and with the host expressions) of the backward sweep: beta, flag, d_j, t_j
    const double dt = opt->T / static_cast<double>(sim->n_steps);
    std::vector<double> host(static_cast<size_t>(mcamd::kAmRow) * (M + 1), 0.0);
    for (uint32_t j = 0; j <= M; ++j) {
        double *row = host.data() + static_cast<size_t>(j) * mcamd::kAmRow;
        const double *src = j ? h_coeffs + static_cast<size_t>(j - 1) * (n_basis + 1) : nullptr;
        const bool regressed = j >= 1 && j < M && src[n_basis] == 1.0;
        for (int q = 0; q < mcamd::kAmMaxBasis; ++q) row[q] = (regressed && q < n_basis) ? src[q] : std::nan("");
        row[4] = regressed ? 1.0 : 0.0;
        row[6] = static_cast<double>(static_cast<uint64_t>(j) * am->exercise_every) * dt;
        row[5] = std::exp(-opt->r * row[6]);
        row[7] = 0.0;
    }

    const uint32_t store_grid = mcamd::store_grid(n_local, sim->precision);
    const uint32_t cont_grid = mcamd::american_cont_grid(static_cast<uint64_t>(M) * n_local);
    const uint32_t scan_grid = mcamd::one_path_per_thread_grid(n_local);
    constexpr int kRec = mcamd::kAmDualRecord + mcamd::kAmContRecord;
    static_assert(kRec <= mcamd_ctx::kRecord, "the pinned record holds both kernels' records");
    arm_record(ctx->h_rec, kRec);
    HIP_TRY(hipMemcpyAsync(table, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    HIP_TRY(mcamd::launch_store(job.path, MCAMD_STEP_MAJOR, traj, nullptr, nullptr, w_partials, store_grid, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(mcamd::launch_american_cont(job, traj, table, Q, w_partials, cont_grid, ctx->h_rec_dev + mcamd::kAmDualRecord,
                                        ctx->d_ticket, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev2, ctx->stream));
    HIP_TRY(mcamd::launch_american_dual_scan(job, traj, table, Q, w_partials, scan_grid, ctx->h_rec_dev, ctx->d_ticket,
                                             ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev3, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipEventElapsedTime(&res->outer_ms, ctx->ev0, ctx->ev1));
    HIP_TRY(hipEventElapsedTime(&res->inner_ms, ctx->ev1, ctx->ev2));
    HIP_TRY(hipEventElapsedTime(&res->scan_ms, ctx->ev2, ctx->ev3));
    HIP_TRY(hipEventElapsedTime(&res->total_ms, ctx->ev0, ctx->ev3));

    double rec[kRec];
    std::memcpy(rec, ctx->h_rec, sizeof rec);
    if (record_unwritten(rec, kRec))
        return fail(MCAMD_ERR_HIP, "the dual-bound kernels left no result (a last workgroup did not finish its sum)");
    const Estimate up = estimate(rec[0], rec[1], n_local, 1.0);   // samples are discounted where paid: D = 1
    res->upper = up.value;
    res->std_err = up.std_err;
    res->sum = rec[0];
    res->sumsq = rec[1];
    res->sum_q0 = rec[2];
    res->n = n_local;
    res->work_steps = 64.0 * rec[mcamd::kAmDualRecord];   // wave-steps x 64 lanes
    res->live_steps = rec[mcamd::kAmDualRecord + 1];
    const double h0 = std::fmax(job.put ? opt->K - opt->S0 : opt->S0 - opt->K, 0.0);
    res->immediate_exercise = floor_at_immediate(h0, &res->upper, &res->std_err) ? 1 : 0;
    res->ci_hi = res->upper + kZ95 * res->std_err;
    res->grid = cont_grid;
    return MCAMD_OK;
}

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

// Reiner and Rubinstein (1991) / Merton (1973): the continuously monitored single barrier without rebate or dividends,
// from the four terms A..D of the standard presentation (phi = 1 call / -1 put, eta = 1 down / -1 up).
int mcamd_barrier_price_f64(double S0, double K, double B, double T, double r, double v, int kind, int payoff,
                            double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (!(K > 0.0) || !(T > 0.0) || !(v > 0.0) || !std::isfinite(K) || !std::isfinite(T) || !std::isfinite(r) ||
        !std::isfinite(v))
        return fail(MCAMD_ERR_INVALID, "the barrier closed form needs finite K, T, v > 0 and a finite r");
    if (int rc = check_barrier_kind(S0, B, kind, payoff)) return rc;
    const bool up = kind == MCAMD_BARRIER_UP_OUT || kind == MCAMD_BARRIER_UP_IN;
    const bool out = kind == MCAMD_BARRIER_DOWN_OUT || kind == MCAMD_BARRIER_UP_OUT;
    const double phi = payoff == MCAMD_PAYOFF_PUT ? -1.0 : 1.0, eta = up ? -1.0 : 1.0;
    const double s = v * std::sqrt(T), mu = (r - 0.5 * v * v) / (v * v), Kd = K * std::exp(-r * T);
    const auto N = [](double x) { return 0.5 * std::erfc(-x / std::sqrt(2.0)); };
    const double x1 = std::log(S0 / K) / s + (1.0 + mu) * s, x2 = std::log(S0 / B) / s + (1.0 + mu) * s;
    const double y1 = std::log(B * B / (S0 * K)) / s + (1.0 + mu) * s, y2 = std::log(B / S0) / s + (1.0 + mu) * s;
    const double p0 = std::pow(B / S0, 2.0 * mu), p1 = p0 * (B / S0) * (B / S0);
    const double tA = phi * S0 * N(phi * x1) - phi * Kd * N(phi * x1 - phi * s);
    const double tB = phi * S0 * N(phi * x2) - phi * Kd * N(phi * x2 - phi * s);
    const double tC = phi * S0 * p1 * N(eta * y1) - phi * Kd * p0 * N(eta * y1 - eta * s);
    const double tD = phi * S0 * p1 * N(eta * y2) - phi * Kd * p0 * N(eta * y2 - eta * s);
    // the knock-in; the knock-out is the vanilla price (term A) less it.  Which combination depends on whether the
    // strike lies on the live side of the barrier for this payoff.
    const bool call = phi > 0.0;
    double in;
    if (call != up) in = (call ? K >= B : K <= B) ? tC : tA - tB + tD;          // down call, up put
    else in = (call ? K >= B : K <= B) ? tA : tB - tC + tD;                     // up call, down put
    *price = out ? tA - in : in;
    return MCAMD_OK;
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

// Goldman, Sosin and Gatto (1979) for the floating strike, Conze and Viswanathan (1991) for the fixed one: the
// continuously monitored, newly issued lookback without dividends.  A fixed strike on the side of the spot the extremum
// has already passed (call: K <= S0, put: K >= S0) is the opposite floating lookback plus a forward.
int mcamd_lookback_price_f64(double S0, double K, double T, double r, double v, int strike, int payoff, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (!(S0 > 0.0) || !(T > 0.0) || !(v > 0.0) || !std::isfinite(S0) || !std::isfinite(T) || !std::isfinite(r) ||
        !std::isfinite(v))
        return fail(MCAMD_ERR_INVALID, "the lookback closed form needs finite S0, T, v > 0 and a finite r");
    if (r == 0.0)
        return fail(MCAMD_ERR_INVALID, "the lookback closed form carries v^2 / (2r): r == 0 is not covered");
    if (int rc = check_lookback_kind(K, strike, payoff)) return rc;
    const bool put = payoff == MCAMD_PAYOFF_PUT;
    const double sq = std::sqrt(T), s = v * sq, D = std::exp(-r * T), G = std::exp(r * T);
    const double lam = v * v / (2.0 * r), shift = 2.0 * r * sq / v;
    const auto N = [](double x) { return 0.5 * std::erfc(-x / std::sqrt(2.0)); };
    const double a = (r + 0.5 * v * v) * T / s;
    const auto floating = [&](bool is_put) {
        if (is_put) return S0 * D * N(-a + s) - S0 * N(-a) + S0 * D * lam * (-N(a - shift) + G * N(a));
        return S0 * N(a) - S0 * D * N(a - s) + S0 * D * lam * (N(-a + shift) - G * N(-a));
    };
    if (strike == MCAMD_LOOKBACK_FLOATING) {
        *price = floating(put);
        return MCAMD_OK;
    }
    const double d = (std::log(S0 / K) + (r + 0.5 * v * v) * T) / s;
    const double pw = std::pow(S0 / K, -2.0 * r / (v * v));
    if (!put) {
        if (K > S0) *price = S0 * N(d) - K * D * N(d - s) + S0 * D * lam * (-pw * N(d - shift) + G * N(d));
        else *price = floating(true) + S0 - K * D;
    } else {
        if (K < S0) *price = K * D * N(-d + s) - S0 * N(-d) + S0 * D * lam * (pw * N(-d + shift) - G * N(-d));
        else *price = floating(false) + K * D - S0;
    }
    return MCAMD_OK;
}

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

// The geometric basket is a lognormal: ln A_T ~ N(m, s^2), m = sum_j w_j (ln S0_j + (r - v_j^2/2) T),
// s^2 = T w'(v o corr o v) w.
int mcamd_basket_geometric_price_f64(const mcamd_basket *basket, double K, double T, double r, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (!basket) return fail(MCAMD_ERR_INVALID, "basket is NULL");
    double L[64];
    if (int rc = check_basket_assets(basket, false, L)) return rc;
    if (!std::isfinite(K) || !(K >= 0.0)) return fail(MCAMD_ERR_INVALID, "a basket option needs a finite K >= 0, got %g", K);
    if (!(T > 0.0) || !std::isfinite(T) || !std::isfinite(r))
        return fail(MCAMD_ERR_INVALID, "the geometric closed form needs a finite T > 0 and a finite r");
    const int d = basket->n_assets;
    double mean = 0.0, var = 0.0;
    for (int j = 0; j < d; ++j) {
        mean += basket->w[j] * (std::log(basket->S0[j]) + (r - 0.5 * basket->v[j] * basket->v[j]) * T);
        for (int k = 0; k < d; ++k)
            var += basket->w[j] * basket->v[j] * basket->corr[8 * j + k] * basket->v[k] * basket->w[k];
    }
    var *= T;
    const double s = std::sqrt(var > 0.0 ? var : 0.0), D = std::exp(-r * T), F = std::exp(mean + 0.5 * var);
    const bool put = basket->payoff == MCAMD_PAYOFF_PUT;
    const auto N = [](double x) { return 0.5 * std::erfc(-x / std::sqrt(2.0)); };
    if (K == 0.0 || !(s > 0.0)) {   // a forward: A_T > 0 = K always, or A_T is not random (weights that cancel)
        const double fwd = K == 0.0 ? F : std::exp(mean);
        *price = D * std::fmax(put ? K - fwd : fwd - K, 0.0);
        return MCAMD_OK;
    }
    const double d1 = (mean - std::log(K)) / s + s, d2 = d1 - s;
    *price = put ? D * (K * N(-d2) - F * N(-d1)) : D * (F * N(d1) - K * N(d2));
    return MCAMD_OK;
}

// Margrabe (1978): the option to exchange b S2 for a S1.
int mcamd_exchange_price_f64(double a_S1, double b_S2, double T, double v1, double v2, double rho, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (!(a_S1 > 0.0) || !(b_S2 > 0.0) || !(T > 0.0) || !(v1 > 0.0) || !(v2 > 0.0) || !std::isfinite(a_S1) ||
        !std::isfinite(b_S2) || !std::isfinite(T) || !std::isfinite(v1) || !std::isfinite(v2))
        return fail(MCAMD_ERR_INVALID, "the exchange closed form needs finite a S1, b S2, T, v1, v2 > 0");
    if (!(rho > -1.0 && rho < 1.0))
        return fail(MCAMD_ERR_INVALID, "the exchange closed form needs -1 < rho < 1, got %g", rho);
    const double s = std::sqrt((v1 * v1 + v2 * v2 - 2.0 * rho * v1 * v2) * T);
    const auto N = [](double x) { return 0.5 * std::erfc(-x / std::sqrt(2.0)); };
    const double d1 = std::log(a_S1 / b_S2) / s + 0.5 * s;
    *price = a_S1 * N(d1) - b_S2 * N(d1 - s);
    return MCAMD_OK;
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

int mcamd_asian_geometric_price_f64(double S0, double K, double T, double r, double v, uint32_t n_steps,
                                    int include_spot, int strike, int payoff, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    return asian_geometric_price(S0, K, T, r, v, n_steps, include_spot, strike, payoff, price);
}

int mcamd_price_autocall(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_autocall *autocall,
                         void *d_samples, mcamd_autocall_result *res)
{
    if (!res) return fail(MCAMD_ERR_INVALID, "opt, sim, autocall and res must be non-NULL");
    std::memset(res, 0, sizeof *res);
    return prepare_autocall(ctx, opt, sim, autocall, d_samples, [&](const auto &call) {
        return run_sync(ctx, call, res, [&](const double *rec) {
            // {sum, sumsq, paths called, sum of their call times, paths not called and knocked in, wave-steps, live}
            const Estimate e = estimate(rec[0], rec[1], sim->n_paths_local, std::exp(-opt->r * opt->T));
            res->sum = rec[0];
            res->sumsq = rec[1];
            res->n = sim->n_paths_local;
            res->price = e.value;
            res->std_err = e.std_err;
            set_ci(res);
            res->n_called = static_cast<uint64_t>(std::llround(rec[2]));
            res->sum_t_call = rec[3];
            res->n_knocked_in = static_cast<uint64_t>(std::llround(rec[4]));
            res->work_steps = 64.0 * rec[5];   // wave-steps x 64 lanes
            res->live_steps = rec[6];
        });
    });
}

int mcamd_price_autocall_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                 const mcamd_autocall *autocall, void *d_samples, double *d_stats)
{
    return prepare_autocall(ctx, opt, sim, autocall, d_samples,
                            [&](const auto &call) { return run_enqueue(ctx, call, d_stats); });
}

// One asset, one date: S_T / S_0 is lognormal, P[S_T / S_0 >= x] = N(d2(x)) and E[(S_T / S_0) 1{S_T / S_0 <= x}] =
// e^{rT} N(-d1(x)).  Called above L: 1 + c; between B and L: 1; at or below B: the performance itself (B <= 1).
int mcamd_autocall_single_date_price_f64(double T, double r, double v, double call_level, double coupon,
                                         double ki_level, int ki_monitoring, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (!(T > 0.0) || !(v > 0.0) || !std::isfinite(T) || !std::isfinite(r) || !std::isfinite(v))
        return fail(MCAMD_ERR_INVALID, "the single-date autocall closed form needs finite T, v > 0 and a finite r");
    if (int rc = check_autocall_terms(coupon, call_level, 0.0, call_level, ki_monitoring, ki_level)) return rc;
    if (ki_monitoring == MCAMD_AUTOCALL_KI_EVERY_STEP)
        return fail(MCAMD_ERR_INVALID, "the closed form covers MCAMD_AUTOCALL_KI_NONE and MCAMD_AUTOCALL_KI_AT_MATURITY: "
                                       "a knock-in monitored at every step has none");
    const auto N = [](double x) { return 0.5 * std::erfc(-x / std::sqrt(2.0)); };
    const double s = v * std::sqrt(T);
    const auto d2 = [&](double x) { return (-std::log(x) + (r - 0.5 * v * v) * T) / s; };
    const double pL = N(d2(call_level));
    double value = (1.0 + coupon) * pL;
    if (ki_monitoring == MCAMD_AUTOCALL_KI_NONE) value += 1.0 - pL;
    else value += (N(d2(ki_level)) - pL) + std::exp(r * T) * N(-(d2(ki_level) + s));
    *price = std::exp(-r * T) * value;
    return MCAMD_OK;
}

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
            const Estimate e = estimate(rec[0], rec[1], sim->n_paths_local, std::exp(-opt->r * opt->T));
            res->sum = rec[0];
            res->sumsq = rec[1];
            res->n = sim->n_paths_local;
            res->price = e.value;
            res->std_err = e.std_err;
            set_ci(res);
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

// Volatility in time only: the period log-returns D_p ~ N((r - q - v_p^2 / 2) tau, v_p^2 tau) are independent, so the
// mean of a sum of clipped returns is the sum of the means and that of their product the product.  A return clipped to
// [F, C] is (1 + F) + (e^D - (1 + F))+ - (e^D - (1 + C))+ gross: two calls on e^D.
int mcamd_cliquet_price_f64(int kind, double T, double r, double q, uint32_t n_periods, uint32_t first_period,
                            const double *period_vol, double local_floor, double local_cap, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (!period_vol) return fail(MCAMD_ERR_INVALID, "period_vol is NULL");
    if (int rc = check_cliquet_kind(kind)) return rc;
    if (int rc = check_cliquet_local(local_floor, local_cap)) return rc;
    if (int rc = check_cliquet_kind_bounds(kind, local_floor, local_cap)) return rc;
    if (!(T > 0.0) || !std::isfinite(T) || !std::isfinite(r) || !std::isfinite(q))
        return fail(MCAMD_ERR_INVALID, "the cliquet closed form needs a finite T > 0 and finite r and q");
    if (n_periods == 0 || first_period < 1 || first_period > n_periods)
        return fail(MCAMD_ERR_INVALID, "n_periods must be >= 1 and first_period 1..n_periods, got %u and %u", n_periods,
                    first_period);
    for (uint32_t p = 0; p < n_periods; ++p)
        if (!std::isfinite(period_vol[p]) || !(period_vol[p] > 0.0))
            return fail(MCAMD_ERR_INVALID, "every period volatility must be finite and > 0: period_vol[%u] = %g", p,
                        period_vol[p]);
    const auto N = [](double x) { return 0.5 * std::erfc(-x / std::sqrt(2.0)); };
    const double tau = T / static_cast<double>(n_periods), fwd = std::exp((r - q) * tau);
    const double F = std::fmax(local_floor, -1.0);   // a floor at or below -1 never binds
    double sum = 0.0, prod = 1.0;
    for (uint32_t p = first_period; p <= n_periods; ++p) {
        const double v = period_vol[p - 1], s = v * std::sqrt(tau);
        const auto call = [&](double k) {   // E[(e^D - k)+]
            if (k <= 0.0) return fwd - k;
            if (k == HUGE_VAL) return 0.0;
            const double d1 = ((r - q + 0.5 * v * v) * tau - std::log(k)) / s;
            return fwd * N(d1) - k * N(d1 - s);
        };
        if (kind == MCAMD_CLIQUET_VARIANCE) {
            const double mean = (r - q - 0.5 * v * v) * tau;
            sum += v * v * tau + mean * mean;
        } else {
            const double E = (1.0 + F) + call(1.0 + F) - call(1.0 + local_cap);
            sum += E - 1.0;
            prod *= E;
        }
    }
    const double P = static_cast<double>(n_periods - first_period + 1);
    const double value = kind == MCAMD_CLIQUET_SUM ? sum : kind == MCAMD_CLIQUET_COMPOUND ? prod - 1.0 : sum / (P * tau);
    *price = std::exp(-r * T) * value;
    return MCAMD_OK;
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

// fills *res from an autocall kernel's record: {sum, sumsq, paths called, sum of their call times, paths not called and
// knocked in, wave-steps, live}
static void fill_autocall_result(const double *rec, uint64_t n, double r, double T, mcamd_autocall_result *res)
{
    const Estimate e = estimate(rec[0], rec[1], n, std::exp(-r * T));
    res->sum = rec[0];
    res->sumsq = rec[1];
    res->n = n;
    res->price = e.value;
    res->std_err = e.std_err;
    set_ci(res);
    res->n_called = static_cast<uint64_t>(std::llround(rec[2]));
    res->sum_t_call = rec[3];
    res->n_knocked_in = static_cast<uint64_t>(std::llround(rec[4]));
    res->work_steps = 64.0 * rec[5];   // wave-steps x 64 lanes
    res->live_steps = rec[6];
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

// The smile's two launches on the context's stream: the walk into the per-wavefront records, then their sum into out.
static int launch_smile_pair(mcamd_ctx *ctx, const mcamd::SmileJob &job, uint32_t grid, double *out, double n_value,
                             hipEvent_t before, hipEvent_t after)
{
    HIP_TRY(hipEventRecord(before, ctx->stream));
    HIP_TRY(mcamd::launch_localvol_smile(job, ctx->d_partials, grid, ctx->stream));
    HIP_TRY(hipEventRecord(after, ctx->stream));
    HIP_TRY(mcamd::launch_smile_finish(ctx->d_partials, grid * mcamd::kSmileWavesPerBlock, job.n_expiries * job.n_strikes,
                                       out, n_value, ctx->stream));
    return MCAMD_OK;
}

int mcamd_price_localvol_smile(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_smile *smile,
                               const uint32_t *h_expiry_steps, const double *h_strikes,
                               const mcamd_localvol_surface *surface, void *d_spots, double *h_stats, mcamd_result *res)
{
    if (!res || !h_stats) return fail(MCAMD_ERR_INVALID, "h_stats and res must be non-NULL");
    zero_result(res);
    return prepare_smile(ctx, opt, sim, smile, h_expiry_steps, h_strikes, surface, d_spots,
                         [&](const mcamd::SmileJob &job, uint32_t grid) -> int {
        const uint32_t nodes = job.n_expiries * job.n_strikes, n_stats = 2 * nodes;
        std::fill(h_stats, h_stats + n_stats, 0.0);
        if (job.n_local == 0) return MCAMD_OK;
        HIP_TRY(hipSetDevice(ctx->device));
        if (!ctx->h_smile) {
            HIP_TRY(hipHostMalloc(&ctx->h_smile, mcamd_ctx::kSmileStats * sizeof(double), hipHostMallocDefault));
            HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&ctx->h_smile_dev), ctx->h_smile, 0));
        }
        if (int rc = ensure_partials(ctx, grid * mcamd::kSmileWavesPerBlock, static_cast<int>(n_stats))) return rc;
        // the finishing kernel writes the pinned buffer itself; all-ones bits there afterwards mean it never ran
        arm_record(ctx->h_smile, static_cast<int>(n_stats));
        if (int rc = launch_smile_pair(ctx, job, grid, ctx->h_smile_dev, -1.0, ctx->ev0, ctx->ev1)) return rc;
        HIP_TRY(hipEventRecord(ctx->ev2, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        float kernel_ms = 0.0f, total_ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&kernel_ms, ctx->ev0, ctx->ev1));
        HIP_TRY(hipEventElapsedTime(&total_ms, ctx->ev0, ctx->ev2));
        if (record_unwritten(ctx->h_smile, static_cast<int>(n_stats)))
            return fail(MCAMD_ERR_HIP, "the smile kernels left no result (the finishing kernel did not write every node)");
        std::memcpy(h_stats, ctx->h_smile, n_stats * sizeof(double));
        const uint32_t last = job.expiry_steps[job.n_expiries - 1];
        finalize_into(h_stats[nodes - 1], h_stats[n_stats - 1], job.n_local, opt->r,
                      static_cast<double>(last) * job.dt, res);
        res->work_steps = 64.0 * static_cast<double>((job.n_local + 63) / 64) * static_cast<double>(last);
        res->live_steps = res->work_steps;
        res->kernel_ms = kernel_ms;
        res->total_ms = total_ms;
        res->grid = grid;
        res->block = mcamd::kBlockThreads;
        return MCAMD_OK;
    });
}

int mcamd_price_localvol_smile_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                       const mcamd_smile *smile, const uint32_t *h_expiry_steps, const double *h_strikes,
                                       const mcamd_localvol_surface *surface, void *d_spots, double *d_stats)
{
    if (!d_stats) return fail(MCAMD_ERR_INVALID, "d_stats is NULL");
    return prepare_smile(ctx, opt, sim, smile, h_expiry_steps, h_strikes, surface, d_spots,
                         [&](const mcamd::SmileJob &job, uint32_t grid) -> int {
        const uint32_t n_stats = 2 * job.n_expiries * job.n_strikes;
        HIP_TRY(hipSetDevice(ctx->device));
        const uint32_t slot = static_cast<uint32_t>(ctx->n_enqueued % mcamd_ctx::kRing);
        if (job.n_local == 0) {
            HIP_TRY(hipMemsetAsync(d_stats, 0, (n_stats + 1) * sizeof(double), ctx->stream));
            HIP_TRY(hipEventRecord(ctx->ring0[slot], ctx->stream));
            HIP_TRY(hipEventRecord(ctx->ring1[slot], ctx->stream));
            ctx->n_enqueued++;
            return MCAMD_OK;
        }
        const uint32_t waves = grid * mcamd::kSmileWavesPerBlock;
        // growing the scratch buffer frees the old one: wait for work that may still read it
        if (static_cast<uint64_t>(waves) * n_stats > ctx->partial_capacity) HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (int rc = ensure_partials(ctx, waves, static_cast<int>(n_stats))) return rc;
        if (int rc = launch_smile_pair(ctx, job, grid, d_stats, static_cast<double>(job.n_local), ctx->ring0[slot],
                                       ctx->ring1[slot]))
            return rc;
        ctx->n_enqueued++;
        return MCAMD_OK;
    });
}

int mcamd_finalize_smile(const double *stats, uint64_t n, const mcamd_option *opt, uint32_t n_steps,
                         const mcamd_smile *smile, const uint32_t *h_expiry_steps, double *h_price, double *h_std_err)
{
    if (!stats || !opt || !smile || !h_expiry_steps || !h_price || !h_std_err)
        return fail(MCAMD_ERR_INVALID, "stats, opt, smile, h_expiry_steps, h_price and h_std_err must be non-NULL");
    if (smile->n_expiries < 1 || smile->n_expiries > MCAMD_SMILE_MAX_EXPIRIES || smile->n_strikes < 1 ||
        smile->n_strikes > MCAMD_SMILE_MAX_STRIKES)
        return fail(MCAMD_ERR_INVALID, "n_expiries must lie in 1 .. %d and n_strikes in 1 .. %d", MCAMD_SMILE_MAX_EXPIRIES,
                    MCAMD_SMILE_MAX_STRIKES);
    if (n_steps == 0 || !(opt->T > 0.0) || !std::isfinite(opt->T) || !std::isfinite(opt->r))
        return fail(MCAMD_ERR_INVALID, "a smile needs n_steps >= 1 and finite r and T > 0");
    finalize_smile_into(stats, n, opt->r, opt->T, n_steps, smile->n_expiries, smile->n_strikes, h_expiry_steps, h_price,
                        h_std_err);
    return MCAMD_OK;
}

int mcamd_localvol_sigma_f64(const mcamd_localvol_grid *grid, const double *h_sigma, uint32_t n_steps, uint32_t step,
                             double x, double *sigma)
{
    if (!sigma) return fail(MCAMD_ERR_INVALID, "sigma is NULL");
    *sigma = 0.0;
    if (int rc = check_localvol_grid(grid, h_sigma, nullptr)) return rc;
    if (n_steps == 0 || step >= n_steps)
        return fail(MCAMD_ERR_INVALID, "step = %u must lie in [0, n_steps = %u)", step, n_steps);
    if (std::isnan(x)) return fail(MCAMD_ERR_INVALID, "x is NaN");
    const uint64_t row = static_cast<uint64_t>(step) * grid->n_t / n_steps;
    const double dx = (grid->x_max - grid->x_min) / static_cast<double>(grid->n_x - 1);
    const double u = std::fmin(std::fmax((x - grid->x_min) * (1.0 / dx), 0.0), static_cast<double>(grid->n_x - 1));
    const uint32_t k = std::min(static_cast<uint32_t>(u), grid->n_x - 2);
    const double *s = h_sigma + row * grid->n_x + k;
    *sigma = std::fma(u - static_cast<double>(k), s[1] - s[0], s[0]);
    return MCAMD_OK;
}

int mcamd_bs_price_f64(double S0, double K, double T, double r, double q, double v, int payoff, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (!(S0 > 0.0) || !(K > 0.0) || !(T > 0.0) || !(v > 0.0) || !std::isfinite(S0) || !std::isfinite(K) ||
        !std::isfinite(T) || !std::isfinite(v) || !std::isfinite(r) || !std::isfinite(q))
        return fail(MCAMD_ERR_INVALID, "Black-Scholes needs finite S0, K, T, v > 0 and finite r, q");
    if (payoff != MCAMD_PAYOFF_CALL && payoff != MCAMD_PAYOFF_PUT)
        return fail(MCAMD_ERR_INVALID, "payoff must be MCAMD_PAYOFF_CALL (0) or MCAMD_PAYOFF_PUT (1), got %d", payoff);
    const double sqrtT = std::sqrt(T);
    const double d1 = (std::log(S0 / K) + (r - q + 0.5 * v * v) * T) / (v * sqrtT), d2 = d1 - v * sqrtT;
    const auto N = [](double x) { return 0.5 * std::erfc(-x / std::sqrt(2.0)); };
    const double Sd = S0 * std::exp(-q * T), Kd = K * std::exp(-r * T);
    *price = payoff == MCAMD_PAYOFF_CALL ? Sd * N(d1) - Kd * N(d2) : Kd * N(-d2) - Sd * N(-d1);
    return MCAMD_OK;
}

int mcamd_bs_implied_vol_f64(double S0, double K, double T, double r, double q, int payoff, double price, double *vol)
{
    if (!vol) return fail(MCAMD_ERR_INVALID, "vol is NULL");
    *vol = std::nan("");
    if (!(S0 > 0.0) || !(K > 0.0) || !(T > 0.0) || !std::isfinite(S0) || !std::isfinite(K) || !std::isfinite(T) ||
        !std::isfinite(r) || !std::isfinite(q) || !std::isfinite(price))
        return fail(MCAMD_ERR_INVALID, "an implied volatility needs finite S0, K, T > 0 and finite r, q and price");
    if (payoff != MCAMD_PAYOFF_CALL && payoff != MCAMD_PAYOFF_PUT)
        return fail(MCAMD_ERR_INVALID, "payoff must be MCAMD_PAYOFF_CALL (0) or MCAMD_PAYOFF_PUT (1), got %d", payoff);
    const bool call = payoff == MCAMD_PAYOFF_CALL;
    const double D = std::exp(-r * T), F = S0 * std::exp((r - q) * T);
    const double lower = D * std::fmax(call ? F - K : K - F, 0.0);
    const double upper = call ? S0 * std::exp(-q * T) : K * D;
    if (!(price > lower) || !(price < upper))
        return fail(MCAMD_ERR_INVALID, "the price %.17g is not strictly inside the no-arbitrage bounds (%.17g, %.17g)", price,
                    lower, upper);
    // The price grows with v from lower to upper: bracket the root, then Newton steps kept inside the bracket and
    // replaced by a bisection whenever they leave it or shrink it too slowly (plain Newton diverges in the wings,
    // where the vega vanishes).  f is "not above" at lo and "above or equal" at hi throughout; a NaN counts as not above.
    double lo = 0.0, hi = 1.0 / std::sqrt(T);
    for (int grow = 0; grow < 64 && !(bs_value(S0, K, T, r, q, hi, call, nullptr) >= price); ++grow) {
        lo = hi;
        hi *= 2.0;
    }
    double x = 0.5 * (lo + hi), dx_old = hi - lo, dx = dx_old, vega = 0.0;
    double f = bs_value(S0, K, T, r, q, x, call, &vega) - price;
    for (int it = 0; it < 400; ++it) {
        const bool newton_leaves = !(((x - hi) * vega - f) * ((x - lo) * vega - f) < 0.0);
        const bool newton_slow = !(std::fabs(2.0 * f) <= std::fabs(dx_old * vega));
        dx_old = dx;
        if (newton_leaves || newton_slow) {
            dx = 0.5 * (hi - lo);
            x = lo + dx;
        } else {
            dx = f / vega;
            x -= dx;
        }
        if (!(std::fabs(dx) > 1e-15 * x)) break;
        f = bs_value(S0, K, T, r, q, x, call, &vega) - price;
        if (f >= 0.0) hi = x;
        else lo = x;
        if (f == 0.0) break;
    }
    *vol = x;
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

// Closed form, host.  Same operation order and the same mixed precision as the reference:
// `0.5 * v * v` and `exp(-r * T)` are evaluated in double and narrowed (inc/BlackandScholes.hpp:37,42).
float mcamd_cnd_f32(float x)
{
    const float p = 0.2316419f;
    const float b1 = 0.31938153f, b2 = -0.356563782f, b3 = 1.781477937f, b4 = -1.821255978f, b5 = 1.330274429f;
    const float one_over_sqrt_twopi = 0.39894228f;
    const float t = 1.0f / (1.0f + p * std::fabs(x));
    const float tail = one_over_sqrt_twopi * expf(-x * x / 2.0f) * t * (t * (t * (t * (t * b5 + b4) + b3) + b2) + b1);
    return x >= 0.0f ? 1.0f - tail : tail;
}

float mcamd_bs_call_f32(float x0, float strike, float T, float r, float sigma)
{
    const float sqrtT = sqrtf(T);
    const float d1 = static_cast<float>(
        (static_cast<double>(logf(x0 / strike)) + (static_cast<double>(r) + 0.5 * sigma * sigma) * T) /
        static_cast<double>(sigma * sqrtT));
    const float d2 = d1 - sigma * sqrtT;
    const float n1 = mcamd_cnd_f32(d1), n2 = mcamd_cnd_f32(d2);
    return static_cast<float>(static_cast<double>(x0 * n1) -
                              static_cast<double>(strike) * std::exp(static_cast<double>(-r * T)) * n2);
}

double mcamd_bs_call_f64(double x0, double strike, double T, double r, double sigma)
{
    const double sqrtT = std::sqrt(T);
    const double d1 = (std::log(x0 / strike) + (r + 0.5 * sigma * sigma) * T) / (sigma * sqrtT);
    const double d2 = d1 - sigma * sqrtT;
    return x0 * 0.5 * std::erfc(-d1 / std::sqrt(2.0)) - strike * std::exp(-r * T) * 0.5 * std::erfc(-d2 / std::sqrt(2.0));
}

}  // extern "C"
