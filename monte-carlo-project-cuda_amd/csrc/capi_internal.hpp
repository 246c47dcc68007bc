// capi_internal.hpp — what more than one translation unit of the C ABI (capi.cpp, capi_*.cpp, closed_forms.cpp,
// group.cpp) needs: the error helpers, the context, the two call drivers, the host statistics and the checks that a
// call shares with another family or with its closed form.  Non-template functions are defined once, in the file of
// the family that owns them (named beside each group); everything here is hidden from the library's dynamic symbols.
// closed_forms.cpp defines MCAMD_CAPI_HOST_ONLY before including this header and so sees no HIP declaration.
#pragma once

#include "mcamd.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#ifndef MCAMD_CAPI_HOST_ONLY
#include "enqueue_intervals.hpp"
#include "launch.hpp"
#endif

// capi.cpp: records the calling thread's last error message (for callers that have the text already)
int mcamd_set_error_(int code, const char *msg);

namespace mcamd {
struct AutocallSchedule;   // autocall.hpp
struct BarrierForm;        // barrier.hpp
struct SmileNodes;         // smile.hpp
}

#pragma GCC visibility push(hidden)

namespace mcamd::capi {

// ---- capi.cpp: errors and the refusals every family shares -------------------------------------------------------

// records the formatted message as the calling thread's last error and returns code
int fail(int code, const char *fmt, ...);

int check_payoff(int payoff);                      // MCAMD_PAYOFF_CALL or MCAMD_PAYOFF_PUT
int check_precision_steps(const mcamd_sim *sim);   // the path precision, then n_steps >= 1

// the cumulative standard normal distribution of every double-precision closed form
inline double norm_cdf(double x)
{
    return 0.5 * std::erfc(-x / std::sqrt(2.0));
}

// the step of the products that start at the spot (check_spot_start refuses an opt->dt of their own) ...
inline double even_dt(const mcamd_option *opt, const mcamd_sim *sim)
{
    return opt->T / static_cast<double>(sim->n_steps);
}

// ... and of the calls that take one: opt->dt if positive
inline double step_dt(const mcamd_option *opt, const mcamd_sim *sim)
{
    return opt->dt > 0.0 ? opt->dt : opt->T / static_cast<double>(sim->n_steps);
}

// a barrier kind (MCAMD_BARRIER_*) as the side the barrier lies on and what touching it does
struct BarrierSides {
    bool up, out;
};
inline BarrierSides barrier_sides(int kind)
{
    return {kind == MCAMD_BARRIER_UP_OUT || kind == MCAMD_BARRIER_UP_IN,
            kind == MCAMD_BARRIER_DOWN_OUT || kind == MCAMD_BARRIER_UP_OUT};
}

// ---- the checks a call shares with another family or with its closed form ------------------------------------------

// capi_pathdep.cpp
int check_monitoring(int monitoring);   // MCAMD_MONITOR_DISCRETE or MCAMD_MONITOR_CONTINUOUS
int check_barrier_kind(double S0, double B, int kind, int payoff);
// what the barrier calls of every model refuse of the barrier: monitoring, reserved, then check_barrier_kind
int check_barrier_terms(const mcamd_barrier *bar, double S0, double B);
// a job's form from enums that passed these checks; MCAMD_LOCALVOL_NO_BARRIER: neither up, out nor continuous
mcamd::BarrierForm barrier_form(int kind, int monitoring, int payoff);
int check_lookback_kind(double K, int strike, int payoff);
int check_asian_kind(double K, int strike, int payoff, int include_spot);
// capi_multi.cpp
int check_basket_assets(const mcamd_basket *b, bool positive_weights, double L[64]);
int check_autocall_terms(double coupon, double call_level, double call_step_down, double L_last, int ki_monitoring,
                         double ki_level);
// ... and what mcamd_price_autocall and mcamd_price_autocall_localvol share, whose structs differ in v / q alone.
// The assets of a note through check_basket_assets (performances: spot 1 and weight 1), with the volatilities v or,
// with v NULL, ones:
int check_autocall_assets(int n_assets, const double *v, const double corr[64], double L[64]);
// the fields the two structs have in common
struct AutocallTerms {
    uint32_t observe_every, first_call_date;
    int ki_monitoring;
    double call_level, call_step_down, coupon, ki_level;
};
template <typename Autocall>
AutocallTerms autocall_terms(const Autocall *ac)
{
    return {ac->observe_every, ac->first_call_date, ac->ki_monitoring, ac->call_level, ac->call_step_down, ac->coupon,
            ac->ki_level};
}
// the refusals from "observe_every must be >= 1" through check_autocall_terms; *M = n_steps / observe_every
int check_autocall_schedule(const AutocallTerms &t, uint32_t n_steps, uint32_t *M);
// the M dates' levels and payments (maturity money at rate r) and the knock-in, for steps of dt
void make_autocall_schedule(const AutocallTerms &t, uint32_t M, double r, double T, double dt,
                            mcamd::AutocallSchedule *schedule);
// capi_localvol.cpp
int check_localvol_grid(const mcamd_localvol_grid *grid, const double *h_sigma, double *sigma_max);
int check_cliquet_kind(int kind);
int check_cliquet_local(double local_floor, double local_cap);
int check_cliquet_kind_bounds(int kind, double local_floor, double local_cap);
int check_cliquet_job(const mcamd_cliquet *cq, uint32_t n_steps);
// capi_smile.cpp: what every smile call refuses of the nodes, in this order: n_expiries and n_strikes out of range,
// expiry steps that are not strictly ascending in 1 .. n_steps, a strike that is not finite and > 0.  Nodes that pass
// are left in *nodes, as a job carries them, with the payoff (checked by the caller) that holds for all of them.
int check_smile_nodes(uint32_t n_expiries, uint32_t n_strikes, const uint32_t *h_expiry_steps, uint32_t n_steps,
                      const double *h_strikes, int payoff, mcamd::SmileNodes *nodes);
// capi_heston.cpp
int check_heston_model(double q, double v0, double kappa, double theta, double xi, double rho);
// closed_forms.cpp
int asian_geometric_price(double S0, double K, double T, double r, double v, uint32_t n_steps, int include_spot,
                          int strike, int payoff, double *price);
double bs_value(double S0, double K, double T, double r, double q, double v, bool call, double *vega);

}  // namespace mcamd::capi

#pragma GCC visibility pop

#ifndef MCAMD_CAPI_HOST_ONLY

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            (void)hipGetLastError();                                                                   \
            return fail(e_ == hipErrorOutOfMemory ? MCAMD_ERR_NOMEM : MCAMD_ERR_HIP, "%s: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                             \
        }                                                                                              \
    } while (0)

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
    // Overlapped enqueues: the simulation kernels of consecutive large mcamd_price_paths_enqueue jobs run
    // on two internal non-blocking streams in turn, each into a scratch buffer of its own, and only the final
    // reduction runs on `stream`.  The streams and events are created by the first such job.
    static_assert(kRing == mcamd::capi::kEnqueueRing, "the interval arithmetic walks this ring");
    bool overlap = false;         // MCAMD_ENQUEUE_OVERLAP as mcamd_ctx_create found it; cleared for good by a failure
    bool overlap_ready = false;   // the two streams and events exist
    hipStream_t lane_stream[2] = {};
    hipEvent_t lane_reduced[2] = {};   // on `stream`, after the reduction that last read the lane's buffer
    bool lane_read[2] = {};            // lane_reduced has been recorded
    double *lane_partials[2] = {};
    uint64_t lane_capacity[2] = {};    // in doubles
    uint64_t n_overlapped = 0;         // the next overlapped job takes lane n_overlapped % 2
    mcamd::capi::OverlapSlot ring_overlap[kRing];
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

#pragma GCC visibility push(hidden)

namespace mcamd::capi {

// ---- capi.cpp: scratch, request checks and jobs ----------------------------------------------------------------------

int ensure_partials(mcamd_ctx *ctx, uint32_t records, int record_doubles = 2);

// what every path call refuses on the request alone (opt and sim non-NULL)
int check_request(const mcamd_option *opt, const mcamd_sim *sim);
int check_common(const mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim);
// check_common plus the refusals of the calls that run plain paths (no variance reduction) and, but for
// mcamd_price_from_normals, take a trajectory layout
int check_plain(const mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int layout = MCAMD_STEP_MAJOR);
// What a plain product that starts at the spot ("American", "barrier", "lookback" options) refuses of the option and
// the flags.  american: the rules of the two American calls, which read only use_window of the window fields, price
// off S0 and K as well, and take the product form; the others allow MCAMD_FLAG_LOG_SPACE alone.
int check_spot_start(const char *name, bool american, const mcamd_option *opt, const mcamd_sim *sim);
// What a call whose volatility is not the option's (the local-volatility calls, Heston; name: how the messages call
// the product) refuses of the option, the flags and sim through the two checks above.  seen: the caller's copy of the
// option with every field it does not read made harmless; it carries no volatility of its own, so check_spot_start
// sees v = 1 and check_request v = 0, which leaves each drift mu[j] = r - q_j alone in the fp64 exponent-range bound.
int check_drift_request(const char *name, mcamd_option seen, const mcamd_sim *sim, const double *mu, int n_mu);

PathJob make_job(const mcamd_option *opt, const mcamd_sim *sim);
// The job of a call that runs plain paths whatever the flags say: no variance reduction, the given window and form.
PathJob make_plain_job(const mcamd_option *opt, const mcamd_sim *sim, bool window, bool logspace);
// the shard's paths as the local-volatility and Heston jobs carry them
inline PathRange path_range(const mcamd_sim *sim)
{
    return {sim->seed, sim->path_offset, sim->n_paths_local, sim->n_steps, sim->precision};
}

void zero_result(mcamd_result *res);

// ---- one device call as both drivers see it --------------------------------------------------------------------------

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
    hipError_t operator()(const FinishSpec &) const { return hipSuccess; }
};
inline DeviceCall<NoLaunch> empty_call(int stats = 6)
{
    return {0, 0, 2, stats, Finish::kReduce, {}};
}

// A self-finishing kernel's final record is filled with all-ones bits before the launch.  No finished sum has that
// pattern (a NaN the arithmetic makes is the canonical one), so finding it after the sync means the kernel's last
// workgroup never wrote the record, e.g. because the arrival ticket was not zero at launch.  Bits, not isnan: an fp32
// job that saturates can sum to a genuine NaN, and that is a result.
void arm_record(double *rec, int n);
bool record_unwritten(const double *rec, int n);

// ---- capi.cpp: the host statistics -------------------------------------------------------------------------------------

constexpr double kZ95 = 1.959963984540054;   // two-sided 95 % quantile of the standard normal

// disc x the mean of n samples and its standard error, from their sum and sum of squares
struct Estimate {
    double value, std_err;
};
Estimate estimate(double sum, double sumsq, uint64_t n, double disc);

template <typename Result>   // mcamd_result, mcamd_american_result and every result struct finalize_into fills
void set_ci(Result *res)
{
    res->ci_lo = res->price - kZ95 * res->std_err;
    res->ci_hi = res->price + kZ95 * res->std_err;
}

// the seven fields every price result starts with: sum, sumsq, n, price, std_err and the interval
template <typename Result>   // mcamd_result, mcamd_autocall_result, mcamd_cliquet_result, mcamd_heston*_result
void finalize_into(double sum, double sumsq, uint64_t n, double r, double T, Result *res)
{
    const Estimate e = estimate(sum, sumsq, n, std::exp(-r * T));
    res->sum = sum;
    res->sumsq = sumsq;
    res->n = n;
    res->price = e.value;
    res->std_err = e.std_err;
    set_ci(res);
}
// the lane-steps of a walk without an early exit: every wavefront that holds a path runs every step
inline double full_walk_work_steps(uint64_t n, uint32_t n_steps)
{
    return 64.0 * static_cast<double>((n + 63) / 64) * static_cast<double>(n_steps);
}
void finalize_cv_into(const double s[5], uint64_t n, double r, double T, mcamd_result *res);
// a price record with the work counters behind it: {sum, sumsq, wave-steps, live lane-steps}
void finalize_counted_into(const double rec[4], uint64_t n, double r, double T, mcamd_result *res);
// price / SE / CI of a pricing record: {sum, sumsq} or, with the control variate, the five sums
void finalize_record(const double *rec, bool control_variate, uint64_t n, double r, double T, mcamd_result *res);
// a nested-MC record over n points: the mean point price is the scalar diagnostic of the wrappers
void finalize_nmc_into(const double rec[kNmcRecord], uint64_t n, mcamd_result *res);
void finalize_greeks_into(const double stats[16], double r, double T, int theta_defined, mcamd_greeks *out);
// capi_localvol.cpp: value / std_err / sums of a (possibly all-reduced) 32-double local-volatility Greeks record
void finalize_localvol_greeks_into(const double stats[32], double r, double T, uint32_t n_buckets, int gamma_defined,
                                   mcamd_localvol_greeks *out);
// capi_multi.cpp: fills *res from an autocall kernel's record: {sum, sumsq, paths called, sum of their call times,
// paths not called and knocked in, wave-steps, live}
void fill_autocall_result(const double *rec, uint64_t n, double r, double T, mcamd_autocall_result *res);

// ---- the two drivers -------------------------------------------------------------------------------------------------

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
    FinishSpec fs;
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
            HIP_TRY(launch_small_final(ctx->d_partials, call.grid, call.rec, ctx->d_out, ctx->stream));
        else
            HIP_TRY(launch_final_reduce(ctx->d_partials, call.grid, call.rec, ctx->d_out, ctx->stream));
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
    res->block = kBlockThreads;
    return MCAMD_OK;
}

// capi.cpp: what every enqueue form (run_enqueue and run_smile_enqueue) does to the ring and the scratch buffer, after
// hipSetDevice.  The slot of the call being enqueued is n_enqueued % kRing; a call counts once its kernels are enqueued.
// The empty shard: n all-zero doubles in d_stats, ordered on the stream, between both events of the slot; counted.
int enqueue_empty_shard(mcamd_ctx *ctx, double *d_stats, uint32_t n);
// ensure_partials under an enqueue: growing the scratch buffer frees the old one, so the stream is waited for first
int ensure_partials_enqueued(mcamd_ctx *ctx, uint32_t records, int record_doubles);

// Asynchronous driver: the kernel runs between a pair of ring events, and its record reaches d_stats in the statistics
// layout with n_value = n, from the kernel itself (kFolded) or from the separate sum.  Nothing waits on the host but the
// growth of the scratch buffer.  An empty shard leaves all-zero statistics, still ordered on the stream.
//
// A kReduce call whose launch can also be aimed at another buffer and stream, launch(fs, d_partials, stream), and whose
// kernel touches neither the ticket nor the queue (mcamd_price_paths_enqueue's large jobs) is overlapped where the
// context allows it: overlap_begin picks the lane, or none for the in-order path below, and readies it up
// to the start event; the kernel runs on the lane's stream into the lane's buffer; overlap_finish records the end
// event there and enqueues the reduction into d_stats on ctx->stream behind it.
int overlap_begin(mcamd_ctx *ctx, uint32_t records, int record_doubles, int *lane);
int overlap_finish(mcamd_ctx *ctx, int lane, uint32_t records, int record_doubles, double *d_stats, double n_value);
// a failure on an internal stream: the context takes the in-order path from now on; returns rc
int overlap_failed(mcamd_ctx *ctx, int rc);

template <typename Launch>
int run_enqueue(mcamd_ctx *ctx, const DeviceCall<Launch> &call, double *d_stats)
{
    if (!d_stats) return fail(MCAMD_ERR_INVALID, "d_stats is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    if (call.n == 0) return enqueue_empty_shard(ctx, d_stats, static_cast<uint32_t>(call.stats));
    const uint32_t slot = static_cast<uint32_t>(ctx->n_enqueued % mcamd_ctx::kRing);
    const double n_value = static_cast<double>(call.n);
    if constexpr (std::is_invocable_v<const Launch &, const FinishSpec &, double *, hipStream_t>) {
        if (call.how == Finish::kReduce && ctx->overlap) {
            int lane = -1;
            if (int rc = overlap_begin(ctx, call.grid, call.rec, &lane)) return rc;
            if (lane >= 0) {
                const hipError_t e = call.launch(FinishSpec{}, ctx->lane_partials[lane], ctx->lane_stream[lane]);
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    return overlap_failed(ctx, fail(MCAMD_ERR_HIP, "simulation kernel on an internal stream: %s",
                                                    hipGetErrorString(e)));
                }
                return overlap_finish(ctx, lane, call.grid, call.rec, d_stats, n_value);
            }
        }
    }
    if (int rc = ensure_partials_enqueued(ctx, call.grid, call.rec)) return rc;
    FinishSpec fs;
    if (call.how == Finish::kFolded) {
        fs.out = d_stats;
        fs.ticket = ctx->d_ticket;
        fs.n_value = n_value;
    }
    HIP_TRY(hipEventRecord(ctx->ring0[slot], ctx->stream));
    HIP_TRY(call.launch(fs));
    HIP_TRY(hipEventRecord(ctx->ring1[slot], ctx->stream));
    if (call.how == Finish::kSmall)
        HIP_TRY(launch_small_final(ctx->d_partials, call.grid, call.rec, d_stats, ctx->stream, n_value));
    else if (call.how == Finish::kReduce)
        HIP_TRY(launch_final_reduce(ctx->d_partials, call.grid, call.rec, d_stats, ctx->stream, n_value));
    ctx->n_enqueued++;
    return MCAMD_OK;
}

// ---- capi_smile.cpp: the smile layer, whatever model walks the paths ----------------------------------------------------

// One smile call (mcamd_price_localvol_smile, mcamd_price_heston_smile) as its two drivers see it.  They are not
// run_sync / run_enqueue: a smile is two kernels, its per-wavefront records are not the reported grid of sums, and a
// record holds up to 4096 doubles where DeviceCall's fit the 32 of h_rec.  launch(job, d_partials, grid, stream) enqueues
// the model's walk, which leaves grid x kSmileWavesPerBlock records; launch_smile_finish sums them for every model.
using SmileLaunch = hipError_t (*)(const void *job, double *d_partials, uint32_t grid, hipStream_t stream);
struct SmileCall {
    uint64_t n;          // paths of the shard; 0: empty shard, nothing runs
    uint32_t grid;       // workgroups of the walk (smile_grid)
    uint32_t n_expiries, n_strikes;
    double r, t_last;    // what the last node is finalized with: the rate, and the time of the last expiry
    uint32_t last_step;  // the step of the last expiry: every wavefront that holds a path runs that many
    SmileLaunch launch;
    const void *job;
};
// a model's launcher of its own job type as a SmileLaunch
template <typename Job, hipError_t (*Launch)(const Job &, double *, uint32_t, hipStream_t)>
hipError_t smile_launch(const void *job, double *d_partials, uint32_t grid, hipStream_t stream)
{
    return Launch(*static_cast<const Job *>(job), d_partials, grid, stream);
}
// The call of a shard of sim->n_paths_local paths that stop at `nodes`, with steps of dt at the rate r: the grid is
// smile_grid's, and an empty shard has n == 0 and grid == 0.  `job` must outlive the call.
SmileCall make_smile_call(const mcamd_ctx *ctx, const mcamd_sim *sim, const mcamd::SmileNodes &nodes, double r, double dt,
                          SmileLaunch launch, const void *job);
// Synchronous: h_stats receives the 2 n_e n_K sums (zeros for an empty shard, which launches nothing) through the
// context's pinned smile record, and *res (zeroed by the caller) the last node, the work and the timings: the walk runs
// between ev0 and ev1, the sum of the records up to ev2.
int run_smile_sync(mcamd_ctx *ctx, const SmileCall &call, double *h_stats, mcamd_result *res);
// Asynchronous: the walk runs between the ring events of the call's slot and the sum leaves the 2 n_e n_K sums and then n
// in d_stats; an empty shard leaves 2 n_e n_K + 1 zeros, still ordered on the stream.
int run_smile_enqueue(mcamd_ctx *ctx, const SmileCall &call, double *d_stats);

}  // namespace mcamd::capi

#pragma GCC visibility pop

#endif  // MCAMD_CAPI_HOST_ONLY
