// capi_smile.cpp — the smile layer of the C ABI, with no model in it: what every smile call refuses of its nodes, the
// nodes as a job carries them, the call as the two smile drivers see it, the drivers, and the host statistics of a
// smile's sums.  A model's own file (capi_localvol.cpp, capi_heston.cpp) keeps its prepare_* step and its entry points.
#include "capi_internal.hpp"
#include "smile.hpp"

#include <algorithm>

static_assert(sizeof(mcamd_smile) == 24, "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(MCAMD_SMILE_MAX_STRIKES == mcamd::kSmileMaxStrikes && MCAMD_SMILE_MAX_EXPIRIES == mcamd::kSmileMaxExpiries,
              "the smile kernel takes one strike per lane and MCAMD_SMILE_MAX_EXPIRIES expiry steps");

using namespace mcamd::capi;

namespace mcamd::capi {

int check_smile_nodes(uint32_t n_expiries, uint32_t n_strikes, const uint32_t *h_expiry_steps, uint32_t n_steps,
                      const double *h_strikes, int payoff, mcamd::SmileNodes *nodes)
{
    if (n_expiries < 1 || n_expiries > MCAMD_SMILE_MAX_EXPIRIES)
        return fail(MCAMD_ERR_INVALID, "n_expiries must lie in 1 .. %d, got %u", MCAMD_SMILE_MAX_EXPIRIES, n_expiries);
    if (n_strikes < 1 || n_strikes > MCAMD_SMILE_MAX_STRIKES)
        return fail(MCAMD_ERR_INVALID, "n_strikes must lie in 1 .. %d, got %u", MCAMD_SMILE_MAX_STRIKES, n_strikes);
    for (uint32_t m = 0; m < n_expiries; ++m) {
        const uint32_t before = m ? h_expiry_steps[m - 1] : 0;
        if (h_expiry_steps[m] <= before || h_expiry_steps[m] > n_steps)
            return fail(MCAMD_ERR_INVALID, "expiry steps must be strictly ascending in 1 .. n_steps = %u: "
                                           "h_expiry_steps[%u] = %u", n_steps, m, h_expiry_steps[m]);
    }
    for (uint32_t k = 0; k < n_strikes; ++k)
        if (!std::isfinite(h_strikes[k]) || !(h_strikes[k] > 0.0))
            return fail(MCAMD_ERR_INVALID, "every strike must be finite and > 0: h_strikes[%u] = %g", k, h_strikes[k]);
    *nodes = {payoff == MCAMD_PAYOFF_PUT, n_expiries, n_strikes, {}, {}};
    std::copy(h_expiry_steps, h_expiry_steps + n_expiries, nodes->expiry_steps);
    std::copy(h_strikes, h_strikes + n_strikes, nodes->strikes);
    return MCAMD_OK;
}

SmileCall make_smile_call(const mcamd_ctx *ctx, const mcamd_sim *sim, const mcamd::SmileNodes &nodes, double r, double dt,
                          SmileLaunch launch, const void *job)
{
    const uint64_t n = sim->n_paths_local;
    const uint32_t last = nodes.expiry_steps[nodes.n_expiries - 1];
    const uint32_t grid = n ? mcamd::smile_grid(n, nodes.n_expiries, nodes.n_strikes, ctx->compute_units) : 0;
    return {n, grid, nodes.n_expiries, nodes.n_strikes, r, static_cast<double>(last) * dt, last, launch, job};
}

namespace {

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

// A smile's two launches on the context's stream: the walk into the per-wavefront records, then their sum into out.
int launch_smile_pair(mcamd_ctx *ctx, const SmileCall &call, double *out, double n_value, hipEvent_t before,
                      hipEvent_t after)
{
    HIP_TRY(hipEventRecord(before, ctx->stream));
    HIP_TRY(call.launch(call.job, ctx->d_partials, call.grid, ctx->stream));
    HIP_TRY(hipEventRecord(after, ctx->stream));
    HIP_TRY(mcamd::launch_smile_finish(ctx->d_partials, call.grid * mcamd::kSmileWavesPerBlock,
                                       call.n_expiries * call.n_strikes, out, n_value, ctx->stream));
    return MCAMD_OK;
}

}  // namespace

int run_smile_sync(mcamd_ctx *ctx, const SmileCall &call, double *h_stats, mcamd_result *res)
{
    const uint32_t nodes = call.n_expiries * call.n_strikes, n_stats = 2 * nodes;
    std::fill(h_stats, h_stats + n_stats, 0.0);
    if (call.n == 0) return MCAMD_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->h_smile) {
        HIP_TRY(hipHostMalloc(&ctx->h_smile, mcamd_ctx::kSmileStats * sizeof(double), hipHostMallocDefault));
        HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&ctx->h_smile_dev), ctx->h_smile, 0));
    }
    if (int rc = ensure_partials(ctx, call.grid * mcamd::kSmileWavesPerBlock, static_cast<int>(n_stats))) return rc;
    // the finishing kernel writes the pinned buffer itself; all-ones bits there afterwards mean it never ran
    arm_record(ctx->h_smile, static_cast<int>(n_stats));
    if (int rc = launch_smile_pair(ctx, call, ctx->h_smile_dev, -1.0, ctx->ev0, ctx->ev1)) return rc;
    HIP_TRY(hipEventRecord(ctx->ev2, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    float kernel_ms = 0.0f, total_ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&kernel_ms, ctx->ev0, ctx->ev1));
    HIP_TRY(hipEventElapsedTime(&total_ms, ctx->ev0, ctx->ev2));
    if (record_unwritten(ctx->h_smile, static_cast<int>(n_stats)))
        return fail(MCAMD_ERR_HIP, "the smile kernels left no result (the finishing kernel did not write every node)");
    std::memcpy(h_stats, ctx->h_smile, n_stats * sizeof(double));
    finalize_into(h_stats[nodes - 1], h_stats[n_stats - 1], call.n, call.r, call.t_last, res);
    res->work_steps = full_walk_work_steps(call.n, call.last_step);
    res->live_steps = res->work_steps;
    res->kernel_ms = kernel_ms;
    res->total_ms = total_ms;
    res->grid = call.grid;
    res->block = mcamd::kBlockThreads;
    return MCAMD_OK;
}

int run_smile_enqueue(mcamd_ctx *ctx, const SmileCall &call, double *d_stats)
{
    const uint32_t n_stats = 2 * call.n_expiries * call.n_strikes;
    HIP_TRY(hipSetDevice(ctx->device));
    if (call.n == 0) return enqueue_empty_shard(ctx, d_stats, n_stats + 1);
    const uint32_t slot = static_cast<uint32_t>(ctx->n_enqueued % mcamd_ctx::kRing);
    if (int rc = ensure_partials_enqueued(ctx, call.grid * mcamd::kSmileWavesPerBlock, static_cast<int>(n_stats))) return rc;
    if (int rc = launch_smile_pair(ctx, call, d_stats, static_cast<double>(call.n), ctx->ring0[slot], ctx->ring1[slot]))
        return rc;
    ctx->n_enqueued++;
    return MCAMD_OK;
}

}  // namespace mcamd::capi

extern "C" {

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

}  // extern "C"
