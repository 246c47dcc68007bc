// capi_american.cpp — the American calls of the C ABI: the least-squares price (mcamd_price_american) and its dual
// upper bound (mcamd_american_upper_bound), each several kernels on a caller's workspace, driven by hand.
#include "capi_internal.hpp"
#include "american.hpp"
#include "american_dual.hpp"

#include <vector>

static_assert(sizeof(mcamd_american) == 32 && sizeof(mcamd_american_result) == 152,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");
static_assert(sizeof(mcamd_american_dual) == 16 && sizeof(mcamd_american_dual_result) == 104,
              "C ABI struct layout changed: bump MCAMD_ABI_VERSION");

using namespace mcamd::capi;

namespace {

// h(S0) replaces an estimate it exceeds (exercise at t = 0); returns whether it did
bool floor_at_immediate(double h0, double *price, double *std_err)
{
    if (!(h0 > *price)) return false;
    *price = h0;
    *std_err = 0.0;
    return true;
}

// The refusals of the American calls that depend on the request's shape alone (shared with the workspace-size query):
// dates and basis size on success.
int check_american_shape(const mcamd_sim *sim, const mcamd_american *am, uint32_t *M, int *n_basis)
{
    if (int rc = check_payoff(am->payoff)) return rc;
    if (am->n_basis != 0 && (am->n_basis < 2 || am->n_basis > static_cast<uint32_t>(mcamd::kAmMaxBasis)))
        return fail(MCAMD_ERR_INVALID, "n_basis must be 2, 3 or 4 (0 = 3), got %u", am->n_basis);
    if (am->reserved != 0) return fail(MCAMD_ERR_INVALID, "am->reserved must be 0, got %u", am->reserved);
    if (int rc = check_precision_steps(sim)) return rc;   // before check_request can: the dates divide n_steps
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

// the workspace layouts (american_layout, american_dual_layout) count from the first 256-byte boundary of d_work
char *workspace_base(void *d_work)
{
    return reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(d_work) + 255) & ~static_cast<uintptr_t>(255));
}

}  // namespace

extern "C" {

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
    char *base = workspace_base(d_work);
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
    job.dt = even_dt(opt, sim);
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
    char *base = workspace_base(d_work);
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
    const double dt = even_dt(opt, sim);
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

}  // extern "C"
