// american.hip — least-squares Monte Carlo (Longstaff and Schwartz, 2001) for gfx950, both path precisions: the
// backward sweep over the stored training trajectories and the out-of-sample pricing pass.
//
// Notation of include/mcamd.h: dates j = 1..M at steps s_j = j k, S_j the price after step s_j (stored row s_j - 1),
// h the exercise value, u = S / K - 1, phi = (1, u, .., u^(m-1)), d_j = exp(-r t_j).  Regression arithmetic is fp64 on
// (double) S whatever the path precision.
//
// Sweep, launch j (j = M-1 .. 0), one pass over the n_train training paths (path_frame.hpp's ThreadPaths):
//   1. every workgroup reads the record launch j+1 finished and solves date j+1's 2..4-unknown normal equations —
//      uniform and redundant, so every workgroup holds identical bits; workgroup 0 writes the table row of date j+1;
//   2. each path applies date j+1's decision to V (launch M-1 sets V = d_M h(S_M) instead);
//   3. each path adds to date j's record: the power sums P_0..P_6 of u, sum V u^q (q < 4) and |I_j| over the paths in
//      the money at date j (launch 0: sum V and sum V^2, the in-sample estimate).  finish_paths sums the
//      record in a fixed order and the last workgroup writes it to the workspace: no host round trip between dates.
// Pricing: one path per thread, the product-form loop of the store kernel (same Philox blocks, same PathState), the
// price evaluated at exercise dates only; a wavefront leaves the step loop once every lane's path has stopped.
//
// Both passes decide through am_exercise, so a path whose stored row and in-register price are the same bits (the
// same path: train_seed == seed) is exercised at the same date by both.
#include "american.hpp"
#include "american_device.hpp"
#include "path_consts.hpp"
#include "path_frame.hpp"

#include <algorithm>

namespace mcamd {

template <typename T>
struct AmSweepArgs {
    const T *traj;           // step-major rows of n training paths
    double *V;
    double *table;
    const double *rec_in;    // the record of date j+1 (unused by launch M-1)
    uint64_t n;
    uint64_t row_next;       // stored row of date j+1
    uint64_t row_j;          // stored row of date j (j >= 1)
    double K;
    double disc_next, t_next;   // d_{j+1}, t_{j+1} (host-computed)
    uint32_t j, M;
    int put;
    GridFinish fin;          // fin.out: the record slot of date j
};

template <typename T, int MB>
__global__ __launch_bounds__(kBlock) void am_sweep_kernel(AmSweepArgs<T> a, double *__restrict__ partials)
{
    const bool put = a.put != 0;
    const bool first = a.j + 1 == a.M;
    double beta[MB];
#pragma unroll
    for (int q = 0; q < MB; ++q) beta[q] = 0.0;
    const bool regressed = first ? false : am_solve<MB>(a.rec_in, beta);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double *row = a.table + static_cast<uint64_t>(a.j + 1) * kAmRow;
#pragma unroll
        for (int q = 0; q < kAmMaxBasis; ++q) row[q] = (regressed && q < MB) ? beta[q < MB ? q : 0] : __builtin_nan("");
        row[4] = regressed ? 1.0 : 0.0;
        row[5] = a.disc_next;
        row[6] = a.t_next;
        row[7] = 0.0;
    }
    double acc[kAmRecord];
#pragma unroll
    for (int q = 0; q < kAmRecord; ++q) acc[q] = 0.0;
    const T *__restrict__ next = a.traj + a.row_next * a.n;
    const T *__restrict__ cur = a.traj + a.row_j * a.n;
    for (const uint64_t i : ThreadPaths{a.n}) {
        const double Sn = static_cast<double>(next[i]);
        double v;
        if (first) {
            v = a.disc_next * am_payoff(put, a.K, Sn);
        } else {
            v = a.V[i];
            double y;
            if (regressed && am_exercise<MB>(beta, a.disc_next, a.K, put, Sn, y)) v = y;
        }
        if (a.j > 0) {
            const double S = static_cast<double>(cur[i]);
            if (am_payoff(put, a.K, S) > 0.0) {
                const double u = S / a.K - 1.0;
                double p = 1.0;
#pragma unroll
                for (int q = 0; q < 7; ++q) {
                    acc[q] += p;
                    if (q < kAmMaxBasis) acc[7 + q] = __builtin_fma(v, p, acc[7 + q]);
                    p *= u;
                }
                acc[11] += 1.0;
            }
            a.V[i] = v;
        } else {
            add_sample(acc, v);
        }
    }
    finish_paths(acc, partials, a.fin);
}

template <typename T>
struct AmPriceArgs {
    StepConsts<T> c;
    const double *table;
    PathShard shard;
    double K;
    uint32_t k, M;
    int put;
    GridFinish fin;
};

template <typename T, int MB>
__global__ __launch_bounds__(kBlock) void am_price_kernel(AmPriceArgs<T> a, double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    const StepConsts<T> c = resident(a.c);
    const bool put = a.put != 0;
    const StepBlocks blocks = step_blocks<NB>(c.n_sim);
    double acc[kAmPriceRecord];
#pragma unroll
    for (int q = 0; q < kAmPriceRecord; ++q) acc[q] = 0.0;
    for (const uint64_t i : ThreadPaths{a.shard.n_local}) {
        const uint64_t subsequence = a.shard.path_offset + i;
        PathState<T> ps = PathState<T>::start(c.S_start);
        bool live = true;
        double y = 0.0;
        uint32_t ex_date = 0;            // date of an exercise before maturity, 0: none
        uint32_t date = 0, until = a.k;  // the same for every lane of the wavefront
        auto step = [&](T x) {
            ps.step(x, m);
            if (--until != 0) return;
            until = a.k;
            ++date;
            const double *row = a.table + static_cast<uint64_t>(date) * kAmRow;
            if (date == a.M) {
                if (live) y = row[5] * am_payoff(put, a.K, static_cast<double>(ps.value(m)));
                live = false;
            } else if (row[4] != 0.0) {
                double beta[MB];
#pragma unroll
                for (int q = 0; q < MB; ++q) beta[q] = row[q];
                double ye;
                if (live && am_exercise<MB>(beta, row[5], a.K, put, static_cast<double>(ps.value(m)), ye)) {
                    y = ye;
                    live = false;
                    ex_date = date;
                }
            }
        };
        Exponents<T> ex;
        walk_steps<NB>(
            blocks, [&](uint32_t b) { ex.fill(m, c, key, subsequence, b); }, [&](uint32_t, int j) { step(ex.x[j]); },
            [&] { return __builtin_amdgcn_ballot_w64(live) == 0; });   // every lane's path has stopped
        add_sample(acc, y);
        if (ex_date != 0) {
            acc[2] += 1.0;
            acc[3] += a.table[static_cast<uint64_t>(ex_date) * kAmRow + 6];
        }
        acc[4] += 1.0;
    }
    finish_paths(acc, partials, a.fin);
}

static uint64_t align256(uint64_t x) { return (x + 255) & ~static_cast<uint64_t>(255); }

AmLayout american_layout(uint64_t n_train, uint32_t n_steps, uint32_t M, int precision)
{
    const uint64_t elem = precision == 32 ? 4 : 8;
    const uint64_t partials = std::max<uint64_t>(2ull * store_grid(n_train, precision),
                                                 static_cast<uint64_t>(kAmRecord) * one_path_per_thread_grid(n_train));
    AmLayout l;
    l.traj = 0;
    l.V = l.traj + align256(static_cast<uint64_t>(n_steps) * n_train * elem);
    l.table = l.V + align256(8 * n_train);
    l.partials = l.table + align256(8 * (static_cast<uint64_t>(kAmRow) * (M + 1) + 2 * kAmRecordSlot));
    l.total = 256 + l.partials + align256(8 * partials);
    return l;
}

template <typename T, int MB>
static hipError_t sweep_t(const AmJob &job, const void *traj, double *V, double *table, double *records,
                          double *partials, uint32_t grid, unsigned int *ticket, hipStream_t stream)
{
    AmSweepArgs<T> a;
    a.traj = static_cast<const T *>(traj);
    a.V = V;
    a.table = table;
    a.n = job.n_train;
    a.K = job.path.K;
    a.M = job.M;
    a.put = job.put;
    const dim3 g(grid), b(kBlock);
    for (uint32_t j = job.M; j-- > 0;) {
        const uint32_t jn = j + 1;
        const uint64_t s_next = static_cast<uint64_t>(jn) * job.k;
        a.j = j;
        a.rec_in = records + ((jn & 1) ? kAmRecordSlot : 0);
        a.row_next = s_next - 1;
        a.row_j = j > 0 ? static_cast<uint64_t>(j) * job.k - 1 : 0;
        a.t_next = static_cast<double>(s_next) * job.dt;
        a.disc_next = std::exp(-job.r * a.t_next);
        a.fin = GridFinish{records + ((j & 1) ? kAmRecordSlot : 0), ticket, -1.0};
        hipLaunchKernelGGL((am_sweep_kernel<T, MB>), g, b, 0, stream, a, partials);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename T, int MB>
static hipError_t price_t(const AmJob &job, const double *table, double *d_partials, uint32_t grid, double *out,
                          unsigned int *ticket, hipStream_t stream)
{
    AmPriceArgs<T> a;
    a.c = make_consts<T>(job.path);
    a.table = table;
    a.shard = shard_of(job.path);
    a.K = job.path.K;
    a.k = job.k;
    a.M = job.M;
    a.put = job.put;
    a.fin = GridFinish{out, ticket, -1.0};
    hipLaunchKernelGGL((am_price_kernel<T, MB>), dim3(grid), dim3(kBlock), 0, stream, a, d_partials);
    return hipGetLastError();
}

#define MCAMD_AM_DISPATCH(FN, ...)                                                                       \
    switch (job.n_basis) {                                                                            \
    case 2: return job.path.precision == 32 ? FN<float, 2>(__VA_ARGS__) : FN<double, 2>(__VA_ARGS__); \
    case 3: return job.path.precision == 32 ? FN<float, 3>(__VA_ARGS__) : FN<double, 3>(__VA_ARGS__); \
    case 4: return job.path.precision == 32 ? FN<float, 4>(__VA_ARGS__) : FN<double, 4>(__VA_ARGS__); \
    default: return hipErrorInvalidValue;                                                             \
    }

hipError_t launch_american_sweep(const AmJob &job, const void *traj, double *V, double *table, double *records,
                                 double *partials, uint32_t grid, unsigned int *ticket, hipStream_t stream)
{
    if (!ticket || grid > kFoldMaxRecords || job.M == 0 || job.M > kAmMaxDates) return hipErrorInvalidValue;
    MCAMD_AM_DISPATCH(sweep_t, job, traj, V, table, records, partials, grid, ticket, stream)
}

hipError_t launch_american_price(const AmJob &job, const double *table, double *d_partials, uint32_t grid, double *out,
                                 unsigned int *ticket, hipStream_t stream)
{
    if (!out || !ticket || grid > kFoldMaxRecords) return hipErrorInvalidValue;
    MCAMD_AM_DISPATCH(price_t, job, table, d_partials, grid, out, ticket, stream)
}

#undef MCAMD_AM_DISPATCH

}  // namespace mcamd
