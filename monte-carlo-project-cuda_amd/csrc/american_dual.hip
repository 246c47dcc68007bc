// american_dual.hip — the Andersen-Broadie (2004) dual bound of a fitted exercise rule for gfx950, both path
// precisions: the nested continuation kernel and the per-path martingale scan.
//
// Notation of include/mcamd.h (mcamd_american_upper_bound): dates j = 0..M at steps s_j = j k, S_{p,j} the outer path p
// after step s_j (stored row s_j - 1; S_{p,0} = S0), Z_{p,j} = d_j h(S_{p,j}), e_{p,j} the rule's decision (am_exercise
// on a regressed date; e_{p,M} = 1), Q_{p,j} the value of following the rule from (p, j) on.
//
// Continuation, one workgroup per point (p, j), j < M: the workgroup's threads stride over the point's n_inner paths
// with the step loop of am_price_kernel started at date j — same PathState, same Exponents, same decision function —
// on Philox subsequence ((path_offset + p) M + j) n_inner + i from block 0.  A wavefront leaves the loop once each of
// its paths has stopped.  block_sumN adds the samples in the order the thread layout fixes, so Q is the same bits in
// every run and under any sharding.
// Scan, one outer path per thread: pi_0 = 0, pi_j = pi_{j-1} + L_j - Q_{j-1} with L_j = Z_j where e_j, else Q_j; the dual
// sample is u = max_j (Z_j - pi_j).  Where e_j holds, Z_j - pi_j is Q_{j-1} - pi_{j-1} and is formed that way: one
// rounding fewer, and with one date u is Q_0 itself.
#include "american_dual.hpp"
#include "american_device.hpp"
#include "path_consts.hpp"
#include "path_frame.hpp"

#include <algorithm>

namespace mcamd {

template <typename T>
struct AmContArgs {
    StepConsts<T> c;         // of the outer job: S_start = S0, n_sim = n_steps
    const T *traj;           // step-major rows of the shard's n_local outer paths
    const double *table;
    double *Q;
    PathShard shard;         // the outer paths, with the inner seed
    uint64_t n_points;       // M n_local
    double K;
    uint32_t k, M, n_inner;
    int put;
    GridFinish fin;
};

template <typename T, int MB>
__global__ __launch_bounds__(kBlock) void am_cont_kernel(AmContArgs<T> a, double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    const StepConsts<T> c = resident(a.c);
    const bool put = a.put != 0;
    const bool first_lane = (threadIdx.x & (kWave - 1)) == 0;
    double rec[kAmContRecord] = {0.0, 0.0};   // thread 0: this workgroup's wave-steps and live lane-steps
    for (uint64_t task = blockIdx.x; task < a.n_points; task += gridDim.x) {
        const uint32_t j0 = static_cast<uint32_t>(task / a.shard.n_local);   // date-major: a workgroup's tasks span the dates
        const uint64_t p = task - static_cast<uint64_t>(j0) * a.shard.n_local;
        const T S_in = j0 == 0 ? c.S_start : a.traj[(static_cast<uint64_t>(j0) * a.k - 1) * a.shard.n_local + p];
        const uint64_t sub0 = ((a.shard.path_offset + p) * a.M + j0) * a.n_inner;
        const uint32_t n_sim = (a.M - j0) * a.k;
        const uint32_t n_full = n_sim / NB;
        const uint32_t rem = n_sim - n_full * NB;
        double acc = 0.0;
        uint64_t work = 0, lane_live = 0;
        for (uint64_t i = threadIdx.x; i < a.n_inner; i += kBlock) {
            const uint64_t subsequence = sub0 + i;
            PathState<T> ps = PathState<T>::start(S_in);
            bool live = true;
            double y = 0.0;
            uint32_t stop = a.M;               // date the path stops at
            uint32_t date = j0, until = a.k;   // the same for every lane of the wavefront
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
                        stop = date;
                    }
                }
            };
            uint32_t steps_run = n_sim;
            bool running = true;
            for (uint32_t b = 0; b < n_full; ++b) {
                Exponents<T> ex;
                ex.fill(m, c, key, subsequence, b);
#pragma unroll
                for (int s = 0; s < NB; ++s) step(ex.x[s]);
                if (__builtin_amdgcn_ballot_w64(live) == 0) {   // every lane's path has stopped
                    steps_run = (b + 1) * NB;
                    running = false;
                    break;
                }
            }
            if (rem && running) {
                Exponents<T> ex;
                ex.fill(m, c, key, subsequence, n_full);
#pragma unroll
                for (int s = 0; s < NB - 1; ++s)
                    if (static_cast<uint32_t>(s) < rem) step(ex.x[s]);
            }
            acc += y;
            lane_live += static_cast<uint64_t>(stop - j0) * a.k;   // steps this path was live for
            work += steps_run;                                     // steps its wavefront ran (counted by the first lane)
        }
        double pt[3] = {acc, first_lane ? static_cast<double>(work) : 0.0, static_cast<double>(lane_live)};
        block_sumN<kBlock, 3>(pt);
        if (threadIdx.x == 0) {
            a.Q[task] = pt[0] / static_cast<double>(a.n_inner);
            rec[0] += pt[1];
            rec[1] += pt[2];
        }
        __syncthreads();   // block_sumN's LDS slots are reused by the next task
    }
    grid_finish<kBlock, kAmContRecord>(rec, partials, a.fin);
}

template <typename T>
struct AmScanArgs {
    const T *traj;
    const double *table;
    const double *Q;
    uint64_t n_local;
    double K;
    uint32_t k, M;
    int put;
    GridFinish fin;
};

template <typename T, int MB>
__global__ __launch_bounds__(kBlock) void am_dual_scan_kernel(AmScanArgs<T> a, double *__restrict__ partials)
{
    const bool put = a.put != 0;
    double acc[kAmDualRecord];
#pragma unroll
    for (int q = 0; q < kAmDualRecord; ++q) acc[q] = 0.0;
    for (const uint64_t p : ThreadPaths{a.n_local}) {
        const double q0 = a.Q[p];
        double q_prev = q0, pi = 0.0, u = -__builtin_inf();
        for (uint32_t j = 1; j <= a.M; ++j) {
            const double *row = a.table + static_cast<uint64_t>(j) * kAmRow;
            const double S = static_cast<double>(a.traj[(static_cast<uint64_t>(j) * a.k - 1) * a.n_local + p]);
            const double Z = row[5] * am_payoff(put, a.K, S);
            bool e = j == a.M;
            double q_j = 0.0;
            if (!e) {
                q_j = a.Q[static_cast<uint64_t>(j) * a.n_local + p];
                if (row[4] != 0.0) {
                    double beta[MB];
#pragma unroll
                    for (int q = 0; q < MB; ++q) beta[q] = row[q];
                    double ye;
                    e = am_exercise<MB>(beta, row[5], a.K, put, S, ye);
                }
            }
            double cand;
            if (e) {
                cand = q_prev - pi;        // = Z_j - pi_j
                pi += Z - q_prev;
            } else {
                pi += q_j - q_prev;
                cand = Z - pi;
            }
            u = cand > u ? cand : u;
            q_prev = q_j;
        }
        add_sample(acc, u);
        acc[2] += q0;
        acc[3] += 1.0;
    }
    finish_paths(acc, partials, a.fin);
}

static uint64_t align256(uint64_t x) { return (x + 255) & ~static_cast<uint64_t>(255); }

uint32_t american_cont_grid(uint64_t n_points)
{
    return static_cast<uint32_t>(n_points < 1 ? 1 : (n_points < kFoldMaxRecords ? n_points : kFoldMaxRecords));
}

AmDualLayout american_dual_layout(uint64_t n_local, uint32_t n_steps, uint32_t M, int precision)
{
    const uint64_t elem = precision == 32 ? 4 : 8;
    const uint64_t partials = std::max<uint64_t>(
        2ull * store_grid(n_local, precision),
        std::max<uint64_t>(static_cast<uint64_t>(kAmContRecord) * american_cont_grid(static_cast<uint64_t>(M) * n_local),
                           static_cast<uint64_t>(kAmDualRecord) * one_path_per_thread_grid(n_local)));
    AmDualLayout l;
    l.traj = 0;
    l.cont = l.traj + align256(static_cast<uint64_t>(n_steps) * n_local * elem);
    l.table = l.cont + align256(8 * static_cast<uint64_t>(M) * n_local);
    l.partials = l.table + align256(8 * static_cast<uint64_t>(kAmRow) * (M + 1));
    l.total = 256 + l.partials + align256(8 * partials);
    return l;
}

template <typename T, int MB>
static hipError_t cont_t(const AmDualJob &job, const void *traj, const double *table, double *Q, double *d_partials,
                         uint32_t grid, double *out, unsigned int *ticket, hipStream_t stream)
{
    AmContArgs<T> a;
    a.c = make_consts<T>(job.path);
    a.traj = static_cast<const T *>(traj);
    a.table = table;
    a.Q = Q;
    a.shard = PathShard{job.inner_seed, job.path.path_offset, job.path.n_local};
    a.n_points = static_cast<uint64_t>(job.M) * job.path.n_local;
    a.K = job.path.K;
    a.k = job.k;
    a.M = job.M;
    a.n_inner = job.n_inner;
    a.put = job.put;
    a.fin = GridFinish{out, ticket, -1.0};
    hipLaunchKernelGGL((am_cont_kernel<T, MB>), dim3(grid), dim3(kBlock), 0, stream, a, d_partials);
    return hipGetLastError();
}

template <typename T, int MB>
static hipError_t scan_t(const AmDualJob &job, const void *traj, const double *table, const double *Q,
                         double *d_partials, uint32_t grid, double *out, unsigned int *ticket, hipStream_t stream)
{
    AmScanArgs<T> a;
    a.traj = static_cast<const T *>(traj);
    a.table = table;
    a.Q = Q;
    a.n_local = job.path.n_local;
    a.K = job.path.K;
    a.k = job.k;
    a.M = job.M;
    a.put = job.put;
    a.fin = GridFinish{out, ticket, -1.0};
    hipLaunchKernelGGL((am_dual_scan_kernel<T, MB>), dim3(grid), dim3(kBlock), 0, stream, a, d_partials);
    return hipGetLastError();
}

#define MCAMD_AM_DISPATCH(FN, ...)                                                                       \
    switch (job.n_basis) {                                                                            \
    case 2: return job.path.precision == 32 ? FN<float, 2>(__VA_ARGS__) : FN<double, 2>(__VA_ARGS__); \
    case 3: return job.path.precision == 32 ? FN<float, 3>(__VA_ARGS__) : FN<double, 3>(__VA_ARGS__); \
    case 4: return job.path.precision == 32 ? FN<float, 4>(__VA_ARGS__) : FN<double, 4>(__VA_ARGS__); \
    default: return hipErrorInvalidValue;                                                             \
    }

static bool shape_ok(const AmDualJob &job, uint32_t grid)
{
    return grid >= 1 && grid <= kFoldMaxRecords && job.M >= 1 && job.M <= kAmMaxDates && job.k >= 1 && job.n_inner >= 1 &&
           job.path.n_local >= 1 && static_cast<uint64_t>(job.M) * job.k == job.path.n_steps;
}

hipError_t launch_american_cont(const AmDualJob &job, const void *traj, const double *table, double *Q,
                                double *d_partials, uint32_t grid, double *out, unsigned int *ticket,
                                hipStream_t stream)
{
    if (!traj || !table || !Q || !d_partials || !out || !ticket || !shape_ok(job, grid)) return hipErrorInvalidValue;
    MCAMD_AM_DISPATCH(cont_t, job, traj, table, Q, d_partials, grid, out, ticket, stream)
}

hipError_t launch_american_dual_scan(const AmDualJob &job, const void *traj, const double *table, const double *Q,
                                     double *d_partials, uint32_t grid, double *out, unsigned int *ticket,
                                     hipStream_t stream)
{
    if (!traj || !table || !Q || !d_partials || !out || !ticket || !shape_ok(job, grid)) return hipErrorInvalidValue;
    MCAMD_AM_DISPATCH(scan_t, job, traj, table, Q, d_partials, grid, out, ticket, stream)
}

#undef MCAMD_AM_DISPATCH

}  // namespace mcamd
