// greeks.hip — in-kernel Greeks for gfx950 (both path precisions): the pathwise kernel on the window-less pair-sum
// loop, and the likelihood-ratio (LR) kernel on the log-space stepping loop of simulate_sample.
//
// Each path contributes one undiscounted sample of price, delta, gamma, vega, rho and theta, formed ONCE per path in
// fp64 from the path-precision state; the block record is the sum and the sum of squares of each (12 doubles),
// summed over the grid by its last workgroup (grid_finish), exactly as the pricing kernel finishes its own sum.
// A path draws the same Philox numbers and takes the same steps as in mcamd_price_paths, so the price sample is the
// same payoff, and the sums are sharding-invariant up to fp64 summation order.
//
// Notation (include/mcamd.h): S_s the segment's start price, T_h = n_sim dt, L = ln(S_T / S_s), z_i the normals,
// D = exp(-r T) applied on the host.
//   pathwise (European only): delta 1{S_T>K} S_T / S_s;  gamma (mixed PW-LR) 1{S_T>K} K (L - (r - v^2/2) T_h) /
//     (S_s^2 v^2 T_h);  vega 1{S_T>K} S_T (L - (r + v^2/2) T_h) / v;  rho -T (S_T-K)+ + 1{S_T>K} S_T T_h;
//     theta r (S_T-K)+ - 1{S_T>K} S_T ((r - v^2/2) + (L - (r - v^2/2) T) / (2T))  (Tk = 0, dt = T / n_steps only).
//   LR (any payoff, y the payoff): delta y z_1 / (S_s v sqrt(dt));  gamma y ((z_1^2 - 1) / (S_s^2 v^2 dt) -
//     z_1 / (S_s^2 v sqrt(dt)));  vega y sum_i ((z_i^2 - 1) / v - z_i sqrt(dt));  rho y (sum_i z_i sqrt(dt) / v - T).
// The LR loop carries, besides ln(S_t / S_s) and the barrier count, the running sum of the squared step deviations
// x - drift = vol z (one subtract and one fma per step); z_1 and sum z_i come from the first step and the log price.
#include "greeks.hpp"
#include "path_consts.hpp"
#include "path_frame.hpp"

namespace mcamd {

template <typename T>
struct GreeksArgs {
    StepConsts<T> c;
    GreeksConsts g;
    PathShard shard;
    GridFinish fin;   // fin.out: the 16-double statistics record
};

// one path's six samples into the running (sum, sumsq) pairs
__device__ __forceinline__ void add_greeks(double (&acc)[kGreeksRecord], const double (&q)[kGreeks])
{
#pragma unroll
    for (int k = 0; k < kGreeks; ++k) {
        acc[2 * k] += q[k];
        acc[2 * k + 1] = __builtin_fma(q[k], q[k], acc[2 * k + 1]);
    }
}

// n and the zero tail of the statistics record (grid_finish writes [0..12)); one lane of the grid, at launch
template <typename T>
__device__ __forceinline__ void write_stats_tail(const GreeksArgs<T> &a)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.fin.out[kGreeksRecord] = static_cast<double>(a.shard.n_local);
        for (int k = kGreeksRecord + 1; k < kGreeksStats; ++k) a.fin.out[k] = 0.0;
    }
}

// pay = (S_T - K)+ and S_T of the path precision; x = ln(S_T / S_s) in the precision's exponent units
template <typename T>
__device__ __forceinline__ void pathwise_samples(const GreeksConsts &g, T pay, T St_t, T x, double (&q)[kGreeks])
{
    const double y = static_cast<double>(pay);
    const double St = static_cast<double>(St_t);
    const double L = static_cast<double>(x) * g.inv_scale;
    const bool itm = pay > T(0);
    q[0] = y;
    q[1] = itm ? St / g.S_s : 0.0;
    q[2] = itm ? g.K * (L - g.mu_h) * g.gamma_pw : 0.0;
    q[3] = itm ? St * (L - g.nu_h) / g.v : 0.0;
    q[4] = itm ? __builtin_fma(-g.T, y, St * g.T_h) : -g.T * y;
    q[5] = g.theta_on ? __builtin_fma(g.r, y, itm ? -St * __builtin_fma(L - g.theta_mu_T, g.inv_2T, g.theta_mu) : 0.0)
                      : 0.0;
}

// y the payoff; z1 the first normal, sz = sum z_i, szz = sum z_i^2 over the n_sim steps
__device__ __forceinline__ void lr_samples(const GreeksConsts &g, double y, double z1, double sz, double szz,
                                           double n_sim, double (&q)[kGreeks])
{
    q[0] = y;
    q[1] = y * z1 * g.delta_lr;
    q[2] = y * __builtin_fma(__builtin_fma(z1, z1, -1.0), g.gamma_lr1, -z1 * g.gamma_lr2);
    q[3] = y * __builtin_fma(szz - n_sim, 1.0 / g.v, -g.sqrt_dt * sz);
    q[4] = y * __builtin_fma(sz, g.sqrt_dt / g.v, -g.T);
    q[5] = 0.0;   // no LR theta: the host reports NaN
}

// European only: the pair-sum loop and launch shape of the default window-less price_kernel; the price sample is
// that kernel's payoff, bit for bit (sample_from_pair_sum), and the other five are an epilogue per path.
template <typename T>
__global__ __launch_bounds__(kBlock) void greeks_pathwise_kernel(GreeksArgs<T> a, double *__restrict__ partials)
{
    constexpr int NP = kPairSumPaths;
    const MathCtx<T> m = MathCtx<T>::template init<true>();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    const StepConsts<T> c = resident(a.c);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    write_stats_tail(a);
    double acc[kGreeksRecord];
#pragma unroll
    for (int k = 0; k < kGreeksRecord; ++k) acc[k] = 0.0;
    // path groups, not paths: the bound g NP < n_local stays a multiplication (ThreadPaths would need the division)
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; g * NP < a.shard.n_local; g += stride) {
        T sums[NP];
        pair_sums_of_paths<T, NP>(m, key, a.shard.path_offset + g * NP, c.n_sim, sums);
#pragma unroll
        for (int p = 0; p < NP; ++p)
            if (g * NP + p < a.shard.n_local) {
                const Sample<T> s = sample_from_pair_sum<T, false>(c, m, sums[p], c.S_start, c.n_sim);
                // the exponent sample_from_pair_sum exponentiated: ln(S_T / S_s) in exponent units
                const T x = fma_t(sums[p], c.vol * PairSum<T>::kUnit, c.drift * static_cast<T>(c.n_sim));
                double q[kGreeks];
                pathwise_samples<T>(a.g, s.pay, s.ctrl, x, q);
                add_greeks(acc, q);
            }
    }
    finish_paths(acc, partials, a.fin);
}

// The log-space stepping loop of simulate_sample (LOGSPACE, no antithetic twin), one path per thread, with the same
// exponents, barrier test and — WINDOW — the same early exit once every lane's window is closed: the payoff, and so
// every LR sample, is 0 there, so the exit stays exact.  (No lane compaction: big bullet jobs run this loop as is.)
template <typename T, bool WINDOW>
__global__ __launch_bounds__(kBlock) void greeks_lr_kernel(GreeksArgs<T> a, double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    const StepConsts<T> c = resident(a.c);
    const ThreadPaths paths(a.shard.n_local);   // made at the loop, the fp64 kernels compile to other instructions
    const uint32_t n_full = c.n_sim / NB;
    const uint32_t rem = c.n_sim - n_full * NB;
    const double inv_vol = 1.0 / static_cast<double>(c.vol);   // exponent units per normal
    const double n_drift = static_cast<double>(c.drift) * static_cast<double>(c.n_sim);
    write_stats_tail(a);
    double acc[kGreeksRecord];
#pragma unroll
    for (int k = 0; k < kGreeksRecord; ++k) acc[k] = 0.0;
    for (const uint64_t i : paths) {
        const uint64_t subsequence = a.shard.path_offset + i;
        int32_t count = c.Ik;
        T lg = T(0);    // ln(S_t / S_s) in exponent units
        T sq = T(0);    // sum of (x - drift)^2 = vol^2 sum z^2
        T d1 = T(0);    // x_1 - drift = vol z_1
        bool rem_live = true;
        Exponents<T> ex;
        auto step = [&](T x) {
            lg += x;
            if (WINDOW) count += (c.logB > lg) ? 1 : 0;
            const T d = x - c.drift;
            sq = fma_t(d, d, sq);
        };
        for (uint32_t k = 0; k < n_full; ++k) {
            ex.fill(m, c, key, subsequence, k);
            if (k == 0) d1 = ex.x[0] - c.drift;
#pragma unroll
            for (int j = 0; j < NB; ++j) step(ex.x[j]);
            if (WINDOW && window_open_lanes<false>(count, count, c.P2) == 0) {
                rem_live = false;
                break;
            }
        }
        if (rem && rem_live) {
            ex.fill(m, c, key, subsequence, n_full);
            if (n_full == 0) d1 = ex.x[0] - c.drift;
#pragma unroll
            for (int j = 0; j < NB - 1; ++j)
                if (static_cast<uint32_t>(j) < rem) step(ex.x[j]);
        }
        const T St = exp_of_logreturn(c.S_start, lg, m);
        const double y = static_cast<double>(payoff<T, WINDOW>(St, count, c));
        const double z1 = static_cast<double>(d1) * inv_vol;
        const double sz = (static_cast<double>(lg) - n_drift) * inv_vol;
        const double szz = static_cast<double>(sq) * inv_vol * inv_vol;
        double q[kGreeks];
        lr_samples(a.g, y, z1, sz, szz, static_cast<double>(c.n_sim), q);
        add_greeks(acc, q);
    }
    finish_paths(acc, partials, a.fin);
}

uint32_t greeks_grid(const GreeksJob &job)
{
    if (!job.lr) {
        const uint32_t blocks = price_grid(job.path, 0);   // window-less log-space job: the pair-sum loop's shape
        return blocks < kFoldMaxRecords ? blocks : kFoldMaxRecords;
    }
    // short paths: enough grid-stride trips per thread for 32 steps
    const uint64_t per_thread = job.path.n_sim >= 32 ? 1 : (32 + job.path.n_sim - 1) / job.path.n_sim;
    return one_path_per_thread_grid((job.path.n_local + per_thread - 1) / per_thread);
}

template <typename T>
static hipError_t launch_greeks_t(const GreeksJob &j, double *d_partials, uint32_t grid, double *out,
                                  unsigned int *ticket, hipStream_t stream)
{
    GreeksConsts gc = j.g;
    gc.inv_scale = exponent_unit<T>();
    const GreeksArgs<T> a{make_consts<T>(j.path), gc, shard_of(j.path), GridFinish{out, ticket, -1.0}};
    const dim3 g(grid), b(kBlock);
    if (!j.lr) hipLaunchKernelGGL((greeks_pathwise_kernel<T>), g, b, 0, stream, a, d_partials);
    else if (j.path.window) hipLaunchKernelGGL((greeks_lr_kernel<T, true>), g, b, 0, stream, a, d_partials);
    else hipLaunchKernelGGL((greeks_lr_kernel<T, false>), g, b, 0, stream, a, d_partials);
    return hipGetLastError();
}

hipError_t launch_greeks(const GreeksJob &job, double *d_partials, uint32_t grid, double *out, unsigned int *ticket,
                         hipStream_t stream)
{
    if (!out || !ticket || grid > kFoldMaxRecords) return hipErrorInvalidValue;
    return dispatch_precision(job.path.precision, [&](auto p) {
        return launch_greeks_t<typename decltype(p)::type>(job, d_partials, grid, out, ticket, stream);
    });
}

}  // namespace mcamd
