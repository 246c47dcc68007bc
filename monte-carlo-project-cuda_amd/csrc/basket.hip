// basket.hip — options on d = 1..8 correlated assets for gfx950 (both path precisions): arithmetic and geometric
// baskets (spreads and exchange options are arithmetic baskets with a negative weight), best-of and worst-of, call or
// put; best-of and worst-of optionally with a barrier on the aggregate, tested at the step ends.
//
// Definitions (include/mcamd.h, mcamd_price_basket): X_{j,i} = ln(S_{j,i} / S0_j) after step i, X_{j,0} = 0,
// X_{j,i} = X_{j,i-1} + x_{j,i}, x_{j,i} = drift_j + sum_{k <= j} c_jk z_{i,k} with c_jk = v_j sqrt(dt) L_jk and L the
// lower Cholesky factor of the correlation matrix; the sum is a chain of fused multiply-adds in ascending k that starts
// from the drift.  z_{i,k} is normal number i d + k of the path's stream: Philox block (i d + k) / NB, slot
// (i d + k) % NB of Normals<T>::z.  With d = 1 that is the normal the barrier and lookback kernels step with.
//
// The loop walks the stream in whole Philox blocks: G = NB / gcd(D, NB) steps consume G D / NB whole blocks, so a
// group of G steps is unrolled with the block boundaries at compile-time positions, and the last n_steps % G steps run
// the same code under a wave-uniform count.  Per step: D (D + 1) / 2 fused multiply-adds, D adds and — monitored — D
// adds, D - 1 max / min and one compare, all in log space: no exponential before maturity.  The D accumulators, the D
// drifts and the D (D + 1) / 2 coefficients stay in registers (D is a template argument): in fp32 in VECTOR registers
// (a scalar operand doubles the issue time of v_fma_f32: vgpr_resident), in fp64 wherever the compiler puts them (an
// fp64 instruction takes its cycles whatever its operands).  Kind, payoff, barrier side and knock-in / knock-out are
// wave-uniform selects.  A knock-out wavefront leaves the loop at the first group end where every lane has hit.
#include "basket.hpp"
#include "path_consts.hpp"
#include "path_frame.hpp"
#include "basket_device.hpp"

namespace mcamd {

template <typename T, int D>
struct BasketArgs {
    T drift[D];                // exponent units
    T coef[D * (D + 1) / 2];   // exponent units, [j (j + 1) / 2 + k]
    T log_w[D];                // best / worst: ln(w_j S0_j) in exponent units; geometric: [0] = sum_j w_j ln S0_j, likewise
    T w_t[D];                  // geometric: the weights in the path precision
    T S0[D];                   // arithmetic: the spots in the path precision
    T logB;                    // ln B in exponent units
    double w[D];               // arithmetic: the weights
    double K;
    int kind, put, up, out;
    uint32_t n_steps;
    PathShard shard;
    T *samples;                // nullable
    GridFinish fin;
};

template <typename T, int D, bool MONITORED>
__global__ __launch_bounds__(kBlock) void basket_kernel(BasketArgs<T, D> a, double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    constexpr int G = NB / gcd_c(D, NB);   // steps that consume whole blocks
    constexpr int BPG = G * D / NB;        // the blocks they consume
    constexpr int NC = D * (D + 1) / 2;
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    T drift[D], coef[NC], log_w[D];
#pragma unroll
    for (int j = 0; j < D; ++j) drift[j] = bk_resident<D>(a.drift[j]);
#pragma unroll
    for (int c = 0; c < NC; ++c) coef[c] = bk_resident<D>(a.coef[c]);
#pragma unroll
    for (int j = 0; j < D; ++j) log_w[j] = MONITORED ? bk_resident<D>(a.log_w[j]) : a.log_w[j];
    const bool best = a.kind == kBasketBestOf;
    const ThreadPaths paths(a.shard.n_local);   // made at the loop, the monitored fp32 kernel of 3 assets runs 4.7 % slower
    const uint32_t n_groups = a.n_steps / G;
    const uint32_t rem = a.n_steps - n_groups * G;
    double acc4[kBasketRecord] = {0.0, 0.0, 0.0, 0.0};
    for (const uint64_t i : paths) {
        const uint64_t subsequence = a.shard.path_offset + i;
        T X[D];              // ln(S_j / S0_j) so far, in exponent units
#pragma unroll
        for (int j = 0; j < D; ++j) X[j] = T(0);
        bool alive = true;   // not yet hit
        uint32_t live = 0;   // steps this path entered not yet hit
        uint32_t steps_run = a.n_steps;
        Normals<T> nz;
        // the log of the best or the worst of the weighted prices, in exponent units
        auto extreme = [&]() {
            T l = log_w[0] + X[0];
#pragma unroll
            for (int j = 1; j < D; ++j) l = best ? bk_max(l, log_w[j] + X[j]) : bk_min(l, log_w[j] + X[j]);
            return l;
        };
        // steps g G .. g G + count - 1 (count <= G, wave-uniform): normals g G D .. of the stream
        auto group = [&](uint32_t g, uint32_t count) {
            const uint64_t first_block = static_cast<uint64_t>(g) * BPG;
#pragma unroll
            for (int s = 0; s < G; ++s) {
                if (static_cast<uint32_t>(s) < count) {
                    T x[D];
#pragma unroll
                    for (int j = 0; j < D; ++j) x[j] = drift[j];
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        const int flat = s * D + k;   // a compile-time position once unrolled
                        if (flat % NB == 0) nz.fill(m, key, subsequence, first_block + flat / NB);
                        const T z = nz.z[flat % NB];
#pragma unroll
                        for (int j = k; j < D; ++j) x[j] = fma_t(coef[j * (j + 1) / 2 + k], z, x[j]);
                    }
#pragma unroll
                    for (int j = 0; j < D; ++j) X[j] += x[j];
                    if (MONITORED) {
                        live += alive ? 1u : 0u;
                        const T l = extreme();
                        const bool hit = a.up ? (l >= a.logB) : (l <= a.logB);
                        alive = alive && !hit;
                    }
                }
            }
        };
        bool finished = true;
        for (uint32_t g = 0; g < n_groups; ++g) {
            group(g, G);
            if (MONITORED && a.out && __builtin_amdgcn_ballot_w64(alive) == 0) {
                steps_run = (g + 1) * G;
                finished = false;
                break;
            }
        }
        if (rem && finished) group(n_groups, rem);
        // the aggregate at maturity, in fp64 from path-precision values
        double A;
        if (a.kind == kBasketArithmetic) {
            A = 0.0;
#pragma unroll
            for (int j = 0; j < D; ++j)
                A = __builtin_fma(a.w[j], static_cast<double>(exp_of_logreturn(a.S0[j], X[j], m)), A);
        } else {
            T l;
            if (a.kind == kBasketGeometric) {
                l = a.log_w[0];
#pragma unroll
                for (int j = 0; j < D; ++j) l = fma_t(a.w_t[j], X[j], l);
            } else {
                l = extreme();
            }
            A = static_cast<double>(exp_of_logreturn(T(1), l, m));
        }
        double y = a.put ? a.K - A : A - a.K;
        y = y > 0.0 ? y : 0.0;
        // a knocked-out path pays 0 whatever its (possibly unfinished) prices are
        if (MONITORED) y = (alive == (a.out != 0)) ? y : 0.0;
        if (a.samples) a.samples[i] = static_cast<T>(y);
        add_sample(acc4, y);
        add_counters(acc4, steps_run, live);
    }
    if (a.fin.n_value >= 0.0) acc4[2] = acc4[3] = 0.0;   // the 6-double statistics layout has no slot for the counters
    finish_paths(acc4, partials, a.fin);
}

template <typename T, int D>
static hipError_t launch_basket_d(const BasketJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                  hipStream_t stream)
{
    const double u = exponent_unit<T>();   // natural log per exponent unit
    BasketArgs<T, D> a{};
    for (int q = 0; q < D; ++q) {
        a.drift[q] = static_cast<T>(j.drift[q] / u);
        a.log_w[q] = static_cast<T>(j.log_w[q] / u);
        a.w_t[q] = static_cast<T>(j.w[q]);
        a.S0[q] = static_cast<T>(j.S0[q]);
        a.w[q] = j.w[q];
    }
    for (int c = 0; c < D * (D + 1) / 2; ++c) a.coef[c] = static_cast<T>(j.coef[c] / u);
    a.logB = static_cast<T>(j.logB / u);
    a.K = j.K;
    a.kind = j.kind;
    a.put = j.put ? 1 : 0;
    a.up = j.up ? 1 : 0;
    a.out = j.out ? 1 : 0;
    a.n_steps = j.path.n_sim;
    a.shard = shard_of(j.path);
    a.samples = static_cast<T *>(j.d_samples);
    a.fin = grid_finish_of(fs);
    const dim3 g(grid), b(kBlock);
    if (j.monitored) hipLaunchKernelGGL((basket_kernel<T, D, true>), g, b, 0, stream, a, d_partials);
    else hipLaunchKernelGGL((basket_kernel<T, D, false>), g, b, 0, stream, a, d_partials);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_basket_t(const BasketJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                  hipStream_t stream)
{
    return dispatch_assets(j.d, [&](auto d) {
        return launch_basket_d<T, decltype(d)::value>(j, d_partials, grid, fs, stream);
    });
}

hipError_t launch_basket(const BasketJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                         hipStream_t stream)
{
    if (!finish_ok(finish, grid)) return hipErrorInvalidValue;
    if (job.monitored && job.kind != kBasketBestOf && job.kind != kBasketWorstOf) return hipErrorInvalidValue;
    return dispatch_precision(job.path.precision, [&](auto p) {
        return launch_basket_t<typename decltype(p)::type>(job, d_partials, grid, finish, stream);
    });
}

}  // namespace mcamd
