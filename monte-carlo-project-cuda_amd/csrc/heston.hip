// heston.hip — European options under Heston stochastic volatility, full-truncation Euler in the log-price, for gfx950
// (both path precisions).
//
// Definitions (include/mcamd.h, mcamd_price_heston): X_i = ln(S_i / S0) in NATURAL-log units and the raw variance v_i,
// moved by heston_device.hpp's heston_move.  Step i takes the normal z of the constant- and local-volatility kernels
// (normal i of Philox blocks 0, 1, .. of the path's subsequence) for the log-price and a second one, z' = normal i of
// blocks 2^63, 2^63 + 1, .. of the same subsequence (where lookback.hip keeps its step uniforms), for the variance:
// a block of the walk is two Philox blocks and two Box-Muller fills.  The path ends as localvol.hip's does, with one
// exponential.
//
// Beside the sample a path leaves two diagnostics of the scheme: how many steps it entered with v < 0 (a 32-bit
// counter, widened at the end) and its average variance (1 / n) sum v+_i (summed in the path precision in step order,
// scaled in fp64).  There is no table in LDS beyond what MathCtx<T> needs and no early exit.
#include "heston.hpp"
#include "heston_device.hpp"
#include "path_frame.hpp"

namespace mcamd {

template <typename T>
struct HestonArgs {
    HestonConsts<T> c;
    T exp_scale;              // exponent units per natural-log unit (log2 e in fp32, 65536 / ln 2 in fp64)
    T v0;
    T K, S0;
    double inv_n;             // 1 / n_steps
    int put;
    uint32_t n_steps;
    PathShard shard;
    T *samples;               // nullable
    T *state;                 // nullable: S_T at [i], v_n at [n_local + i]
    GridFinish fin;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void heston_kernel(HestonArgs<T> a, double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    const HestonConsts<T> c = heston_resident(a.c);
    const StepBlocks blocks = step_blocks<NB>(a.n_steps);
    double acc4[kHestonRecord] = {0.0, 0.0, 0.0, 0.0};
    for (const uint64_t i : ThreadPaths{a.shard.n_local}) {
        const uint64_t subsequence = a.shard.path_offset + i;
        T X = T(0);           // ln(S / S0), natural units
        T v = a.v0;           // the raw variance
        T v_sum = T(0);       // sum of v+ over the steps
        uint32_t trunc = 0;   // steps entered with v < 0
        HestonNormals<T> nz;
        walk_steps<NB>(
            blocks, [&](uint32_t kb) { nz.fill(m, key, subsequence, kb); },
            [&](uint32_t, int j) {
                trunc += v < T(0) ? 1u : 0u;
                v_sum += heston_move(X, v, nz.z.z[j], nz.zv.z[j], c);
            });
        const T St = exp_of_logreturn(a.S0, X * a.exp_scale, m);
        const T h = vanilla_payoff(a.put, a.K, St);
        const double y = static_cast<double>(h);
        if (a.samples) a.samples[i] = h;
        if (a.state) {
            a.state[i] = St;
            a.state[a.shard.n_local + i] = v;
        }
        add_sample(acc4, y);
        acc4[2] += static_cast<double>(trunc);
        acc4[3] += static_cast<double>(v_sum) * a.inv_n;
    }
    finish_paths(acc4, partials, a.fin);
}

template <typename T>
static hipError_t launch_heston_t(const HestonJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                  hipStream_t stream)
{
    HestonArgs<T> a;
    heston_walk_args<T>(a, j.walk);
    a.K = static_cast<T>(j.K);
    a.S0 = static_cast<T>(j.S0);
    a.inv_n = 1.0 / static_cast<double>(j.walk.paths.n_steps);
    a.put = j.put ? 1 : 0;
    a.n_steps = j.walk.paths.n_steps;
    a.samples = static_cast<T *>(j.d_samples);
    a.state = static_cast<T *>(j.d_state);
    a.fin = grid_finish_of(fs);
    hipLaunchKernelGGL((heston_kernel<T>), dim3(grid), dim3(kBlock), 0, stream, a, d_partials);
    return hipGetLastError();
}

hipError_t launch_heston(const HestonJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                         hipStream_t stream)
{
    if (!finish_ok(finish, grid)) return hipErrorInvalidValue;
    if (!heston_walk_ok(job.walk)) return hipErrorInvalidValue;
    return dispatch_precision(job.walk.paths.precision, [&](auto p) {
        return launch_heston_t<typename decltype(p)::type>(job, d_partials, grid, finish, stream);
    });
}

}  // namespace mcamd
