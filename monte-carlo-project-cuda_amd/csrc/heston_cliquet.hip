// heston_cliquet.hip — cliquets, forward-start options and realized-variance swaps under Heston stochastic volatility,
// for gfx950 (both path precisions).
//
// Definitions (include/mcamd.h, mcamd_price_heston_cliquet): the path is mcamd_price_heston's, X_i = ln(S_i / S0) in
// NATURAL-log units and the raw variance v_i, moved by heston_device.hpp's heston_move on the two normals of heston.hip
// (z of Philox blocks 0, 1, .., z' of blocks 2^63, 2^63 + 1, .. of the path's subsequence).  The reset dates, the
// period rule and the end of the path are cliquet.hip's, operation for operation: date p = 1..M falls on the end of step
// p reset_every, D_p = X at date p minus X at date p - 1, and a counted period (p >= first_period) adds
//   SUM       c_p = min(max(e^{D_p} - 1, lo), hi), A = sum c_p: one exponential per counted period;
//   COMPOUND  l_p = min(max(D_p, ln(1 + lo)), ln(1 + hi)), L = sum l_p, A = e^L - 1: one exponential per path, at the end;
//   VARIANCE  V = fma(D_p, D_p, V), A = V / (P tau): no exponential at all.
// y = min(max(A, global floor), global cap) in fp64.
//
// What a counted period adds and what the sum becomes at the end are cliquet_device.hpp's, stated once for both files.
//
// KIND is a template parameter, so the exponential exists in the SUM loop only.  The step index is wave-uniform: the
// reset test is a scalar compare, the period counter and "does this period count" are scalars.  A reset may fall on any
// step of a Philox block, so the test sits in the step.  A path also leaves heston.hip's two diagnostics: the steps it
// entered with v < 0 and its average variance.  There is no table in LDS beyond what MathCtx<T> needs and no early exit:
// every wavefront runs every step.
#include "heston_cliquet.hpp"
#include "cliquet_device.hpp"
#include "heston_device.hpp"
#include "path_frame.hpp"

namespace mcamd {

template <typename T>
struct HestonCliquetArgs {
    HestonConsts<T> c;
    T exp_scale;              // exponent units per natural-log unit (log2 e in fp32, 65536 / ln 2 in fp64)
    T v0;
    T lo, hi;                 // the local bounds: of R_p (SUM), of D_p (COMPOUND: ln(1 + bound)); unread by VARIANCE
    double g_lo, g_hi;        // the global bounds of A; -inf / +inf: none
    double scale;             // VARIANCE: 1 / (P tau)
    double inv_n;             // 1 / n_steps
    uint32_t n_steps, reset_every, first_period;
    PathShard shard;
    T *samples;               // nullable
    GridFinish fin;
};

template <typename T, int KIND>
__global__ __launch_bounds__(kBlock) void heston_cliquet_kernel(HestonCliquetArgs<T> a, double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    const HestonConsts<T> c = heston_resident(a.c);
    // the payoff's three constants live as heston_resident keeps the step's
    const T lo = resident_t(a.lo), hi = resident_t(a.hi), exp_scale = resident_t(a.exp_scale);
    const StepBlocks blocks = step_blocks<NB>(a.n_steps);
    // an infinite bound never binds and counts nothing, whatever the arithmetic made of A
    const bool has_floor = a.g_lo > -__builtin_huge_val(), has_cap = a.g_hi < __builtin_huge_val();
    double acc6[kHestonCliquetRecord] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (const uint64_t i : ThreadPaths{a.shard.n_local}) {
        const uint64_t subsequence = a.shard.path_offset + i;
        T X = T(0);           // ln(S / S0), natural units
        T v = a.v0;           // the raw variance
        T X_reset = T(0);     // X at the last reset date
        T sum = T(0);         // sum c_p (SUM), sum l_p (COMPOUND), sum D_p^2 (VARIANCE)
        T v_sum = T(0);       // sum of v+ over the steps
        uint32_t trunc = 0;   // steps entered with v < 0
        uint32_t p = 0;                         // reset dates behind the wavefront
        uint32_t next_reset = a.reset_every;    // the step that ends on date p + 1
        HestonNormals<T> nz;
        // step `index` (wave-uniform) with the log-price normal z and the variance's own zv
        auto step = [&](T z, T zv, uint32_t index) {
            trunc += v < T(0) ? 1u : 0u;
            v_sum += heston_move(X, v, z, zv, c);
            if (index + 1 == next_reset) {   // a scalar compare
                const T D = X - X_reset;
                X_reset = X;
                if (p + 1 >= a.first_period) cliquet_add_period<KIND>(sum, D, lo, hi, exp_scale, m);
                ++p;
                next_reset += a.reset_every;
            }
        };
        walk_steps<NB>(
            blocks, [&](uint32_t kb) { nz.fill(m, key, subsequence, kb); },
            [&](uint32_t kb, int j) { step(nz.z.z[j], nz.zv.z[j], kb * NB + j); });
        const double A = cliquet_amount<KIND>(sum, exp_scale, a.scale, m);
        const double y = __builtin_fmin(__builtin_fmax(A, a.g_lo), a.g_hi);
        if (a.samples) a.samples[i] = static_cast<T>(y);
        add_sample(acc6, y);
        acc6[2] += (has_floor && A <= a.g_lo) ? 1.0 : 0.0;
        acc6[3] += (has_cap && A >= a.g_hi) ? 1.0 : 0.0;
        acc6[4] += static_cast<double>(v_sum) * a.inv_n;
        acc6[5] += static_cast<double>(trunc);
    }
    finish_paths(acc6, partials, a.fin);
}

template <typename T, int KIND>
static void launch_heston_cliquet_k(const HestonCliquetArgs<T> &a, double *d_partials, uint32_t grid, hipStream_t stream)
{
    hipLaunchKernelGGL((heston_cliquet_kernel<T, KIND>), dim3(grid), dim3(kBlock), 0, stream, a, d_partials);
}

template <typename T>
static hipError_t launch_heston_cliquet_t(const HestonCliquetJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                          hipStream_t stream)
{
    HestonCliquetArgs<T> a;
    heston_walk_args<T>(a, j.walk);
    a.lo = static_cast<T>(j.local_lo);
    a.hi = static_cast<T>(j.local_hi);
    a.g_lo = j.global_lo;
    a.g_hi = j.global_hi;
    a.scale = j.scale;
    a.inv_n = 1.0 / static_cast<double>(j.walk.paths.n_steps);
    a.n_steps = j.walk.paths.n_steps;
    a.reset_every = j.reset_every;
    a.first_period = j.first_period;
    a.samples = static_cast<T *>(j.d_samples);
    a.fin = grid_finish_of(fs);
    if (j.kind == kCliquetSum) launch_heston_cliquet_k<T, kCliquetSum>(a, d_partials, grid, stream);
    else if (j.kind == kCliquetCompound) launch_heston_cliquet_k<T, kCliquetCompound>(a, d_partials, grid, stream);
    else launch_heston_cliquet_k<T, kCliquetVariance>(a, d_partials, grid, stream);
    return hipGetLastError();
}

hipError_t launch_heston_cliquet(const HestonCliquetJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                                 hipStream_t stream)
{
    if (!finish_ok(finish, grid)) return hipErrorInvalidValue;
    if (!heston_walk_ok(job.walk)) return hipErrorInvalidValue;
    const PathRange &paths = job.walk.paths;
    if (job.kind < kCliquetSum || job.kind > kCliquetVariance || job.reset_every == 0 ||
        paths.n_steps % job.reset_every != 0 || job.first_period == 0 ||
        job.first_period > paths.n_steps / job.reset_every)
        return hipErrorInvalidValue;
    return dispatch_precision(paths.precision, [&](auto p) {
        return launch_heston_cliquet_t<typename decltype(p)::type>(job, d_partials, grid, finish, stream);
    });
}

}  // namespace mcamd
