// cliquet.hip — cliquets, forward-start options and realized-variance swaps under a local-volatility surface, for gfx950
// (both path precisions).
//
// Definitions (include/mcamd.h, mcamd_price_cliquet): the path is mcamd_price_localvol's, X_i = ln(S_i / S0) in
// NATURAL-log units, walked by localvol_device.hpp's lookup, row carry and move on the normals of localvol.hip (one per
// step, whole Philox blocks, the remainder block as there).  Reset date p = 1..M falls on the end of step p reset_every;
// D_p = X at date p minus X at date p - 1.  What a counted period (p >= first_period) adds depends on KIND:
//   SUM       c_p = min(max(e^{D_p} - 1, lo), hi), A = sum c_p: one exponential per counted period;
//   COMPOUND  l_p = min(max(D_p, ln(1 + lo)), ln(1 + hi)), L = sum l_p, A = e^L - 1: one exponential per path, at the end;
//   VARIANCE  V = fma(D_p, D_p, V), A = V / (P tau): no exponential at all.
// y = min(max(A, global floor), global cap) in fp64.  What a counted period adds and what the sum becomes at the end are
// cliquet_device.hpp's, shared with heston_cliquet.hip.
//
// KIND is a template parameter, so the exponential exists in the SUM loop only.  The step index is wave-uniform: the
// reset test is a scalar compare of the step with the step of the next reset, the period counter and "does this period
// count" are scalars, and no lane divides or takes a remainder (autocall.hip's date counter).  A reset may fall on any
// step of a Philox block (reset_every may be 1, odd, or larger than a block), so the test sits in the step, not at the
// block ends.  There is no early exit: every wavefront runs every step.
#include "cliquet.hpp"
#include "cliquet_device.hpp"
#include "localvol_device.hpp"
#include "path_frame.hpp"

namespace mcamd {

template <typename T>
struct CliquetArgs {
    LvSurface<T> surf;
    T mu_dt, half_dt, sqrt_dt;
    T exp_scale;              // exponent units per natural-log unit (log2 e in fp32, 65536 / ln 2 in fp64)
    T lo, hi;                 // the local bounds: of R_p (SUM), of D_p (COMPOUND: ln(1 + bound)); unread by VARIANCE
    double g_lo, g_hi;        // the global bounds of A; -inf / +inf: none
    double scale;             // VARIANCE: 1 / (P tau)
    uint32_t n_steps, reset_every, first_period;
    PathShard shard;
    T *samples;               // nullable
    GridFinish fin;
};

template <typename T, int KIND>
__global__ __launch_bounds__(kBlock) void cliquet_kernel(CliquetArgs<T> a, double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    VolPair<T> *tab = reinterpret_cast<VolPair<T> *>(lv_table_lds);
    lv_copy_table(tab, 0, a.surf.table, a.surf.rows.n_entries);
    __syncthreads();
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    const LvAxis<T> axis = lv_resident(a.surf.axis);
    const T mu_dt = resident_t(a.mu_dt), half_dt = resident_t(a.half_dt), sqrt_dt = resident_t(a.sqrt_dt);
    const T lo = resident_t(a.lo), hi = resident_t(a.hi), exp_scale = resident_t(a.exp_scale);
    const StepBlocks blocks = step_blocks<NB>(a.n_steps);
    // an infinite bound never binds and counts nothing, whatever the arithmetic made of A
    const bool has_floor = a.g_lo > -__builtin_huge_val(), has_cap = a.g_hi < __builtin_huge_val();
    double acc5[kCliquetRecord] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (const uint64_t i : ThreadPaths{a.shard.n_local}) {
        const uint64_t subsequence = a.shard.path_offset + i;
        T X = T(0);          // ln(S / S0), natural units
        T X_reset = T(0);    // X at the last reset date
        T sum = T(0);        // sum c_p (SUM), sum l_p (COMPOUND), sum D_p^2 (VARIANCE)
        uint32_t p = 0;                         // reset dates behind the wavefront
        uint32_t next_reset = a.reset_every;    // the step that ends on date p + 1
        LvRow row{0, 0};
        Normals<T> nz;
        // step `index` (wave-uniform) with the normal z
        auto step = [&](T z, uint32_t index) {
            const T s = lv_sigma(X, axis, a.surf.rows, tab, row);
            lv_move(X, s, z, sqrt_dt, half_dt, mu_dt);
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
            [&](uint32_t kb, int j) { step(nz.z[j], kb * NB + j); });
        const double A = cliquet_amount<KIND>(sum, exp_scale, a.scale, m);
        const double y = __builtin_fmin(__builtin_fmax(A, a.g_lo), a.g_hi);
        if (a.samples) a.samples[i] = static_cast<T>(y);
        add_sample(acc5, y);
        acc5[2] += (has_floor && A <= a.g_lo) ? 1.0 : 0.0;
        acc5[3] += (has_cap && A >= a.g_hi) ? 1.0 : 0.0;
        add_wave_steps(acc5[4], a.n_steps);
    }
    if (a.fin.n_value >= 0.0) acc5[4] = 0.0;   // the 6-double statistics layout has no slot for the step counter
    finish_paths(acc5, partials, a.fin);
}

template <typename T, int KIND>
static void launch_cliquet_k(const CliquetArgs<T> &a, double *d_partials, uint32_t grid, hipStream_t stream)
{
    const size_t lds_bytes = static_cast<size_t>(a.surf.rows.n_entries) * sizeof(VolPair<T>);
    hipLaunchKernelGGL((cliquet_kernel<T, KIND>), dim3(grid), dim3(kBlock), lds_bytes, stream, a, d_partials);
}

template <typename T>
static hipError_t launch_cliquet_t(const CliquetJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                   hipStream_t stream)
{
    CliquetArgs<T> a;
    lv_step_args<T>(a, j.walk);
    a.shard = shard_of(j.walk.paths);
    a.lo = static_cast<T>(j.local_lo);
    a.hi = static_cast<T>(j.local_hi);
    a.g_lo = j.global_lo;
    a.g_hi = j.global_hi;
    a.scale = j.scale;
    a.n_steps = j.walk.paths.n_steps;
    a.reset_every = j.reset_every;
    a.first_period = j.first_period;
    a.samples = static_cast<T *>(j.d_samples);
    a.fin = grid_finish_of(fs);
    if (j.kind == kCliquetSum) launch_cliquet_k<T, kCliquetSum>(a, d_partials, grid, stream);
    else if (j.kind == kCliquetCompound) launch_cliquet_k<T, kCliquetCompound>(a, d_partials, grid, stream);
    else launch_cliquet_k<T, kCliquetVariance>(a, d_partials, grid, stream);
    return hipGetLastError();
}

hipError_t launch_cliquet(const CliquetJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                          hipStream_t stream)
{
    if (!finish_ok(finish, grid)) return hipErrorInvalidValue;
    const uint32_t n_steps = job.walk.paths.n_steps;
    if (!lv_grid_ok(job.walk.surface, n_steps)) return hipErrorInvalidValue;
    if (job.kind < kCliquetSum || job.kind > kCliquetVariance || job.reset_every == 0 ||
        n_steps % job.reset_every != 0 || job.first_period == 0 || job.first_period > n_steps / job.reset_every)
        return hipErrorInvalidValue;
    return dispatch_precision(job.walk.paths.precision, [&](auto p) {
        return launch_cliquet_t<typename decltype(p)::type>(job, d_partials, grid, finish, stream);
    });
}

}  // namespace mcamd
