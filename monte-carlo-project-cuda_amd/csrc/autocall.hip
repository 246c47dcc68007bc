// autocall.hip — worst-of autocallable notes on d = 1..8 correlated assets for gfx950 (both path precisions).
//
// Definitions (include/mcamd.h, mcamd_price_autocall): X_{j,i} = ln(S_{j,i} / S_{j,0}) after step i, stepped exactly as
// basket.hip steps it — x_{j,i} = drift_j + sum_{k <= j} c_jk z_{i,k}, a chain of fused multiply-adds in ascending k from
// the drift, z_{i,k} normal number i d + k of the path's stream — and l_i = min_j X_{j,i}, the log of the worst
// performance, in exponent units.  Observation date q = 1..M falls on the end of step q observe_every.  A path is called
// at the first date q >= first_call_date with l >= ln L_q and is paid pay_q (a double of the host's table, maturity
// money); a path never called pays 1, or min(A_n, 1) with A_n = exp(l_n) once knocked in (l <= ln ki_level at maturity,
// or at any step end).
//
// The loop is basket.hip's: G = NB / gcd(D, NB) steps consume whole Philox blocks and are unrolled with the block
// boundaries at compile-time positions; the D accumulators, the D drifts and the D (D + 1) / 2 coefficients stay in
// registers (bk_resident).  Per step: D (D + 1) / 2 fused multiply-adds and D adds; with KI_EVERY_STEP also D - 1 min
// and one compare — D adds fewer than basket.hip's monitored step, because a performance carries no ln(w_j S0_j).  The
// step index is wave-uniform, so the observation test is a scalar compare against the step of the next date (no divide,
// no modulo), the date counter is a scalar, and ln L_q and pay_q are scalar loads from the kernel arguments.  Without
// KI_EVERY_STEP the minimum is taken at the observation dates only.  No exponential is taken before maturity, and none
// at all by a wavefront whose lanes have all been called: it leaves the loop at the first group end where that is so.
#include "autocall.hpp"
#include "path_consts.hpp"
#include "path_frame.hpp"
#include "basket_device.hpp"

namespace mcamd {

template <typename T, int D>
struct AutocallArgs {
    T drift[D];                      // exponent units
    T coef[D * (D + 1) / 2];         // exponent units, [j (j + 1) / 2 + k]
    T log_level[kAutocallMaxDates];  // ln L_q in exponent units at [q - 1]
    T log_ki;                        // ln ki_level in exponent units
    double pay[kAutocallMaxDates];   // pay_q at [q - 1]
    double dt;
    int ki;                          // a knock-in applies (always, with KI_EVERY_STEP)
    uint32_t n_steps, observe_every, first_call_date;
    PathShard shard;
    T *samples;                      // nullable
    GridFinish fin;
};

template <typename T, int D, bool KI_EVERY_STEP>
__global__ __launch_bounds__(kBlock) void autocall_kernel(AutocallArgs<T, D> a, double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    constexpr int G = NB / gcd_c(D, NB);   // steps that consume whole blocks
    constexpr int BPG = G * D / NB;        // the blocks they consume
    constexpr int NC = D * (D + 1) / 2;
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    T drift[D], coef[NC];
#pragma unroll
    for (int j = 0; j < D; ++j) drift[j] = bk_resident<D>(a.drift[j]);
#pragma unroll
    for (int c = 0; c < NC; ++c) coef[c] = bk_resident<D>(a.coef[c]);
    const uint32_t n_groups = a.n_steps / G;
    const uint32_t rem = a.n_steps - n_groups * G;
    double acc[kAutocallRecord] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (const uint64_t i : ThreadPaths{a.shard.n_local}) {
        const uint64_t subsequence = a.shard.path_offset + i;
        T X[D];                  // ln(S_j / S_{j,0}) so far, in exponent units
#pragma unroll
        for (int j = 0; j < D; ++j) X[j] = T(0);
        bool called = false, knocked = false;
        uint32_t q_call = 0;     // the date this path was called at
        double y_call = 0.0;     // and what it was paid there
        uint32_t q = 0;                          // dates behind the wavefront
        uint32_t next_obs = a.observe_every;     // the step that ends on date q + 1
        uint32_t steps_run = a.n_steps;
        Normals<T> nz;
        // the log of the worst performance, in exponent units
        auto worst = [&]() {
            T l = X[0];
#pragma unroll
            for (int j = 1; j < D; ++j) l = bk_min(l, X[j]);
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
                    const bool observe = g * G + s + 1 == next_obs;   // wave-uniform
                    if (KI_EVERY_STEP || observe) {
                        const T l = worst();
                        if (KI_EVERY_STEP) knocked = knocked || l <= a.log_ki;
                        if (observe) {
                            if (q + 1 >= a.first_call_date) {
                                const bool now = !called && l >= a.log_level[q];
                                y_call = now ? a.pay[q] : y_call;
                                q_call = now ? q + 1 : q_call;
                                called = called || now;
                            }
                            ++q;
                            next_obs += a.observe_every;
                        }
                    }
                }
            }
        };
        bool finished = true;
        for (uint32_t g = 0; g < n_groups; ++g) {
            group(g, G);
            if (__builtin_amdgcn_ballot_w64(!called) == 0) {
                steps_run = (g + 1) * G;
                finished = false;
                break;
            }
        }
        if (rem && finished) group(n_groups, rem);
        // A path never called: its worst performance at maturity, in fp64 from the path-precision logarithm.  A wavefront
        // that left early holds no such path, and its X are not those of maturity.
        double y = 1.0;
        if (finished) {
            const T l = worst();
            if (!KI_EVERY_STEP) knocked = a.ki != 0 && l <= a.log_ki;
            const double A = static_cast<double>(exp_of_logreturn(T(1), l, m));
            y = knocked ? (A < 1.0 ? A : 1.0) : 1.0;
        }
        // at date M the call test comes first: a called path is paid pay_q whatever its knock-in state
        y = called ? y_call : y;
        if (a.samples) a.samples[i] = static_cast<T>(y);
        const uint32_t s_call = q_call * a.observe_every;   // the step the path was called at
        add_sample(acc, y);
        acc[2] += called ? 1.0 : 0.0;
        acc[3] += called ? static_cast<double>(s_call) * a.dt : 0.0;
        acc[4] += (!called && knocked) ? 1.0 : 0.0;
        add_wave_steps(acc[5], steps_run);
        // the steps this path entered not yet called: all of them, or those up to its call
        acc[6] += static_cast<double>(called ? s_call : a.n_steps);
    }
    block_sumN<kBlock, kAutocallRecord>(acc);
    if (a.fin.n_value >= 0.0) {
        // the 6-double statistics layout has no slot for the two step counters: n takes the sixth
        double stats[6] = {acc[0], acc[1], acc[2], acc[3], acc[4], 0.0};
        grid_finish<kBlock, 6>(stats, partials, a.fin);
    } else {
        grid_finish<kBlock, kAutocallRecord>(acc, partials, a.fin);
    }
}

template <typename T, int D>
static hipError_t launch_autocall_d(const AutocallJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                    hipStream_t stream)
{
    const double u = exponent_unit<T>();   // natural log per exponent unit
    const AutocallSchedule &sc = j.schedule;
    AutocallArgs<T, D> a{};
    for (int q = 0; q < D; ++q) a.drift[q] = static_cast<T>(j.drift[q] / u);
    for (int c = 0; c < D * (D + 1) / 2; ++c) a.coef[c] = static_cast<T>(j.coef[c] / u);
    for (uint32_t q = 0; q < sc.n_dates; ++q) {
        a.log_level[q] = static_cast<T>(sc.log_level[q] / u);
        a.pay[q] = sc.pay[q];
    }
    a.log_ki = sc.ki ? static_cast<T>(sc.log_ki / u) : T(0);
    a.dt = sc.dt;
    a.ki = sc.ki ? 1 : 0;
    a.n_steps = j.path.n_sim;
    a.observe_every = sc.observe_every;
    a.first_call_date = sc.first_call_date;
    a.shard = shard_of(j.path);
    a.samples = static_cast<T *>(j.d_samples);
    a.fin = grid_finish_of(fs);
    const dim3 g(grid), b(kBlock);
    if (sc.ki && sc.ki_every_step) hipLaunchKernelGGL((autocall_kernel<T, D, true>), g, b, 0, stream, a, d_partials);
    else hipLaunchKernelGGL((autocall_kernel<T, D, false>), g, b, 0, stream, a, d_partials);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_autocall_t(const AutocallJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                    hipStream_t stream)
{
    return dispatch_assets(j.d, [&](auto d) {
        return launch_autocall_d<T, decltype(d)::value>(j, d_partials, grid, fs, stream);
    });
}

hipError_t launch_autocall(const AutocallJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                           hipStream_t stream)
{
    if (!finish_ok(finish, grid)) return hipErrorInvalidValue;
    if (!autocall_schedule_ok(job.schedule, job.path.n_sim)) return hipErrorInvalidValue;
    return dispatch_precision(job.path.precision, [&](auto p) {
        return launch_autocall_t<typename decltype(p)::type>(job, d_partials, grid, finish, stream);
    });
}

}  // namespace mcamd
