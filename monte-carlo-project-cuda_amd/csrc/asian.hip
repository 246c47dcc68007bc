// asian.hip — Asian (average-rate) options for gfx950 (both path precisions): arithmetic or geometric average over the
// step ends (and t = 0 with include_spot), fixed or floating strike, call or put, and the geometric average as the
// control variate of the arithmetic one.
//
// Definitions (include/mcamd.h, mcamd_price_asian): x_i is the step exponent of Exponents<T>, X_i = X_{i-1} + x_i.
// Arithmetic: P_0 = S0, P_i = P_{i-1} e^{x_i} through PathState<T> — the bits mcamd_simulate_trajectories stores —
// summed in fp64 in ascending i; A = sum / m, S_T = P_n.  Geometric: L = sum_i X_i in the path precision,
// G = exp_of_logreturn(S0, L / m), S_T = exp_of_logreturn(S0, X_n): no exponential inside the step loop.
//
// The loop is walk_steps (mc_device.hpp): per Philox block one Exponents<T>::fill; per step, geometric: two adds;
// arithmetic: one PathState<T> step (the exponential of the step is what the product costs), in fp32 one widening, and
// one fp64 add.  The controlled job (ARITH and GEO) does both on the same exponents.  Strike type, payoff and
// include_spot are wave-uniform selects outside the step loop.
#include "asian.hpp"
#include "path_consts.hpp"
#include "path_frame.hpp"

namespace mcamd {

template <typename T>
struct AsianArgs {
    StepConsts<T> c;     // drift, vol, S_start, n_sim in exponent units (K, B, logB unused)
    T inv_m;             // 1 / m, m = n_steps + include_spot averaging dates, narrowed once on the host
    double m;            // m itself: the arithmetic average divides in fp64
    double K;            // fixed strike
    double control_mean; // E[g] (ARITH and GEO)
    int floating, put, include_spot;
    PathShard shard;
    T *samples;          // nullable
    GridFinish fin;
};

template <typename T, bool ARITH, bool GEO>
__global__ __launch_bounds__(kBlock) void asian_kernel(AsianArgs<T> a, double *__restrict__ partials)
{
    static_assert(ARITH || GEO, "an Asian kernel averages something");
    constexpr int NB = Exponents<T>::kPerBlock;
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    const StepConsts<T> c = resident(a.c);
    const StepBlocks blocks = step_blocks<NB>(c.n_sim);
    // one sample from an average and a terminal price, both already fp64
    auto sample = [&](double avg, double St) {
        const double d = a.floating ? (a.put ? avg - St : St - avg) : (a.put ? a.K - avg : avg - a.K);
        return d > 0.0 ? d : 0.0;
    };
    double acc6[kAsianRecord] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (const uint64_t i : ThreadPaths{a.shard.n_local}) {
        const uint64_t subsequence = a.shard.path_offset + i;
        PathState<T> ps = PathState<T>::start(c.S_start);                               // ARITH: P_i
        double sum_p = a.include_spot ? static_cast<double>(c.S_start) : 0.0;           // ARITH: P_0 + .. + P_i
        T X = T(0);                                                                     // GEO: X_i, exponent units
        T L = T(0);                                                                     // GEO: X_1 + .. + X_i
        Exponents<T> ex;
        auto step = [&](T x) {
            if (ARITH) {
                ps.step(x, m);
                sum_p += static_cast<double>(ps.value(m));
            }
            if (GEO) {
                X += x;
                L += X;
            }
        };
        walk_steps<NB>(
            blocks, [&](uint32_t k) { ex.fill(m, c, key, subsequence, k); }, [&](uint32_t, int j) { step(ex.x[j]); });
        double y, g = 0.0;
        if (GEO) {
            // the same routine for both prices: one step without the spot has L / m == X bit for bit, so G == S_T
            const double St = static_cast<double>(exp_of_logreturn(c.S_start, X, m));
            const double G = static_cast<double>(exp_of_logreturn(c.S_start, L * a.inv_m, m));
            g = sample(G, St);
        }
        if (ARITH) y = sample(sum_p / a.m, static_cast<double>(ps.value(m)));
        else y = g;
        if (a.samples) a.samples[i] = static_cast<T>(y);
        add_sample(acc6, y);
        if (ARITH && GEO) {
            const double ctl = g - a.control_mean;
            acc6[2] += ctl;
            acc6[3] = __builtin_fma(ctl, ctl, acc6[3]);
            acc6[4] = __builtin_fma(y, ctl, acc6[4]);
        }
        add_wave_steps(acc6[5], c.n_sim);
    }
    finish_paths(acc6, partials, a.fin);   // the statistics layout puts n where the counter is
}

template <typename T>
static hipError_t launch_asian_t(const AsianJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                 hipStream_t stream)
{
    const double dates = static_cast<double>(j.path.n_sim) + (j.include_spot ? 1.0 : 0.0);
    const AsianArgs<T> a{make_consts<T>(j.path), static_cast<T>(1.0 / dates), dates, j.K, j.control_mean,
                         j.floating ? 1 : 0, j.put ? 1 : 0, j.include_spot ? 1 : 0, shard_of(j.path),
                         static_cast<T *>(j.d_samples), grid_finish_of(fs)};
    const dim3 g(grid), b(kBlock);
    if (!j.arithmetic) hipLaunchKernelGGL((asian_kernel<T, false, true>), g, b, 0, stream, a, d_partials);
    else if (j.control) hipLaunchKernelGGL((asian_kernel<T, true, true>), g, b, 0, stream, a, d_partials);
    else hipLaunchKernelGGL((asian_kernel<T, true, false>), g, b, 0, stream, a, d_partials);
    return hipGetLastError();
}

hipError_t launch_asian(const AsianJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                        hipStream_t stream)
{
    if (!finish_ok(finish, grid)) return hipErrorInvalidValue;
    return dispatch_precision(job.path.precision, [&](auto p) {
        return launch_asian_t<typename decltype(p)::type>(job, d_partials, grid, finish, stream);
    });
}

}  // namespace mcamd
