// barrier.hip — single-barrier options for gfx950 (both path precisions): down / up, knock-out / knock-in, call / put,
// monitored at the step ends (discrete) or all the time (continuous, by the Brownian-bridge survival weight).
//
// Definitions (include/mcamd.h, mcamd_price_barrier): X_i = ln(S_i / S0) after step i, b = ln(B / S0); a path is hit at
// step end i when b > X_i (down) or X_i > b (up); d_i = X_i - b (down) or b - X_i (up), d_0 = |b|.  The survival weight
// w is the product over the steps of 1{no hit at i} and — continuous monitoring — of f_i = 1 - exp(-q_i) with
// q_i = 2 d_{i-1} d_i / (v^2 dt), where f_i is DEFINED as 1 for q_i >= Q (Q = 38 in fp64, 18 in fp32: there
// exp(-q) < 2^-54 / 2^-25 and 1 - exp(-q) rounds to 1 anyway).  The sample is w h(S_T) (knock-out) or (1 - w) h(S_T)
// (knock-in), formed once per path in fp64.
//
// The loop is walk_steps (mc_device.hpp) on the log-space window step of simulate_sample: per Philox block one
// Exponents<T>::fill, per step acc += x, one subtract for d, the strict compare.  The bridge factor costs one
// multiply-multiply-compare per step and an exponential only where a live lane has q < Q; that skip is decided per
// wavefront (one ballot), and paths spend most of their steps far from the barrier.  A knock-out wavefront leaves the
// step loop at the first block end where every lane is knocked; a knock-in runs to maturity, because it needs S_T.
#include "barrier.hpp"
#include "path_consts.hpp"
#include "path_frame.hpp"

namespace mcamd {

template <typename T>
struct BarrierArgs {
    StepConsts<T> c;   // logB = b in exponent units; K, S_start, drift, vol, n_sim
    T kq;              // fp64: 2 u^2 / (v^2 dt), u = ln 2 / 65536: q = kq d d' in natural-log units (f64::mul_exp's)
                       // fp32: 2 ln 2 / (v^2 dt): q = kq d d' in log2 units (v_exp_f32's)
    T q_cut;           // Q in the units of q
    int put;
    PathShard shard;
    T *samples;        // nullable
    GridFinish fin;
};

template <typename T, bool UP, bool CONT, bool OUT>
__global__ __launch_bounds__(kBlock) void barrier_kernel(BarrierArgs<T> a, double *__restrict__ partials)
{
    constexpr int NB = Exponents<T>::kPerBlock;
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    const StepConsts<T> c = resident(a.c);
    const StepBlocks blocks = step_blocks<NB>(c.n_sim);
    const T d0 = UP ? c.logB : -c.logB;   // |b|: the spot is strictly on the live side (checked on the host)
    double acc4[kBarrierRecord] = {0.0, 0.0, 0.0, 0.0};
    for (const uint64_t i : ThreadPaths{a.shard.n_local}) {
        const uint64_t subsequence = a.shard.path_offset + i;
        T acc = T(0);        // X so far, in exponent units
        T d_prev = d0;
        T w = T(1);          // the bridge factors so far (CONT); the hits are in `alive`
        bool alive = true;
        uint32_t live = 0;   // steps this path entered not yet knocked
        Exponents<T> ex;
        auto step = [&](T x) {
            live += alive ? 1u : 0u;
            acc += x;
            const T d = UP ? c.logB - acc : acc - c.logB;
            const bool hit = UP ? (acc > c.logB) : (c.logB > acc);
            alive = alive && !hit;
            if (CONT) {
                const T q = a.kq * d_prev * d;
                const bool close_by = alive && (q < a.q_cut);
                if (__builtin_amdgcn_ballot_w64(close_by) != 0) {   // wave-uniform: most steps take no exponential at all
                    const T f = bridge_factor(q, m);
                    w = close_by ? w * f : w;
                }
                d_prev = d;
            }
        };
        const uint32_t steps_run = walk_steps<NB>(
            blocks, [&](uint32_t k) { ex.fill(m, c, key, subsequence, k); }, [&](uint32_t, int j) { step(ex.x[j]); },
            [&] { return OUT && __builtin_amdgcn_ballot_w64(alive) == 0; });
        const T St = exp_of_logreturn(c.S_start, acc, m);
        T h = a.put ? c.K - St : St - c.K;
        h = h > T(0) ? h : T(0);
        const double wd = alive ? static_cast<double>(w) : 0.0;
        // a knocked path of a knock-out pays 0 whatever its (possibly unfinished) price is
        const double y = OUT ? (alive ? wd * static_cast<double>(h) : 0.0) : (1.0 - wd) * static_cast<double>(h);
        if (a.samples) a.samples[i] = static_cast<T>(y);
        add_sample(acc4, y);
        add_counters(acc4, steps_run, live);
    }
    if (a.fin.n_value >= 0.0) acc4[2] = acc4[3] = 0.0;   // the 6-double statistics layout has no slot for the counters
    finish_paths(acc4, partials, a.fin);
}

template <typename T, bool UP, bool CONT>
static void launch_barrier_k(const BarrierJob &j, const BarrierArgs<T> &a, double *d_partials, uint32_t grid,
                             hipStream_t stream)
{
    const dim3 g(grid), b(kBlock);
    if (j.out) hipLaunchKernelGGL((barrier_kernel<T, UP, CONT, true>), g, b, 0, stream, a, d_partials);
    else hipLaunchKernelGGL((barrier_kernel<T, UP, CONT, false>), g, b, 0, stream, a, d_partials);
}

template <typename T>
static hipError_t launch_barrier_t(const BarrierJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                   hipStream_t stream)
{
    const double u = exponent_unit<T>();   // and the natural log per unit of q:
    const double q_unit = sizeof(T) == 4 ? kLn2 : 1.0;
    const double q_cut = sizeof(T) == 4 ? 18.0 : 38.0;
    const BarrierArgs<T> a{make_consts<T>(j.path), static_cast<T>(j.kq * u * u / q_unit), static_cast<T>(q_cut / q_unit),
                           j.put ? 1 : 0, shard_of(j.path), static_cast<T *>(j.d_samples), grid_finish_of(fs)};
    if (j.up) {
        if (j.continuous) launch_barrier_k<T, true, true>(j, a, d_partials, grid, stream);
        else launch_barrier_k<T, true, false>(j, a, d_partials, grid, stream);
    } else {
        if (j.continuous) launch_barrier_k<T, false, true>(j, a, d_partials, grid, stream);
        else launch_barrier_k<T, false, false>(j, a, d_partials, grid, stream);
    }
    return hipGetLastError();
}

hipError_t launch_barrier(const BarrierJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                          hipStream_t stream)
{
    if (!finish_ok(finish, grid)) return hipErrorInvalidValue;
    return dispatch_precision(job.path.precision, [&](auto p) {
        return launch_barrier_t<typename decltype(p)::type>(job, d_partials, grid, finish, stream);
    });
}

}  // namespace mcamd
