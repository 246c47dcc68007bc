// barrier.hip — single-barrier options for gfx950 (both path precisions): down / up, knock-out / knock-in, call / put,
// monitored at the step ends (discrete) or all the time (continuous, by the Brownian-bridge survival weight).
//
// Definitions: barrier_device.hpp, with the constant volatility v in the bridge factor and X, b in exponent units.
//
// The loop is walk_steps (mc_device.hpp) on the log-space window step of simulate_sample: per Philox block one
// Exponents<T>::fill, per step acc += x, one subtract for d, the strict compare.  The bridge factor costs one
// multiply-multiply-compare per step and an exponential only where a live lane has q < Q; that skip is decided per
// wavefront (one ballot), and paths spend most of their steps far from the barrier.  A knock-out wavefront leaves the
// step loop at the first block end where every lane is knocked; a knock-in runs to maturity, because it needs S_T.
#include "barrier.hpp"
#include "barrier_device.hpp"
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
        const T h = vanilla_payoff(a.put, c.K, St);
        const double wd = alive ? static_cast<double>(w) : 0.0;
        const double y = barrier_sample<OUT>(alive, wd, h);
        if (a.samples) a.samples[i] = static_cast<T>(y);
        add_sample(acc4, y);
        add_counters(acc4, steps_run, live);
    }
    if (a.fin.n_value >= 0.0) acc4[2] = acc4[3] = 0.0;   // the 6-double statistics layout has no slot for the counters
    finish_paths(acc4, partials, a.fin);
}

template <typename T>
static hipError_t launch_barrier_t(const BarrierJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                   hipStream_t stream)
{
    const double u = exponent_unit<T>();
    const BridgeUnits bu = bridge_units<T>();
    const BarrierArgs<T> a{make_consts<T>(j.path), static_cast<T>(j.kq * u * u / bu.q_unit), static_cast<T>(bu.q_cut),
                           j.form.put ? 1 : 0, shard_of(j.path), static_cast<T *>(j.d_samples), grid_finish_of(fs)};
    dispatch_barrier_form(j.form, [&](auto up, auto cont, auto out) {
        hipLaunchKernelGGL((barrier_kernel<T, decltype(up)::value, decltype(cont)::value, decltype(out)::value>),
                           dim3(grid), dim3(kBlock), 0, stream, a, d_partials);
    });
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
