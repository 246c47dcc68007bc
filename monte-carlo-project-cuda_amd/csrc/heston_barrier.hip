// heston_barrier.hip — single-barrier options under Heston stochastic volatility, full-truncation Euler in the
// log-price, for gfx950 (both path precisions).
//
// Definitions (include/mcamd.h, mcamd_price_heston_barrier): the path is mcamd_price_heston's, X_i = ln(S_i / S0) in
// NATURAL-log units and the raw variance v_i, moved by heston_device.hpp's heston_move on the two normals of heston.hip
// (z of Philox blocks 0, 1, .., z' of blocks 2^63, 2^63 + 1, .. of the path's subsequence).  The barrier tests,
// distances, survival weight and samples are barrier_device.hpp's for a volatility that changes from step to step, as
// in localvol.hip: b = ln(B / S0) in natural units and, in the bridge factor, the variance v+ the step was taken at
// (what heston_move returns), q_i = 2 d d' / (v+ dt).  The scheme freezes v+ over a step, so the bridge between
// two step ends is Brownian with that variance rate and the factor is its exact survival probability.
//
// The factor is taken iff kq d d' < q_cut v+ (division-free, in the path precision): a step taken at v+ = 0 takes none
// and divides nothing, it moves along a straight line and the end-point test decides.  A wave-uniform ballot skips the
// exponential and the division on steps where no live lane is near the level, which is most of them.
//
// A knock-out wavefront leaves the walk at the first Philox-block end where every lane is knocked (walk_steps' exit
// predicate); a knock-in runs to maturity.  Beside the sample a path leaves the steps it entered not yet hit (live),
// and over the steps that count — all of them for a knock-in, the live ones for a knock-out — the steps entered with
// v < 0 and the sum of v+ (in the path precision, in step order).  All of these depend on the path's global id alone.
// Put / call is a wave-uniform select after the walk.  There is no table in LDS beyond what MathCtx<T> needs.
#include "heston_barrier.hpp"
#include "barrier_device.hpp"
#include "heston_device.hpp"
#include "path_consts.hpp"
#include "path_frame.hpp"

namespace mcamd {

template <typename T>
struct HestonBarrierArgs {
    HestonConsts<T> c;
    T exp_scale;              // exponent units per natural-log unit (log2 e in fp32, 65536 / ln 2 in fp64)
    T v0;
    T b;                      // ln(B / S0)
    T kq;                     // 2 / dt, in the unit bridge_factor's exponential takes (fp32: times log2 e)
    T q_cut;                  // Q in the same unit
    T K, S0;
    int put;
    uint32_t n_steps;
    PathShard shard;
    T *samples;               // nullable
    T *state;                 // nullable: S_T at [i], v_n at [n_local + i], w at [2 n_local + i]
    GridFinish fin;
};

template <typename T, bool UP, bool CONT, bool OUT>
__global__ __launch_bounds__(kBlock) void heston_barrier_kernel(HestonBarrierArgs<T> a, double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    const HestonConsts<T> c = heston_resident(a.c);
    // the barrier's three constants live as heston_resident keeps the step's
    const T b = resident_t(a.b), kq = resident_t(a.kq), q_cut = resident_t(a.q_cut);
    const StepBlocks blocks = step_blocks<NB>(a.n_steps);
    const T d0 = UP ? b : -b;   // |b|: the spot is strictly on the live side (checked on the host)
    double acc6[kHestonBarrierRecord] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (const uint64_t i : ThreadPaths{a.shard.n_local}) {
        const uint64_t subsequence = a.shard.path_offset + i;
        T X = T(0);           // ln(S / S0), natural units
        T v = a.v0;           // the raw variance
        T d_prev = d0;
        T w = T(1);           // the bridge factors so far (CONT); the hits are in `alive`
        T v_sum = T(0);       // sum of v+ over the counted steps
        bool alive = true;
        uint32_t live = 0;    // steps this path entered not yet knocked
        uint32_t trunc = 0;   // counted steps entered with v < 0
        HestonNormals<T> nz;
        auto step = [&](T z, T zv) {
            const bool counted = OUT ? alive : true;   // a knock-out's diagnostics stop where its walk may
            live += alive ? 1u : 0u;
            trunc += (counted && v < T(0)) ? 1u : 0u;
            const T vp = heston_move(X, v, z, zv, c);
            v_sum += counted ? vp : T(0);
            const T d = UP ? b - X : X - b;
            const bool hit = UP ? (X > b) : (b > X);
            alive = alive && !hit;
            if (CONT) {
                const T num = kq * d_prev * d;   // q v+
                const bool close_by = alive && (num < q_cut * vp);   // never at v+ = 0: num >= 0 on a live path
                if (__builtin_amdgcn_ballot_w64(close_by) != 0) {    // wave-uniform: most steps take no exponential
                    const T fac = bridge_factor(num / vp, m);
                    w = close_by ? w * fac : w;
                }
                d_prev = d;
            }
        };
        const uint32_t steps_run = walk_steps<NB>(
            blocks, [&](uint32_t kb) { nz.fill(m, key, subsequence, kb); },
            [&](uint32_t, int j) { step(nz.z.z[j], nz.zv.z[j]); },
            [&] { return OUT && __builtin_amdgcn_ballot_w64(alive) == 0; });
        const T St = exp_of_logreturn(a.S0, X * a.exp_scale, m);
        const T h = vanilla_payoff(a.put, a.K, St);
        const T w_end = alive ? w : T(0);
        const double wd = static_cast<double>(w_end);
        const double y = barrier_sample<OUT>(alive, wd, h);
        if (a.samples) a.samples[i] = static_cast<T>(y);
        if (a.state) {
            // where a knocked knock-out path stops depends on its wavefront's other lanes: nothing is defined there
            const bool defined = !OUT || alive;
            const T nan = static_cast<T>(__builtin_nan(""));
            a.state[i] = defined ? St : nan;
            a.state[a.shard.n_local + i] = defined ? v : nan;
            a.state[2 * a.shard.n_local + i] = w_end;
        }
        add_sample(acc6, y);
        acc6[2] += static_cast<double>(live);
        acc6[3] += static_cast<double>(trunc);
        acc6[4] += static_cast<double>(v_sum);
        add_wave_steps(acc6[5], steps_run);
    }
    finish_paths(acc6, partials, a.fin);
}

template <typename T>
static hipError_t launch_heston_barrier_t(const HestonBarrierJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                          hipStream_t stream)
{
    const BridgeUnits bu = bridge_units<T>();
    HestonBarrierArgs<T> a;
    heston_walk_args<T>(a, j.walk);
    a.b = static_cast<T>(std::log(j.B / j.S0));
    a.kq = static_cast<T>(2.0 / (j.walk.dt * bu.q_unit));
    a.q_cut = static_cast<T>(bu.q_cut);
    a.K = static_cast<T>(j.K);
    a.S0 = static_cast<T>(j.S0);
    a.put = j.form.put ? 1 : 0;
    a.n_steps = j.walk.paths.n_steps;
    a.samples = static_cast<T *>(j.d_samples);
    a.state = static_cast<T *>(j.d_state);
    a.fin = grid_finish_of(fs);
    dispatch_barrier_form(j.form, [&](auto up, auto cont, auto out) {
        hipLaunchKernelGGL((heston_barrier_kernel<T, decltype(up)::value, decltype(cont)::value, decltype(out)::value>),
                           dim3(grid), dim3(kBlock), 0, stream, a, d_partials);
    });
    return hipGetLastError();
}

hipError_t launch_heston_barrier(const HestonBarrierJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                                 hipStream_t stream)
{
    if (!finish_ok(finish, grid)) return hipErrorInvalidValue;
    if (!heston_walk_ok(job.walk)) return hipErrorInvalidValue;
    if (!(job.B > 0.0) || !(job.S0 > 0.0) || !(job.form.up ? job.S0 < job.B : job.S0 > job.B)) return hipErrorInvalidValue;
    return dispatch_precision(job.walk.paths.precision, [&](auto p) {
        return launch_heston_barrier_t<typename decltype(p)::type>(job, d_partials, grid, finish, stream);
    });
}

}  // namespace mcamd
