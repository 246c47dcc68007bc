// localvol.hip — European and single-barrier options under a local-volatility surface, for gfx950 (both path precisions).
//
// Definitions (include/mcamd.h, mcamd_price_localvol): X_i = ln(S_i / S0) in NATURAL-log units (the surface's axis);
// the lookup of the step's volatility s, the row carry and the move X += ((r - q) - s^2/2) dt + s sqrt(dt) z are
// localvol_device.hpp's, which the smile and the autocallable kernels walk as well.  The barrier tests, distances,
// survival weight and samples are barrier_device.hpp's with b = ln(B / S0) in natural units and the step's own s in
// the bridge factor, q_i = 2 d d' / (s^2 dt).
//
// The table — n_t n_x (sigma_k, slope_k) pairs of the path precision — is copied from global memory into dynamic LDS
// once per workgroup; a step then costs one ds_read_b64 (fp32) / ds_read_b128 (fp64) per lane at a wave-uniform row
// base plus the lane's k, and FMAs.  The volatility differs per lane and per step, so the exponent cannot be pre-scaled
// as Exponents<T> does: the loop takes plain normals (Normals<T>) and converts X to the exponential's unit once, at the
// end of the path.
#include "barrier_device.hpp"
#include "localvol_device.hpp"
#include "path_frame.hpp"

namespace mcamd {

template <typename T>
struct LocalVolArgs {
    LvSurface<T> surf;
    T mu_dt, half_dt, sqrt_dt;
    T exp_scale;              // exponent units per natural-log unit (log2 e in fp32, 65536 / ln 2 in fp64)
    T b;                      // ln(B / S0)
    T kq;                     // 2 / dt, in the unit bridge_factor's exponential takes (fp32: times log2 e)
    T q_cut;                  // Q in the same unit
    T K, S0;
    int put;
    uint32_t n_steps;
    PathShard shard;
    T *samples;               // nullable
    GridFinish fin;
};

// BAR: 0 no barrier, 1 down, 2 up.  CONT and OUT are read with a barrier only.
template <typename T, int BAR, bool CONT, bool OUT>
__global__ __launch_bounds__(kBlock) void localvol_kernel(LocalVolArgs<T> a, double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    constexpr bool UP = BAR == 2;
    VolPair<T> *tab = reinterpret_cast<VolPair<T> *>(lv_table_lds);
    lv_copy_table(tab, 0, a.surf.table, a.surf.rows.n_entries);
    __syncthreads();
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    const LvAxis<T> axis = lv_resident(a.surf.axis);
    const T mu_dt = resident_t(a.mu_dt), half_dt = resident_t(a.half_dt), sqrt_dt = resident_t(a.sqrt_dt);
    const ThreadPaths paths(a.shard.n_local);   // made at the loop, one fp64 kernel spills 8 scalars for 4
    const StepBlocks blocks = step_blocks<NB>(a.n_steps);
    const T d0 = UP ? a.b : -a.b;   // |b|: the spot is strictly on the live side (checked on the host)
    double acc4[kLocalVolRecord] = {0.0, 0.0, 0.0, 0.0};
    for (const uint64_t i : paths) {
        const uint64_t subsequence = a.shard.path_offset + i;
        T X = T(0);          // ln(S / S0), natural units
        T d_prev = d0;
        T w = T(1);          // the bridge factors so far (CONT); the hits are in `alive`
        bool alive = true;
        uint32_t live = 0;   // steps this path entered not yet knocked
        LvRow row{0, 0};
        Normals<T> nz;
        auto step = [&](T z) {
            live += alive ? 1u : 0u;
            const T s = lv_sigma(X, axis, a.surf.rows, tab, row);
            const T s2 = lv_move(X, s, z, sqrt_dt, half_dt, mu_dt);
            if (BAR != 0) {
                const T d = UP ? a.b - X : X - a.b;
                const bool hit = UP ? (X > a.b) : (a.b > X);
                alive = alive && !hit;
                if (CONT) {
                    const T num = a.kq * d_prev * d;   // q s^2
                    const bool close_by = alive && (num < a.q_cut * s2);
                    if (__builtin_amdgcn_ballot_w64(close_by) != 0) {   // wave-uniform: most steps take no exponential
                        const T fac = bridge_factor(num / s2, m);
                        w = close_by ? w * fac : w;
                    }
                    d_prev = d;
                }
            }
        };
        const uint32_t steps_run = walk_steps<NB>(
            blocks, [&](uint32_t kb) { nz.fill(m, key, subsequence, kb); }, [&](uint32_t, int j) { step(nz.z[j]); },
            [&] { return BAR != 0 && OUT && __builtin_amdgcn_ballot_w64(alive) == 0; });
        const T St = exp_of_logreturn(a.S0, X * a.exp_scale, m);
        const T h = vanilla_payoff(a.put, a.K, St);
        double y;
        if (BAR == 0) {
            y = static_cast<double>(h);
        } else {
            const double wd = alive ? static_cast<double>(w) : 0.0;
            y = barrier_sample<OUT>(alive, wd, h);
        }
        if (a.samples) a.samples[i] = static_cast<T>(y);
        add_sample(acc4, y);
        add_counters(acc4, steps_run, live);
    }
    if (a.fin.n_value >= 0.0) acc4[2] = acc4[3] = 0.0;   // the 6-double statistics layout has no slot for the counters
    finish_paths(acc4, partials, a.fin);
}

template <typename T, int BAR, bool CONT, bool OUT>
static void launch_localvol_k(const LocalVolArgs<T> &a, double *d_partials, uint32_t grid, hipStream_t stream)
{
    const size_t lds_bytes = static_cast<size_t>(a.surf.rows.n_entries) * sizeof(VolPair<T>);
    hipLaunchKernelGGL((localvol_kernel<T, BAR, CONT, OUT>), dim3(grid), dim3(kBlock), lds_bytes, stream, a, d_partials);
}

template <typename T>
static hipError_t launch_localvol_t(const LocalVolJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                    hipStream_t stream)
{
    const BridgeUnits bu = bridge_units<T>();
    LocalVolArgs<T> a;
    lv_step_args<T>(a, j.walk);
    a.shard = shard_of(j.walk.paths);
    a.b = j.barrier ? static_cast<T>(std::log(j.B / j.S0)) : T(0);
    a.kq = static_cast<T>(2.0 / (j.walk.dt * bu.q_unit));
    a.q_cut = static_cast<T>(bu.q_cut);
    a.K = static_cast<T>(j.K);
    a.S0 = static_cast<T>(j.S0);
    a.put = j.form.put ? 1 : 0;
    a.n_steps = j.walk.paths.n_steps;
    a.samples = static_cast<T *>(j.d_samples);
    a.fin = grid_finish_of(fs);
    if (!j.barrier) {
        launch_localvol_k<T, 0, false, false>(a, d_partials, grid, stream);
    } else {
        dispatch_barrier_form(j.form, [&](auto up, auto cont, auto out) {
            launch_localvol_k<T, decltype(up)::value ? 2 : 1, decltype(cont)::value, decltype(out)::value>(
                a, d_partials, grid, stream);
        });
    }
    return hipGetLastError();
}

hipError_t launch_localvol(const LocalVolJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                           hipStream_t stream)
{
    if (!finish_ok(finish, grid)) return hipErrorInvalidValue;
    if (!lv_grid_ok(job.walk.surface, job.walk.paths.n_steps)) return hipErrorInvalidValue;
    return dispatch_precision(job.walk.paths.precision, [&](auto p) {
        return launch_localvol_t<typename decltype(p)::type>(job, d_partials, grid, finish, stream);
    });
}

}  // namespace mcamd
