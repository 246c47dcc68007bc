// autocall_localvol_impl.hpp — the worst-of autocallable kernel under per-asset local-volatility surfaces, for gfx950.
// Included by autocall_localvol.hip (fp64) and autocall_localvol_f32.hip (fp32), which instantiate D = 1..8 each.
//
// Definitions (include/mcamd.h, mcamd_price_autocall_localvol): X_{j,i} = ln(S_{j,i} / S_{j,0}) in NATURAL-log units.
// Step i looks asset j's volatility s_j up at X_j in row_j(i) = floor(i n_t,j / n) of asset j's surface
// (localvol_device.hpp's lookup and row carry, which localvol.hip walks as well), forms
// w_j = sum_{k <= j} l_jk z_{i,k} as a chain of fused multiply-adds in ascending k from 0 (z_{i,k} normal number
// i d + k of the path's stream, as basket.hip draws it) and moves
// X_j += fma(s_j sqrt(dt), w_j, fma(-s_j^2, dt / 2, (r - q_j) dt)): localvol_device.hpp's move with w_j in the place of z.
// l_i = min_j X_{j,i}.  Dates, levels, payments, the call test, the knock-in modes, the sample and the block record are
// those of autocall.hip, with ln L_q and ln ki_level in natural-log units; A_n = exp_of_logreturn(1, l_n exp_scale).
//
// The loop is written as autocall.hip's is (groups of G = NB / gcd(D, NB) steps on whole Philox blocks, unrolled with
// the block boundaries at compile-time positions; a wave-uniform observation test and date counter; a wavefront leaves
// at the first group end where no lane is uncalled) and keeps the note's state as that kernel does.  Each was tried in
// one place for both kernels: with one group walk or one note, kernels of this file compiled to other vector
// instructions or crossed an occupancy step, and with one function for the chain of fused multiply-adds the fp64
// kernel of D = 8 without a step-wise knock-in spilled 11 more scalars and ran 2.8 % slower (profiles/README.md, "One
// schedule for two autocall calls; one walk for three kernels, tried").  The lookup, the row carry and the move are
// localvol_device.hpp's, one per asset.  The D pair tables lie back to back in dynamic LDS, copied once per workgroup;
// a step costs D reads (ds_read_b64 in fp32, ds_read_b128 in fp64) at asset j's row base — which starts at the
// table's own base — plus the lane's k_j.  The per-asset grid constants and the row carries are wave-uniform (scalar
// unit).
#pragma once

#include "autocall_localvol.hpp"
#include "localvol_device.hpp"
#include "basket_device.hpp"
#include "path_frame.hpp"

namespace mcamd {

template <typename T, int D>
struct AutocallLocalVolArgs {
    // The D surfaces field by field (LvSurface's fields, asset j's at [j]), in the order the kernels were tuned with:
    // where a field lies among the kernel's arguments decides which scalar registers the compiler spills at D >= 3,
    // and an array of LvSurface moved up to 140 spills and put scratch into the fp64 kernels of D = 4, 6 and 8.
    T x_min[D], inv_dx[D], u_max[D];
    T mu_dt[D];                      // (r - q_j) dt
    T chol[D * (D + 1) / 2];         // l_jk at [j (j + 1) / 2 + k]
    uint32_t k_max[D], n_x[D];
    uint32_t base[D];                // where asset j's table starts in LDS, in entries
    uint32_t n_entries[D], row_whole_nx[D], row_rem[D], row_thr[D];
    const VolPair<T> *table[D];
    __device__ LvAxis<T> axis(int j) const { return {x_min[j], inv_dx[j], u_max[j]}; }
    __device__ LvRows rows(int j) const
    {
        return {k_max[j], n_x[j], n_entries[j], row_whole_nx[j], row_rem[j], row_thr[j]};
    }
    T half_dt, sqrt_dt;
    T exp_scale;                     // exponent units per natural-log unit (log2 e in fp32, 65536 / ln 2 in fp64)
    T log_level[kAutocallMaxDates];  // ln L_q at [q - 1]
    T log_ki;                        // ln ki_level
    double pay[kAutocallMaxDates];   // pay_q at [q - 1]
    double dt;
    int ki;                          // a knock-in applies (always, with KI_EVERY_STEP)
    uint32_t n_steps, observe_every, first_call_date;
    PathShard shard;
    T *samples;                      // nullable
    GridFinish fin;
};

// Where the step's floating-point constants live: the per-asset grid constants and drifts follow resident_t (vector
// registers in fp32 only); the D (D + 1) / 2 entries of the Cholesky factor follow basket_device.hpp's bk_resident
// (vector registers in fp32, and in fp64 from D = 3): left scalar they do not fit beside the kernel's other scalars and
// are read back one v_readlane at a time inside the step, which measured 5 % (D = 3) and 7 % (D = 8) slower on the
// benchmark note.
template <typename T, int D, bool KI_EVERY_STEP>
__global__ __launch_bounds__(kBlock) void autocall_localvol_kernel(AutocallLocalVolArgs<T, D> a,
                                                                   double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    constexpr int G = NB / gcd_c(D, NB);   // steps that consume whole blocks
    constexpr int BPG = G * D / NB;        // the blocks they consume
    constexpr int NC = D * (D + 1) / 2;
    VolPair<T> *tab = reinterpret_cast<VolPair<T> *>(lv_table_lds);
#pragma unroll
    for (int j = 0; j < D; ++j) lv_copy_table(tab, a.base[j], a.table[j], a.n_entries[j]);
    __syncthreads();
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    LvAxis<T> axis[D];
    T mu_dt[D], chol[NC];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        axis[j] = lv_resident(a.axis(j));
        mu_dt[j] = resident_t(a.mu_dt[j]);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) chol[c] = bk_resident<D>(a.chol[c]);
    const T half_dt = resident_t(a.half_dt), sqrt_dt = resident_t(a.sqrt_dt);
    const uint32_t n_groups = a.n_steps / G;
    const uint32_t rem = a.n_steps - n_groups * G;
    double acc[kAutocallRecord] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (const uint64_t i : ThreadPaths{a.shard.n_local}) {
        const uint64_t subsequence = a.shard.path_offset + i;
        T X[D];                  // ln(S_j / S_{j,0}) so far, natural units
        LvRow row[D];            // asset j's starts at its table's own base
#pragma unroll
        for (int j = 0; j < D; ++j) {
            X[j] = T(0);
            row[j] = LvRow{a.base[j], 0};
        }
        bool called = false, knocked = false;
        uint32_t q_call = 0;     // the date this path was called at
        double y_call = 0.0;     // and what it was paid there
        uint32_t q = 0;                          // dates behind the wavefront
        uint32_t next_obs = a.observe_every;     // the step that ends on date q + 1
        uint32_t steps_run = a.n_steps;
        Normals<T> nz;
        // the log of the worst performance
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
                    // the D volatilities of the step, each at its own asset's X in its own table
                    T sig[D];
#pragma unroll
                    for (int j = 0; j < D; ++j) sig[j] = lv_sigma(X[j], axis[j], a.rows(j), tab, row[j]);
                    T w[D];
#pragma unroll
                    for (int j = 0; j < D; ++j) w[j] = T(0);
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        const int flat = s * D + k;   // a compile-time position once unrolled
                        if (flat % NB == 0) nz.fill(m, key, subsequence, first_block + flat / NB);
                        const T z = nz.z[flat % NB];
#pragma unroll
                        for (int j = k; j < D; ++j) w[j] = fma_t(chol[j * (j + 1) / 2 + k], z, w[j]);
                    }
#pragma unroll
                    for (int j = 0; j < D; ++j) lv_move(X[j], sig[j], w[j], sqrt_dt, half_dt, mu_dt[j]);
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
            const double A = static_cast<double>(exp_of_logreturn(T(1), l * a.exp_scale, m));
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
static hipError_t launch_autocall_localvol_d(const AutocallLocalVolJob &j, double *d_partials, uint32_t grid,
                                             const FinishSpec &fs, hipStream_t stream)
{
    const AutocallSchedule &sc = j.schedule;
    AutocallLocalVolArgs<T, D> a{};
    uint32_t total = 0;
    for (int q = 0; q < D; ++q) {
        const LvSurface<T> s = lv_surface<T>(j.surface[q], j.paths.n_steps);
        a.x_min[q] = s.axis.x_min;
        a.inv_dx[q] = s.axis.inv_dx;
        a.u_max[q] = s.axis.u_max;
        a.k_max[q] = s.rows.k_max;
        a.n_x[q] = s.rows.n_x;
        a.n_entries[q] = s.rows.n_entries;
        a.row_whole_nx[q] = s.rows.row_whole_nx;
        a.row_rem[q] = s.rows.row_rem;
        a.row_thr[q] = s.rows.row_thr;
        a.table[q] = s.table;
        a.base[q] = total;
        a.mu_dt[q] = static_cast<T>(j.mu[q] * sc.dt);
        total += s.rows.n_entries;
    }
    for (int c = 0; c < D * (D + 1) / 2; ++c) a.chol[c] = static_cast<T>(j.chol[c]);
    a.half_dt = static_cast<T>(0.5 * sc.dt);
    a.sqrt_dt = static_cast<T>(std::sqrt(sc.dt));
    a.exp_scale = lv_exp_scale<T>();
    for (uint32_t q = 0; q < sc.n_dates; ++q) {
        a.log_level[q] = static_cast<T>(sc.log_level[q]);
        a.pay[q] = sc.pay[q];
    }
    a.log_ki = sc.ki ? static_cast<T>(sc.log_ki) : T(0);
    a.dt = sc.dt;
    a.ki = sc.ki ? 1 : 0;
    a.n_steps = j.paths.n_steps;
    a.observe_every = sc.observe_every;
    a.first_call_date = sc.first_call_date;
    a.shard = shard_of(j.paths);
    a.samples = static_cast<T *>(j.d_samples);
    a.fin = grid_finish_of(fs);
    const dim3 g(grid), b(kBlock);
    const size_t lds_bytes = static_cast<size_t>(total) * sizeof(VolPair<T>);
    if (sc.ki && sc.ki_every_step)
        hipLaunchKernelGGL((autocall_localvol_kernel<T, D, true>), g, b, lds_bytes, stream, a, d_partials);
    else
        hipLaunchKernelGGL((autocall_localvol_kernel<T, D, false>), g, b, lds_bytes, stream, a, d_partials);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_autocall_localvol_t(const AutocallLocalVolJob &j, double *d_partials, uint32_t grid,
                                             const FinishSpec &fs, hipStream_t stream)
{
    return dispatch_assets(j.d, [&](auto d) {
        return launch_autocall_localvol_d<T, decltype(d)::value>(j, d_partials, grid, fs, stream);
    });
}

}  // namespace mcamd
