// autocall_localvol_impl.hpp — the worst-of autocallable kernel under per-asset local-volatility surfaces, for gfx950.
// Included by autocall_localvol.hip (fp64) and autocall_localvol_f32.hip (fp32), which instantiate D = 1..8 each.
//
// Definitions (include/mcamd.h, mcamd_price_autocall_localvol): X_{j,i} = ln(S_{j,i} / S_{j,0}) in NATURAL-log units.
// Step i looks asset j's volatility up at X_j in row_j(i) = floor(i n_t,j / n) of asset j's surface, exactly as
// localvol.hip does — u = clamp((X_j - x_min,j) / dx_j, 0, n_x,j - 1), k = min(floor u, n_x,j - 2), f = u - k,
// s_j = fma(f, slope_k, sigma_k) — forms w_j = sum_{k <= j} l_jk z_{i,k} as a chain of fused multiply-adds in ascending
// k from 0 (z_{i,k} normal number i d + k of the path's stream, as basket.hip draws it) and moves
// X_j += fma(s_j sqrt(dt), w_j, fma(-s_j^2, dt / 2, (r - q_j) dt)): localvol.hip's step with w_j in the place of z.
// l_i = min_j X_{j,i}.  Dates, levels, payments, the call test, the knock-in modes, the sample and the block record are
// those of autocall.hip, with ln L_q and ln ki_level in natural-log units; A_n = exp_of_logreturn(1, l_n exp_scale).
//
// The walk is restated here, not shared: the loop is autocall.hip's (groups of G = NB / gcd(D, NB) steps on whole Philox
// blocks, unrolled with the block boundaries at compile-time positions; a wave-uniform observation test and date
// counter; a wavefront leaves at the first group end where no lane is uncalled), the lookup and the row carry are
// localvol.hip's, one per asset.  The D pair tables lie back to back in dynamic LDS, copied once per workgroup; a step
// costs D reads (ds_read_b64 in fp32, ds_read_b128 in fp64) at asset j's row base — which starts at the table's own
// base — plus the lane's k_j.  The per-asset grid constants and the row carries are wave-uniform (scalar unit).
#pragma once

#include "autocall_localvol.hpp"
#include "path_consts.hpp"
#include "basket_device.hpp"

namespace mcamd {

template <typename T, int D>
struct AutocallLocalVolArgs {
    T x_min[D], inv_dx[D];           // node 0 and 1 / dx of asset j's axis
    T u_max[D];                      // n_x - 1
    T mu_dt[D];                      // (r - q_j) dt
    T chol[D * (D + 1) / 2];         // l_jk at [j (j + 1) / 2 + k]
    uint32_t k_max[D];               // n_x - 2
    uint32_t n_x[D];
    uint32_t base[D];                // where asset j's table starts in LDS, in entries
    uint32_t n_entries[D];           // n_t n_x
    uint32_t row_whole_nx[D];        // (n_t / n_steps) n_x: what the row base grows by at every step
    uint32_t row_rem[D];             // n_t % n_steps
    uint32_t row_thr[D];             // n_steps - row_rem: the remainder counter carries when it reaches this
    const VolPair<T> *table[D];      // global memory
    T half_dt, sqrt_dt;
    T exp_scale;                     // exponent units per natural-log unit (log2 e in fp32, 65536 / ln 2 in fp64)
    T log_level[kAutocallMaxDates];  // ln L_q at [q - 1]
    T log_ki;                        // ln ki_level
    double pay[kAutocallMaxDates];   // pay_q at [q - 1]
    double dt;
    int ki;                          // a knock-in applies (always, with KI_EVERY_STEP)
    uint32_t n_steps, observe_every, first_call_date;
    uint64_t seed;
    uint64_t path_offset;
    uint64_t n_local;
    T *samples;                      // nullable
    GridFinish fin;
};

// Where the step's floating-point constants live.  fp32: in vector registers, because a scalar operand doubles the
// issue time of the full-rate fp32 instructions (mc_device.hpp vgpr_resident).  fp64: an operation issues in 4 cycles
// with or without a scalar operand, so the per-asset grid constants and drifts stay where the compiler puts them; the
// D (D + 1) / 2 entries of the Cholesky factor follow basket_device.hpp's bk_resident (vector registers from D = 3):
// left scalar they do not fit beside the kernel's other scalars and are read back one v_readlane at a time inside the
// step, which measured 5 % (D = 3) and 7 % (D = 8) slower on the benchmark note.
__device__ __forceinline__ float alv_resident(float s) { return vgpr_resident(s); }
__device__ __forceinline__ double alv_resident(double s) { return s; }

extern __shared__ __attribute__((aligned(16))) unsigned char alv_table_lds[];

template <typename T, int D, bool KI_EVERY_STEP>
__global__ __launch_bounds__(kBlock) void autocall_localvol_kernel(AutocallLocalVolArgs<T, D> a,
                                                                   double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    constexpr int G = NB / gcd_c(D, NB);   // steps that consume whole blocks
    constexpr int BPG = G * D / NB;        // the blocks they consume
    constexpr int NC = D * (D + 1) / 2;
    // every thread of the workgroup copies its share of the D tables; one barrier, then the tables are read-only
    VolPair<T> *tab = reinterpret_cast<VolPair<T> *>(alv_table_lds);
#pragma unroll
    for (int j = 0; j < D; ++j)
        for (uint32_t e = threadIdx.x; e < a.n_entries[j]; e += kBlock) tab[a.base[j] + e] = a.table[j][e];
    __syncthreads();
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.seed);
    T x_min[D], inv_dx[D], u_max[D], mu_dt[D], chol[NC];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        x_min[j] = alv_resident(a.x_min[j]);
        inv_dx[j] = alv_resident(a.inv_dx[j]);
        u_max[j] = alv_resident(a.u_max[j]);
        mu_dt[j] = alv_resident(a.mu_dt[j]);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) chol[c] = bk_resident<D>(a.chol[c]);
    const T half_dt = alv_resident(a.half_dt), sqrt_dt = alv_resident(a.sqrt_dt);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    const uint32_t n_groups = a.n_steps / G;
    const uint32_t rem = a.n_steps - n_groups * G;
    double acc[kAutocallRecord] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < a.n_local; i += stride) {
        const uint64_t subsequence = a.path_offset + i;
        T X[D];                  // ln(S_j / S_{j,0}) so far, natural units
        uint32_t row_base[D];    // base_j + row_j(i) n_x,j, wave-uniform
        uint32_t row_phase[D];   // (i row_rem_j) mod n_steps, wave-uniform
#pragma unroll
        for (int j = 0; j < D; ++j) {
            X[j] = T(0);
            row_base[j] = a.base[j];
            row_phase[j] = 0;
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
                    for (int j = 0; j < D; ++j) {
                        T u = (X[j] - x_min[j]) * inv_dx[j];
                        u = bk_min(bk_max(u, T(0)), u_max[j]);   // a NaN lands on node 0: the index stays inside the table
                        uint32_t k = static_cast<uint32_t>(u);
                        k = k < a.k_max[j] ? k : a.k_max[j];
                        const T f = u - static_cast<T>(k);
                        const VolPair<T> p = tab[row_base[j] + k];
                        sig[j] = fma_t(f, p.slope, p.sigma);
                        // row_j(i + 1)
                        row_base[j] += a.row_whole_nx[j];
                        if (row_phase[j] >= a.row_thr[j]) {
                            row_phase[j] -= a.row_thr[j];
                            row_base[j] += a.n_x[j];
                        } else {
                            row_phase[j] += a.row_rem[j];
                        }
                    }
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
                    for (int j = 0; j < D; ++j) {
                        const T s2 = sig[j] * sig[j];
                        X[j] += fma_t(sig[j] * sqrt_dt, w[j], fma_t(-s2, half_dt, mu_dt[j]));
                    }
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
        acc[0] += y;
        acc[1] = __builtin_fma(y, y, acc[1]);
        acc[2] += called ? 1.0 : 0.0;
        acc[3] += called ? static_cast<double>(s_call) * a.dt : 0.0;
        acc[4] += (!called && knocked) ? 1.0 : 0.0;
        // a wavefront's active lanes are a prefix (path ids grow with the lane): lane 0 counts the wavefront's steps
        if ((threadIdx.x & (kWave - 1)) == 0) acc[5] += static_cast<double>(steps_run);
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
    AutocallLocalVolArgs<T, D> a{};
    uint32_t total = 0;
    for (int q = 0; q < D; ++q) {
        const double dx = (j.x_max[q] - j.x_min[q]) / static_cast<double>(j.n_x[q] - 1);
        a.x_min[q] = static_cast<T>(j.x_min[q]);
        a.inv_dx[q] = static_cast<T>(1.0 / dx);
        a.u_max[q] = static_cast<T>(j.n_x[q] - 1);
        a.mu_dt[q] = static_cast<T>(j.mu[q] * j.dt);
        a.k_max[q] = j.n_x[q] - 2;
        a.n_x[q] = j.n_x[q];
        a.base[q] = total;
        a.n_entries[q] = j.n_t[q] * j.n_x[q];
        a.row_whole_nx[q] = (j.n_t[q] / j.n_steps) * j.n_x[q];
        a.row_rem[q] = j.n_t[q] % j.n_steps;
        a.row_thr[q] = j.n_steps - a.row_rem[q];
        a.table[q] = static_cast<const VolPair<T> *>(j.d_table[q]);
        total += a.n_entries[q];
    }
    for (int c = 0; c < D * (D + 1) / 2; ++c) a.chol[c] = static_cast<T>(j.chol[c]);
    a.half_dt = static_cast<T>(0.5 * j.dt);
    a.sqrt_dt = static_cast<T>(std::sqrt(j.dt));
    a.exp_scale = static_cast<T>(sizeof(T) == 4 ? 1.4426950408889634 : f64::kExpScale);   // make_consts' literals
    for (uint32_t q = 0; q < j.n_dates; ++q) {
        a.log_level[q] = static_cast<T>(j.log_level[q]);
        a.pay[q] = j.pay[q];
    }
    a.log_ki = j.ki ? static_cast<T>(j.log_ki) : T(0);
    a.dt = j.dt;
    a.ki = j.ki ? 1 : 0;
    a.n_steps = j.n_steps;
    a.observe_every = j.observe_every;
    a.first_call_date = j.first_call_date;
    a.seed = j.seed;
    a.path_offset = j.path_offset;
    a.n_local = j.n_local;
    a.samples = static_cast<T *>(j.d_samples);
    a.fin = GridFinish{fs.out, fs.ticket, fs.n_value};
    const dim3 g(grid), b(kBlock);
    const size_t lds_bytes = static_cast<size_t>(total) * sizeof(VolPair<T>);
    if (j.ki && j.ki_every_step)
        hipLaunchKernelGGL((autocall_localvol_kernel<T, D, true>), g, b, lds_bytes, stream, a, d_partials);
    else
        hipLaunchKernelGGL((autocall_localvol_kernel<T, D, false>), g, b, lds_bytes, stream, a, d_partials);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_autocall_localvol_t(const AutocallLocalVolJob &j, double *d_partials, uint32_t grid,
                                             const FinishSpec &fs, hipStream_t stream)
{
    switch (j.d) {
    case 1: return launch_autocall_localvol_d<T, 1>(j, d_partials, grid, fs, stream);
    case 2: return launch_autocall_localvol_d<T, 2>(j, d_partials, grid, fs, stream);
    case 3: return launch_autocall_localvol_d<T, 3>(j, d_partials, grid, fs, stream);
    case 4: return launch_autocall_localvol_d<T, 4>(j, d_partials, grid, fs, stream);
    case 5: return launch_autocall_localvol_d<T, 5>(j, d_partials, grid, fs, stream);
    case 6: return launch_autocall_localvol_d<T, 6>(j, d_partials, grid, fs, stream);
    case 7: return launch_autocall_localvol_d<T, 7>(j, d_partials, grid, fs, stream);
    case 8: return launch_autocall_localvol_d<T, 8>(j, d_partials, grid, fs, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mcamd
