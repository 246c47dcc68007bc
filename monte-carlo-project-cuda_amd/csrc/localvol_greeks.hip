// localvol_greeks.hip — price, delta, gamma, vega, bucketed vega, rho and dividend rho of a European option under a
// local-volatility surface from ONE walk of the paths, for gfx950 (both path precisions).
//
// Definitions (include/mcamd.h, mcamd_price_localvol_greeks): the path is mcamd_price_localvol's without a barrier —
// localvol_device.hpp's lookup, row carry and move, draw for draw.  Differentiating the log-Euler step gives a
// first-order recurrence per tangent, all driven by one factor per step:
//     c = sqrt(dt) z - s dt,   g = fma(s', c, 1),   s' = slope_k / dx strictly inside the axis, else 0
//     J <- J g (spot),  U <- fma(U, g, c) (parallel vega),  R <- fma(R, g, dt) (rate),
//     U^b <- fma(U^b, g, c) in the step's bucket, U^b g in an earlier one, 0 in a later one.
// The normal and the table entry are those the step loads anyway: a tangent costs two or three FMAs, no memory.
// Gamma is a central difference of the pathwise delta over two more walks from X_0 = +-eta on the same normals; each
// takes its own lookup (one more LDS read per walk and step) and carries its own J.
//
// The bucket of a step, floor(i B / n), is carried like the rows (a remainder counter, wave-uniform, scalar unit); the
// eight U^b live in registers and are addressed by an unrolled compare against that uniform index, never by a dynamic
// array index, which would send them to scratch.  BUCKETS = false and GAMMA = false drop their state altogether.
#include "localvol_device.hpp"
#include "localvol_greeks.hpp"
#include "path_frame.hpp"

namespace mcamd {

template <typename T>
struct LvGreeksArgs {
    LvSurface<T> surf;
    T mu_dt, half_dt, sqrt_dt, dt;
    T exp_scale;              // exponent units per natural-log unit (log2 e in fp32, 65536 / ln 2 in fp64)
    T K, S0;
    T eta;                    // gamma_bump
    int put;
    uint32_t n_steps;
    uint32_t n_buckets;
    uint32_t bkt_whole, bkt_rem, bkt_thr;   // B / n, B % n, n - B % n: the rows' carry on the bucket index
    PathShard shard;
    double S0d, T_mat;        // the sample's fp64 constants
    double S_up, S_dn, dS;    // S0 e^{+-eta} and their difference
    double *samples;          // nullable
    GridFinish fin;           // fin.out: the 32-double statistics record
};

// The step's common factor.  The two products and their difference stay three operations: the numpy restatement
// rounds each, and a contraction here would move the last bit of every tangent.
template <typename T>
__device__ __forceinline__ void lv_tangent_factor(const LvLookup<T> &l, T z, T inv_dx, T sqrt_dt, T dt, T &c, T &g)
{
#pragma clang fp contract(off)
    const T a = sqrt_dt * z;
    const T b = l.s * dt;
    c = a - b;
    const T sp = l.inside ? l.slope * inv_dx : T(0);
    g = fma_t(sp, c, T(1));
}

// One path's samples from its final state; every product, quotient and difference is one fp64 operation.
struct LvPathEnd {
    double y, m;   // h(S_T) and omega 1{omega (S_T - K) > 0} S_T
};
template <typename T>
__device__ __forceinline__ LvPathEnd lv_path_end(T X, const LvGreeksArgs<T> &a, const MathCtx<T> &m)
{
    const T St = exp_of_logreturn(a.S0, X * a.exp_scale, m);
    // not vanilla_payoff: the counted opcodes and figures stay, but the assembly's text does not
    T h = a.put ? a.K - St : St - a.K;
    h = h > T(0) ? h : T(0);
    const double Sd = static_cast<double>(St);
    return {static_cast<double>(h), h > T(0) ? (a.put ? -Sd : Sd) : 0.0};
}

template <typename T, bool GAMMA, bool BUCKETS>
__global__ __launch_bounds__(kBlock) void localvol_greeks_kernel(LvGreeksArgs<T> a, double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    constexpr int NBK = kLvGreeksMaxBuckets;
    VolPair<T> *tab = reinterpret_cast<VolPair<T> *>(lv_table_lds);
    lv_copy_table(tab, 0, a.surf.table, a.surf.rows.n_entries);
    __syncthreads();
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    const LvAxis<T> axis = lv_resident(a.surf.axis);
    const T mu_dt = resident_t(a.mu_dt), half_dt = resident_t(a.half_dt), sqrt_dt = resident_t(a.sqrt_dt);
    const T dt = resident_t(a.dt);
    const ThreadPaths paths(a.shard.n_local);   // made at the loop, seven of the eight kernels spill otherwise
    const uint32_t n_full = a.n_steps / NB;
    const uint32_t rem = a.n_steps - n_full * NB;
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // n and the zero tail of the statistics record
        a.fin.out[kLvGreeksRecord] = static_cast<double>(a.shard.n_local);
        for (int k = kLvGreeksRecord + 1; k < kLvGreeksStats; ++k) a.fin.out[k] = 0.0;
    }
    double acc[kLvGreeksRecord];
#pragma unroll
    for (int k = 0; k < kLvGreeksRecord; ++k) acc[k] = 0.0;
    for (const uint64_t i : paths) {
        const uint64_t subsequence = a.shard.path_offset + i;
        T X = T(0), J = T(1), U = T(0), R = T(0);
        T Xp = a.eta, Xm = -a.eta, Jp = T(1), Jm = T(1);   // GAMMA
        T Ub[NBK];                                          // BUCKETS
#pragma unroll
        for (int b = 0; b < NBK; ++b) Ub[b] = T(0);
        LvRow row{0, 0};
        uint32_t bkt = 0, bkt_phase = 0;   // floor(i B / n) and (i (B % n)) mod n, wave-uniform
        Normals<T> nz;
        auto step = [&](T z) {
            T c, g;
            const LvLookup<T> l = lv_sigma_slope(X, axis, a.surf.rows, tab, row);
            lv_tangent_factor(l, z, axis.inv_dx, sqrt_dt, dt, c, g);
            J = J * g;
            U = fma_t(U, g, c);
            R = fma_t(R, g, dt);
            if (BUCKETS) {
#pragma unroll
                for (int b = 0; b < NBK; ++b) {
                    if (static_cast<uint32_t>(b) < bkt) Ub[b] = Ub[b] * g;
                    else if (static_cast<uint32_t>(b) == bkt) Ub[b] = fma_t(Ub[b], g, c);
                }
                bkt += a.bkt_whole;
                if (bkt_phase >= a.bkt_thr) {
                    bkt_phase -= a.bkt_thr;
                    bkt += 1;
                } else {
                    bkt_phase += a.bkt_rem;
                }
            }
            lv_move(X, l.s, z, sqrt_dt, half_dt, mu_dt);
            if (GAMMA) {
                T cp, gp, cm, gm;
                const LvLookup<T> lp = lv_sigma_slope(Xp, axis, a.surf.rows, tab, row);
                const LvLookup<T> lm = lv_sigma_slope(Xm, axis, a.surf.rows, tab, row);
                lv_tangent_factor(lp, z, axis.inv_dx, sqrt_dt, dt, cp, gp);
                lv_tangent_factor(lm, z, axis.inv_dx, sqrt_dt, dt, cm, gm);
                Jp = Jp * gp;
                Jm = Jm * gm;
                lv_move(Xp, lp.s, z, sqrt_dt, half_dt, mu_dt);
                lv_move(Xm, lm.s, z, sqrt_dt, half_dt, mu_dt);
            }
            lv_next_row(a.surf.rows, row);
        };
        for (uint32_t kb = 0; kb < n_full; ++kb) {
            nz.fill(m, key, subsequence, kb);
#pragma unroll
            for (int j = 0; j < NB; ++j) step(nz.z[j]);
        }
        if (rem) {
            nz.fill(m, key, subsequence, n_full);
#pragma unroll
            for (int j = 0; j < NB - 1; ++j)
                if (static_cast<uint32_t>(j) < rem) step(nz.z[j]);
        }
        double q[kLvGreeks + NBK];
        {
#pragma clang fp contract(off)
            const LvPathEnd e = lv_path_end(X, a, m);
            const double mR = e.m * static_cast<double>(R);
            q[0] = e.y;
            q[1] = e.m * static_cast<double>(J) / a.S0d;
            q[2] = 0.0;
            q[3] = e.m * static_cast<double>(U);
            q[4] = mR - a.T_mat * e.y;
            q[5] = -mR;
            if (GAMMA) {
                const LvPathEnd ep = lv_path_end(Xp, a, m), em = lv_path_end(Xm, a, m);
                const double dp = ep.m * static_cast<double>(Jp) / a.S_up;
                const double dm = em.m * static_cast<double>(Jm) / a.S_dn;
                q[2] = (dp - dm) / a.dS;
            }
#pragma unroll
            for (int b = 0; b < NBK; ++b) q[kLvGreeks + b] = BUCKETS ? e.m * static_cast<double>(Ub[b]) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kLvGreeks + NBK; ++k) {
            if (!BUCKETS && k >= kLvGreeks) break;
            if (!GAMMA && k == 2) continue;
            acc[2 * k] += q[k];
            acc[2 * k + 1] = __builtin_fma(q[k], q[k], acc[2 * k + 1]);
        }
        if (a.samples) {
#pragma unroll
            for (int k = 0; k < kLvGreeks + NBK; ++k)
                if (static_cast<uint32_t>(k) < kLvGreeks + a.n_buckets) a.samples[static_cast<uint64_t>(k) * a.shard.n_local + i] = q[k];
        }
    }
    // one accumulator set in the last workgroup's sum: four sets of 28 doubles are 224 vector registers, which would
    // set the whole kernel's allocation (one wavefront per SIMD); a record's 28 loads are independent as it is
    finish_paths<kLvGreeksRecord, 1>(acc, partials, a.fin);
}

template <typename T, bool GAMMA, bool BUCKETS>
static void launch_lv_greeks_k(const LvGreeksArgs<T> &a, double *d_partials, uint32_t grid, hipStream_t stream)
{
    const size_t lds_bytes = static_cast<size_t>(a.surf.rows.n_entries) * sizeof(VolPair<T>);
    hipLaunchKernelGGL((localvol_greeks_kernel<T, GAMMA, BUCKETS>), dim3(grid), dim3(kBlock), lds_bytes, stream, a,
                       d_partials);
}

template <typename T>
static hipError_t launch_lv_greeks_t(const LocalVolGreeksJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                     hipStream_t stream)
{
    const uint32_t n_steps = j.walk.paths.n_steps;
    LvGreeksArgs<T> a;
    lv_step_args<T>(a, j.walk);
    a.shard = shard_of(j.walk.paths);
    a.dt = static_cast<T>(j.walk.dt);
    a.K = static_cast<T>(j.K);
    a.S0 = static_cast<T>(j.S0);
    a.eta = static_cast<T>(j.gamma_bump);
    a.put = j.put ? 1 : 0;
    a.n_steps = n_steps;
    a.n_buckets = j.n_buckets;
    a.bkt_whole = j.n_buckets / n_steps;
    a.bkt_rem = j.n_buckets % n_steps;
    a.bkt_thr = n_steps - a.bkt_rem;
    a.S0d = j.S0;
    a.T_mat = j.T;
    a.S_up = j.S0 * std::exp(j.gamma_bump);
    a.S_dn = j.S0 * std::exp(-j.gamma_bump);
    a.dS = a.S_up - a.S_dn;
    a.samples = j.d_samples;
    a.fin = GridFinish{fs.out, fs.ticket, -1.0};   // the kernel writes its own 32-double layout, n included
    const bool gamma = j.gamma_bump > 0.0, buckets = j.n_buckets != 0;
    if (gamma) {
        if (buckets) launch_lv_greeks_k<T, true, true>(a, d_partials, grid, stream);
        else launch_lv_greeks_k<T, true, false>(a, d_partials, grid, stream);
    } else {
        if (buckets) launch_lv_greeks_k<T, false, true>(a, d_partials, grid, stream);
        else launch_lv_greeks_k<T, false, false>(a, d_partials, grid, stream);
    }
    return hipGetLastError();
}

hipError_t launch_localvol_greeks(const LocalVolGreeksJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                                  hipStream_t stream)
{
    if (!finish_ok(finish, grid)) return hipErrorInvalidValue;
    if (!lv_grid_ok(job.walk.surface, job.walk.paths.n_steps) || job.n_buckets > kLvGreeksMaxBuckets)
        return hipErrorInvalidValue;
    return dispatch_precision(job.walk.paths.precision, [&](auto p) {
        return launch_lv_greeks_t<typename decltype(p)::type>(job, d_partials, grid, finish, stream);
    });
}

}  // namespace mcamd
