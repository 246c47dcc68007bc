// heston_greeks.hip — price, delta, gamma, rho, dividend rho and the five model-parameter sensitivities of a European
// option under Heston stochastic volatility from ONE simulation, for gfx950 (both path precisions).
//
// Definitions (include/mcamd_heston_greeks.h): the base walk is mcamd_price_heston's, heston_device.hpp's heston_move
// draw for draw.  X = ln(S / S0) does not depend on S0 and moves with r and q by +-T exactly, so delta, gamma, rho and
// dividend rho are read off the base walk's S_T.  The model parameters are NOT differentiated along the path (the
// tangent of sqrt(v+) is 1 / (2 sqrt(v+)), and the scheme visits v+ = 0 on everyday inputs): each requested parameter
// gets two more (X, v) walks at the parameter +- its bump, on the SAME z and z' of every step.  The two Philox blocks
// and Box-Muller fills of a block of the walk are made once per path whatever P is; a bumped walk adds the ten
// operations of heston_move per step and one exponential at the end.
//
// The 1 + 2 P states live in registers (every loop over the walks is unrolled on the template argument P; nothing is
// indexed by a runtime value).  Which parameters are bumped is data: a walk is its five constants that a parameter
// can move (kappa dt, kappa theta dt, xi sqrt(dt), rho, sqrt(1 - rho^2)) and its v0; (r - q) dt, dt / 2 and sqrt(dt)
// are the same bits in every walk and are held once.  fp64 reads the per-walk constants as scalar operands (free in
// fp64); fp32 keeps them in vector registers, as heston_resident does for the one walk of heston.hip.
#include "heston_device.hpp"
#include "heston_greeks.hpp"
#include "path_frame.hpp"

#include <cstring>

namespace mcamd {

// what a bump can change of a walk
template <typename T>
struct HestonGreeksWalk {
    T kappa_dt, kappa_theta_dt, xi_sqrt_dt, rho, rho_c;
    T v0;
};

template <typename T, int P>
struct HestonGreeksArgs {
    T mu_dt, half_dt, sqrt_dt;            // the same in every walk
    HestonGreeksWalk<T> w[1 + 2 * P];     // the base walk, then (+, -) per requested parameter
    T exp_scale;                          // exponent units per natural-log unit (log2 e in fp32, 65536 / ln 2 in fp64)
    T K, S0;
    T u_up, u_dn;                         // e^{eta}, e^{-eta}: formed in double, narrowed once
    double inv_n;                         // 1 / n_steps
    int put;
    uint32_t n_steps;
    PathShard shard;
    T *samples;                           // nullable
    GridFinish fin;                       // fin.out: the 32-double statistics record
};

template <typename T, int P>
__global__ __launch_bounds__(kBlock) void heston_greeks_kernel(HestonGreeksArgs<T, P> a, double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    constexpr int W = 1 + 2 * P;
    constexpr int R = heston_greeks_record(P);
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    const T mu_dt = resident_t(a.mu_dt), half_dt = resident_t(a.half_dt), sqrt_dt = resident_t(a.sqrt_dt);
    HestonConsts<T> c[W];
#pragma unroll
    for (int w = 0; w < W; ++w)
        c[w] = HestonConsts<T>{mu_dt, half_dt, sqrt_dt, resident_t(a.w[w].kappa_dt), resident_t(a.w[w].kappa_theta_dt),
                               resident_t(a.w[w].xi_sqrt_dt), resident_t(a.w[w].rho), resident_t(a.w[w].rho_c)};
    const StepBlocks blocks = step_blocks<NB>(a.n_steps);
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // n and the zero tail of the statistics record
        a.fin.out[R] = static_cast<double>(a.shard.n_local);
        for (int k = R + 1; k < kHestonGreeksStats; ++k) a.fin.out[k] = 0.0;
    }
    double acc[R];
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] = 0.0;
    for (const uint64_t i : ThreadPaths{a.shard.n_local}) {
        const uint64_t subsequence = a.shard.path_offset + i;
        T X[W], v[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            X[w] = T(0);
            v[w] = a.w[w].v0;
        }
        T v_sum = T(0);       // the base walk's sum of v+ over the steps
        uint32_t trunc = 0;   // the base walk's steps entered with v < 0
        HestonNormals<T> nz;
        walk_steps<NB>(
            blocks, [&](uint32_t kb) { nz.fill(m, key, subsequence, kb); },
            [&](uint32_t, int j) {
                const T z = nz.z.z[j], zv = nz.zv.z[j];
                trunc += v[0] < T(0) ? 1u : 0u;
                v_sum += heston_move(X[0], v[0], z, zv, c[0]);
#pragma unroll
                for (int w = 1; w < W; ++w) heston_move(X[w], v[w], z, zv, c[w]);
            });
        T h[W];
        T St = T(0);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const T Sw = exp_of_logreturn(a.S0, X[w] * a.exp_scale, m);
            h[w] = vanilla_payoff(a.put, a.K, Sw);
            if (w == 0) St = Sw;
        }
        T d, g;
        {
#pragma clang fp contract(off)   // each product below is one multiply: nothing fuses into the payoff's difference
            const T S_up = St * a.u_up;
            const T S_dn = St * a.u_dn;
            const bool in_up = vanilla_payoff(a.put, a.K, S_up) > T(0);
            const bool in_dn = vanilla_payoff(a.put, a.K, S_dn) > T(0);
            d = h[0] > T(0) ? (a.put ? -St : St) : T(0);
            g = in_up != in_dn ? St : T(0);   // sgn S_T ([up] - [dn]): a call is in the money up before down, a put down before up
        }
        if (a.samples) {
            const uint64_t n = a.shard.n_local;
            a.samples[i] = h[0];
            a.samples[n + i] = d;
            a.samples[2 * n + i] = g;
#pragma unroll
            for (int w = 1; w < W; ++w) a.samples[static_cast<uint64_t>(2 + w) * n + i] = h[w];
        }
        {
#pragma clang fp contract(off)   // y, d, d - y, g and c_p are rounded before they are squared
            const double y = static_cast<double>(h[0]), dd = static_cast<double>(d), gg = static_cast<double>(g);
            const double e = dd - y;
            add_sample(acc, y);
            acc[2] += dd;
            acc[3] = __builtin_fma(dd, dd, acc[3]);
            acc[4] = __builtin_fma(e, e, acc[4]);
            acc[5] += gg;
            acc[6] = __builtin_fma(gg, gg, acc[6]);
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const double cp = static_cast<double>(h[1 + 2 * p]) - static_cast<double>(h[2 + 2 * p]);
                acc[7 + 2 * p] += cp;
                acc[8 + 2 * p] = __builtin_fma(cp, cp, acc[8 + 2 * p]);
            }
        }
        acc[7 + 2 * P] += static_cast<double>(trunc);
        acc[8 + 2 * P] += static_cast<double>(v_sum) * a.inv_n;
    }
    // one accumulator set in the last workgroup's sum (localvol_greeks.hip: four sets of a wide record would set the
    // whole kernel's register allocation); a grid of up to 256 workgroups sums in heston.hip's order all the same
    finish_paths<R, 1>(acc, partials, a.fin);
}

template <typename T>
static bool same_bits(T a, T b)
{
    return std::memcmp(&a, &b, sizeof(T)) == 0;
}

template <typename T, int P>
static hipError_t launch_heston_greeks_k(const HestonGreeksJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                         hipStream_t stream)
{
    HestonGreeksArgs<T, P> a;
    const HestonConsts<T> base = heston_consts<T>(j.walk[0]);
    a.mu_dt = base.mu_dt;
    a.half_dt = base.half_dt;
    a.sqrt_dt = base.sqrt_dt;
    for (int w = 0; w < 1 + 2 * P; ++w) {
        // each walk's constants from its own HestonWalk, as every launcher of these paths forms them
        const HestonConsts<T> c = heston_consts<T>(j.walk[w]);
        if (!same_bits(c.mu_dt, base.mu_dt) || !same_bits(c.half_dt, base.half_dt) || !same_bits(c.sqrt_dt, base.sqrt_dt))
            return hipErrorInvalidValue;   // a bump moves no drift and no step
        a.w[w] = HestonGreeksWalk<T>{c.kappa_dt, c.kappa_theta_dt, c.xi_sqrt_dt, c.rho, c.rho_c, static_cast<T>(j.walk[w].v0)};
    }
    const PathRange &paths = j.walk[0].paths;
    a.exp_scale = heston_exp_scale<T>();
    a.K = static_cast<T>(j.K);
    a.S0 = static_cast<T>(j.S0);
    a.u_up = static_cast<T>(std::exp(j.gamma_eta));
    a.u_dn = static_cast<T>(std::exp(-j.gamma_eta));
    a.inv_n = 1.0 / static_cast<double>(paths.n_steps);
    a.put = j.put ? 1 : 0;
    a.n_steps = paths.n_steps;
    a.shard = shard_of(paths);
    a.samples = static_cast<T *>(j.d_samples);
    a.fin = GridFinish{fs.out, fs.ticket, -1.0};   // the kernel writes its own 32-double layout, n included
    hipLaunchKernelGGL((heston_greeks_kernel<T, P>), dim3(grid), dim3(kBlock), 0, stream, a, d_partials);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_heston_greeks_t(const HestonGreeksJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                         hipStream_t stream)
{
    switch (j.n_params) {
    case 0: return launch_heston_greeks_k<T, 0>(j, d_partials, grid, fs, stream);
    case 1: return launch_heston_greeks_k<T, 1>(j, d_partials, grid, fs, stream);
    case 2: return launch_heston_greeks_k<T, 2>(j, d_partials, grid, fs, stream);
    case 3: return launch_heston_greeks_k<T, 3>(j, d_partials, grid, fs, stream);
    case 4: return launch_heston_greeks_k<T, 4>(j, d_partials, grid, fs, stream);
    case 5: return launch_heston_greeks_k<T, 5>(j, d_partials, grid, fs, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_heston_greeks(const HestonGreeksJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                                hipStream_t stream)
{
    if (!finish_ok(finish, grid)) return hipErrorInvalidValue;
    if (job.n_params < 0 || job.n_params > kHestonGreeksMaxParams) return hipErrorInvalidValue;
    for (int w = 0; w < 1 + 2 * job.n_params; ++w)
        if (!heston_walk_ok(job.walk[w])) return hipErrorInvalidValue;
    return dispatch_precision(job.walk[0].paths.precision, [&](auto p) {
        return launch_heston_greeks_t<typename decltype(p)::type>(job, d_partials, grid, finish, stream);
    });
}

}  // namespace mcamd
