// heston_device.hpp — the step of a Heston path under the full-truncation Euler scheme in the log-price, for any kernel
// that walks such paths (heston.hip, heston_smile.hip, heston_cliquet.hip, heston_barrier.hip; Asians can reuse it):
// the step constants, the four kernel arguments every launcher fills from the walk, the two normals of a step, and the
// move of one step.
//
// Definitions (include/mcamd.h, mcamd_price_heston): X = ln(S / S0) in NATURAL-log units, v the raw variance, which may
// go below zero; v+ = max(v, 0) is what the drift, the diffusion and the mean reversion read.  With the step's two
// independent normals z (the log-price's) and z' (the variance's own),
//     w = fma(rho, z, sqrt(1 - rho^2) z')
//     X += fma(s sqrt(dt), z, fma(-v+, dt / 2, (r - q) dt))                        s = sqrt(v+)
//     v += fma(s (xi sqrt(dt)), w, fma(-v+, kappa dt, kappa theta dt)).
// The X line is localvol_device.hpp's lv_move with s^2 replaced by v+ itself, so with xi = 0 and kappa = 0 a Heston path
// is the constant-volatility path of the surface kernels up to the rounding of s s against v+.  Every fused operation
// is an explicit fma_t and nothing else here is of the form a * b + c, so the compiler contracts nothing on its own and
// every kernel that includes this header computes the same bits.
//
// The map is continuous in every input — max, sqrt and fused multiply-adds, no branch on a moment ratio, no inverse
// distribution function — so two precisions of one path never take different formulas.
#pragma once

#include "heston.hpp"
#include "mc_device.hpp"

namespace mcamd {

// The variance normals' block of a step block: same key and subsequence, 2^63 beyond (n_steps is 32-bit: the
// log-price normals never get there).
constexpr uint64_t kHestonVarianceBlocks = 1ull << 63;

// The normals of one block of the walk: two Philox blocks, two Box-Muller fills.  Step j of block kb takes z.z[j] for
// the log-price and zv.z[j] for the variance.
template <typename T>
struct HestonNormals {
    Normals<T> z, zv;
    __device__ __forceinline__ void fill(const MathCtx<T> &m, const PhiloxKeys &key, uint64_t subsequence, uint32_t kb)
    {
        z.fill(m, key, subsequence, kb);
        zv.fill(m, key, subsequence, kHestonVarianceBlocks + kb);
    }
};

// The floating-point constants of a step, formed in double on the host and narrowed once.
template <typename T>
struct HestonConsts {
    T mu_dt;            // (r - q) dt
    T half_dt;          // dt / 2
    T sqrt_dt;          // sqrt(dt)
    T kappa_dt;         // kappa dt
    T kappa_theta_dt;   // kappa theta dt
    T xi_sqrt_dt;       // xi sqrt(dt)
    T rho;
    T rho_c;            // sqrt(1 - rho^2): 0 at rho = +-1
};

// Host: the constants of a walk's step, as every launcher of these paths forms them ...
template <typename T>
inline HestonConsts<T> heston_consts(const HestonWalk &w)
{
    const double sqrt_dt = std::sqrt(w.dt);
    HestonConsts<T> c;
    c.mu_dt = static_cast<T>(w.mu * w.dt);
    c.half_dt = static_cast<T>(0.5 * w.dt);
    c.sqrt_dt = static_cast<T>(sqrt_dt);
    c.kappa_dt = static_cast<T>(w.kappa * w.dt);
    c.kappa_theta_dt = static_cast<T>(w.kappa * w.theta * w.dt);
    c.xi_sqrt_dt = static_cast<T>(w.xi * sqrt_dt);
    c.rho = static_cast<T>(w.rho);
    c.rho_c = static_cast<T>(std::sqrt(1.0 - w.rho * w.rho));
    return c;
}
// ... and the exponent units per natural-log unit of the exponential that ends a path (exp_of_logreturn): log2 e in
// fp32, 65536 / ln 2 in fp64
template <typename T>
inline T heston_exp_scale()
{
    return static_cast<T>(sizeof(T) == 4 ? 1.4426950408889634 : f64::kExpScale);
}
// What the argument structs of the four kernels have in common, from the walk of their job (as lv_step_args: the
// structs share no sub-struct, each kernel's scalar loads are compiled against its own layout).
template <typename T, typename Args>
inline void heston_walk_args(Args &a, const HestonWalk &w)
{
    a.c = heston_consts<T>(w);
    a.exp_scale = heston_exp_scale<T>();
    a.v0 = static_cast<T>(w.v0);
    a.shard = shard_of(w.paths);
}

// Where they live.  fp32: in vector registers, because a scalar operand doubles the issue time of the full-rate fp32
// instructions (mc_device.hpp vgpr_resident).  fp64: an operation issues in 4 cycles with or without a scalar operand.
__device__ __forceinline__ HestonConsts<float> heston_resident(const HestonConsts<float> &c)
{
    return {vgpr_resident(c.mu_dt),    vgpr_resident(c.half_dt),        vgpr_resident(c.sqrt_dt),
            vgpr_resident(c.kappa_dt), vgpr_resident(c.kappa_theta_dt), vgpr_resident(c.xi_sqrt_dt),
            vgpr_resident(c.rho),      vgpr_resident(c.rho_c)};
}
__device__ __forceinline__ HestonConsts<double> heston_resident(const HestonConsts<double> &c) { return c; }

__device__ __forceinline__ float heston_positive(float v) { return __builtin_fmaxf(v, 0.0f); }
__device__ __forceinline__ double heston_positive(double v) { return __builtin_fmax(v, 0.0); }
// fp32: v_sqrt_f32 (1 ulp; 0 gives 0).  fp64: the correctly rounded square root, exact at 0 and on subnormal arguments,
// which f64::sqrt_pos (clamped to 1e-300, so sqrt 0 = 1e-150) is not; v+ = 0 is an everyday argument here.
__device__ __forceinline__ float heston_root(float a) { return __builtin_amdgcn_sqrtf(a); }
__device__ __forceinline__ double heston_root(double a) { return __builtin_sqrt(a); }

// One step from (X, v) with the log-price normal z and the variance's own normal zv.  Returns v+, the variance the step
// was taken at.
template <typename T>
__device__ __forceinline__ T heston_move(T &X, T &v, T z, T zv, const HestonConsts<T> &c)
{
    const T vp = heston_positive(v);
    const T s = heston_root(vp);
    const T w = fma_t(c.rho, z, c.rho_c * zv);
    X += fma_t(s * c.sqrt_dt, z, fma_t(-vp, c.half_dt, c.mu_dt));
    v += fma_t(s * c.xi_sqrt_dt, w, fma_t(-vp, c.kappa_dt, c.kappa_theta_dt));
    return vp;
}

}  // namespace mcamd
