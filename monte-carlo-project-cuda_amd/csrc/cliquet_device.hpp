// cliquet_device.hpp — what a counted period adds to a cliquet path's sum and what the sum becomes at the end of the
// path, for every kernel that accumulates mcamd_price_cliquet's payoff whatever model walks the path (cliquet.hip on a
// local-volatility surface, heston_cliquet.hip under Heston).  Plain functions on the few values they need
// (path_frame.hpp says why).
//
// Definitions (include/mcamd.h, mcamd_price_cliquet): D = the period's log-return, one subtraction in the path precision;
//   SUM       sum += min(max(e^D - 1, lo), hi): one exponential per counted period;
//   COMPOUND  sum += min(max(D, lo), hi), lo and hi being ln(1 + bound) formed on the host; A = e^sum - 1 in fp64;
//   VARIANCE  sum = fma(D, D, sum); A = sum scale in fp64.
#pragma once

#include "cliquet.hpp"
#include "mc_device.hpp"

namespace mcamd {

__device__ __forceinline__ float cq_min(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double cq_min(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ float cq_max(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double cq_max(double a, double b) { return __builtin_fmax(a, b); }

// a counted period of log-return D into the path's sum
template <int KIND, typename T>
__device__ __forceinline__ void cliquet_add_period(T &sum, T D, T lo, T hi, T exp_scale, const MathCtx<T> &m)
{
    if (KIND == kCliquetSum) {
        const T R = exp_of_logreturn(T(1), D * exp_scale, m) - T(1);
        sum += cq_min(cq_max(R, lo), hi);
    } else if (KIND == kCliquetCompound) {
        sum += cq_min(cq_max(D, lo), hi);
    } else {
        sum = fma_t(D, D, sum);
    }
}

// the accumulated payoff A of a finished path, before the global bounds
template <int KIND, typename T>
__device__ __forceinline__ double cliquet_amount(T sum, T exp_scale, double scale, const MathCtx<T> &m)
{
    if (KIND == kCliquetSum) return static_cast<double>(sum);
    if (KIND == kCliquetCompound) return static_cast<double>(exp_of_logreturn(T(1), sum * exp_scale, m)) - 1.0;
    return static_cast<double>(sum) * scale;
}

}  // namespace mcamd
