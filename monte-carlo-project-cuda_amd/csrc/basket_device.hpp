// basket_device.hpp — device helpers shared by the kernels that step d correlated assets in registers (basket.hip,
// autocall.hip, autocall_localvol_impl.hpp): the step group's arithmetic, the extremum and where the loop's constants
// live.  The group walk and the chain of fused multiply-adds are written out in each kernel: one walk_groups and one
// bk_correlate for the three were tried, and each changed the kernels' vector instructions or their speed
// (profiles/README.md, "One schedule for two autocall calls; one walk for three kernels, tried").
#pragma once

#include "mc_device.hpp"

namespace mcamd {

constexpr int gcd_c(int a, int b) { return b == 0 ? a : gcd_c(b, a % b); }

__device__ __forceinline__ float bk_max(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double bk_max(double a, double b) { return __builtin_fmax(a, b); }
__device__ __forceinline__ float bk_min(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double bk_min(double a, double b) { return __builtin_fmin(a, b); }
// Where the loop's constants live.  fp32: in vector registers, because a scalar operand doubles the issue time of the
// full-rate v_fma_f32 / v_add_f32 (vgpr_resident).  fp64: a scalar operand costs nothing, but D + D (D + 1) / 2 doubles
// are 2 D + D (D + 1) scalar registers, and beyond D = 2 they no longer fit beside the kernel's other scalars — the
// compiler then spills them to vector-register lanes and reads them back one v_readlane at a time inside the step (up
// to 203 spills at D = 7, and scratch).  From D = 3 they are therefore moved to vector registers once per kernel.
template <int D>
__device__ __forceinline__ float bk_resident(float s) { return vgpr_resident(s); }
template <int D>
__device__ __forceinline__ double bk_resident(double s)
{
    if (D >= 3) asm volatile("" : "+v"(s));
    return s;
}

}  // namespace mcamd
