// barrier_device.hpp — the single barrier's definitions and its sample, for every kernel that prices one (barrier.hip
// under constant volatility, localvol.hip under a surface, heston_barrier.hip under Heston).
//
// Definitions (include/mcamd.h, mcamd_price_barrier): X_i = ln(S_i / S0) after step i, b = ln(B / S0); a path is hit at
// step end i when b > X_i (down) or X_i > b (up); d_i = X_i - b (down) or b - X_i (up), d_0 = |b|.  The survival weight
// w is the product over the steps of 1{no hit at i} and — continuous monitoring — of f_i = 1 - exp(-q_i) with
// q_i = 2 d_{i-1} d_i / (s_i^2 dt), s_i^2 the variance rate step i was taken at (v^2, the surface's s^2, Heston's v+);
// f_i is DEFINED as 1 for q_i >= Q (Q = 38 in fp64, 18 in fp32: there exp(-q) < 2^-54 / 2^-25 and 1 - exp(-q) rounds to
// 1 anyway; barrier.hpp bridge_units).  The sample is w h(S_T) (knock-out) or (1 - w) h(S_T) (knock-in), formed once per
// path in fp64 (barrier_sample below), with h the vanilla payoff (path_frame.hpp vanilla_payoff).
//
// What is NOT here: the step's barrier body — d, the hit test, alive, and with continuous monitoring the product
// kq d' d, close_by, the wave-uniform ballot, bridge_factor and w — stays written out in each of the three kernels.
// Every function boundary around it changed machine code (tools/isa_diff.py against the commit before this header,
// cross-compiled, never timed on a GPU):
//   - the hit test as barrier_end<UP>(alive, X, b) changed the four fp32 discrete kernels of barrier.hip: another mix
//     of v_cmp / v_cndmask / v_and, SGPRs 69 -> 71;
//   - the continuous part (the product, close_by, ballot, bridge_factor, w), tried by reference, by value returning w,
//     without __forceinline__ and inside a BarrierWatch struct: every form gave +6 v_cndmask_b32_e64 and VGPRs 98 -> 96
//     in the fp64 continuous kernels of barrier.hip, +6 or +7 v_cndmask in all 8 continuous kernels of localvol.hip and
//     of heston_barrier.hip, and moved the SGPR spills of two local-volatility fp64 kernels (4 -> 8, 8 -> 0).
// Whoever tries again brings a same-box GPU A/B; barrier_sample and vanilla_payoff change no kernel.
#pragma once

#include "mc_device.hpp"

namespace mcamd {

// One path's sample from its weight wd (0 on a hit path) and h = h(S_T).  A knocked path of a knock-out pays 0 whatever
// its (possibly unfinished) price is.
template <bool OUT, typename T>
__device__ __forceinline__ double barrier_sample(bool alive, double wd, T h)
{
    return OUT ? (alive ? wd * static_cast<double>(h) : 0.0) : (1.0 - wd) * static_cast<double>(h);
}

}  // namespace mcamd
