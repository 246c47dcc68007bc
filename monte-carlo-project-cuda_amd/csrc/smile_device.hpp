// smile_device.hpp — the strike phase of a smile kernel, for any kernel that stops its paths at expiry steps with one
// path per lane (localvol_smile.hip, heston_smile.hip): what a lane keeps of its strike, the loop over the wavefront's
// spots with the read-modify-write of the wavefront's record, and the rule for a wavefront without any path.
//
// At an expiry the wavefront holds 64 spots, one per lane, and turns the work a quarter-turn: lane k holds strike k and
// runs over the wavefront's valid paths j (a prefix; its length comes from the ballot), reading S_j by v_readlane into
// scalar registers, and keeps sum h and sum h^2 of node (m, k) in two fp64 registers.  After the loop lane k adds them
// to its own 16-byte entry of the wavefront's private record [m][k] in global memory — a plain read-modify-write that
// only this lane of this wavefront ever touches, in program order; the first trip of a wavefront writes instead of
// adding (its old value is taken as 0 and the entry is not read), and a wavefront without any path writes zeros, so
// every entry of every record is written whatever the buffer held.  smile_finish_kernel (smile.hip), one thread per
// node, sums the entries over the wavefronts in index order.  The host side of a smile is smile.hpp.
#pragma once

#include "mc_device.hpp"

namespace mcamd {

// lane j's value, j wave-uniform: v_readlane_b32 into scalar registers (a pair for fp64)
__device__ __forceinline__ float sm_broadcast(float v, uint32_t j)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), static_cast<int>(j)));
}
__device__ __forceinline__ double sm_broadcast(double v, uint32_t j)
{
    const uint64_t bits = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(bits), static_cast<int>(j)));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(bits >> 32), static_cast<int>(j)));
    return __builtin_bit_cast(double, (static_cast<uint64_t>(hi) << 32) | lo);
}

struct alignas(16) SmileEntry {
    double sum, sumsq;
};

// What lane k keeps of strike k.  h = max(+-(S - K), 0) as one fma with the sign in a lane constant:
// fma(S, sign, -sign K) rounds S - K or K - S once, as the subtraction does (the product with +-1 is exact).
template <typename T>
struct SmileLane {
    T sign;           // +1: calls, -1: puts
    T minus_sign_K;
};
template <typename T>
__device__ __forceinline__ SmileLane<T> smile_lane(const T *strikes, int put, uint32_t lane, bool has_node)
{
    const T sign = put ? T(-1) : T(1);
    T minus_sign_K = -sign * strikes[has_node ? lane : 0];
    asm volatile("" : "+v"(minus_sign_K));   // the strike has arrived before the first strike loop, not inside it
    return {sign, minus_sign_K};
}

// The record of a wavefront without any path (only its first trip can be empty) is all zeros.  That rule is two lines
// and stays written out in the kernels: as a function of this header, in any of five forms, it changed the compares,
// moves and scalar registers of both kernels of localvol_smile.hip, and the fp64 one ran 3.6 % slower at 32 x 64 nodes
// (DESIGN 25).

// The strike phase of one expiry: S is this lane's spot, count the wavefront's valid paths (lanes 0 .. count - 1),
// entry this lane's entry of the expiry's row (read and written where has_node: lane < n_strikes), first whether this is
// the wavefront's first trip (wave-uniform).
template <typename T>
__device__ __forceinline__ void smile_strike_phase(T S, uint32_t count, const SmileLane<T> &ln, bool has_node, bool first,
                                                   SmileEntry *entry)
{
    // the entry's load is issued before the strike loop, whose length hides its latency
    SmileEntry old{0.0, 0.0};
    if (!first && has_node) old = *entry;
    double sum = 0.0, sumsq = 0.0;
    for (uint32_t j = 0; j < count; ++j) {
        const T Sj = sm_broadcast(S, j);
        T h = fma_t(Sj, ln.sign, ln.minus_sign_K);
        h = h > T(0) ? h : T(0);
        const double hd = static_cast<double>(h);
        sum += hd;
        sumsq = __builtin_fma(hd, hd, sumsq);
    }
    if (has_node) *entry = SmileEntry{old.sum + sum, old.sumsq + sumsq};
}

}  // namespace mcamd
