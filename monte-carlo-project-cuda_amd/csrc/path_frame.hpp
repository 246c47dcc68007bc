// path_frame.hpp — the frame of a one-path-per-thread kernel around the step walk of mc_device.hpp: which paths a
// thread takes, what a path leaves in the thread's record, how the grid's records become the final one.
// Plain functions and small structs on the few values they need: a helper that took the kernel's body as a capturing
// lambda changed the registers and instructions of some eighty kernels (tools/isa_diff.py); these change none.
#pragma once

#include "launch.hpp"
#include "mc_device.hpp"

namespace mcamd {

// The ids below n that this thread takes: for (const uint64_t i : ThreadPaths{a.shard.n_local}) { ... }.  It takes the
// bound, not the Args (the American sweep walks training paths, no shard), and reads the stride where it is made: a
// kernel whose registers depend on where that happens names its range ahead of the loop (localvol_greeks.hip).
struct ThreadPaths {
    uint64_t n, stride;
    __device__ __forceinline__ explicit ThreadPaths(uint64_t n_) : n(n_), stride(static_cast<uint64_t>(gridDim.x) * kBlock) {}
    struct Iterator {
        uint64_t i, stride;
        __device__ __forceinline__ uint64_t operator*() const { return i; }
        __device__ __forceinline__ void operator++() { i += stride; }
        __device__ __forceinline__ bool operator!=(const Iterator &end) const { return i < end.i; }
    };
    __device__ __forceinline__ Iterator begin() const { return {static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x, stride}; }
    __device__ __forceinline__ Iterator end() const { return {n, 0}; }
};

// h(S) = (K - S)+ for a put, (S - K)+ for a call, in the path precision; put is wave-uniform.
template <typename T>
__device__ __forceinline__ T vanilla_payoff(int put, T K, T St)
{
    const T h = put ? K - St : St - K;
    return h > T(0) ? h : T(0);
}

// One path's sample into the record's first two slots: the sum and the sum of squares.
template <int N>
__device__ __forceinline__ void add_sample(double (&acc)[N], double y)
{
    acc[0] += y;
    acc[1] = __builtin_fma(y, y, acc[1]);
}

// The steps a path's wavefront ran (wave-uniform), counted once per wavefront: a wavefront's active lanes are a prefix
// (path ids grow with the lane), so lane 0 is active whenever any lane is, and it alone counts.
__device__ __forceinline__ void add_wave_steps(double &slot, uint32_t wave_steps)
{
    if ((threadIdx.x & (kWave - 1)) == 0) slot += static_cast<double>(wave_steps);
}
// The counted record {sum, sumsq, wave-steps, live lane-steps} of the barrier, lookback, basket and local-volatility
// kernels.  (They zero both counters before finishing when fin.n_value >= 0; that line stays in the kernels: as a
// function it changed 14 of barrier.hip's 16 kernels.)
__device__ __forceinline__ void add_counters(double (&acc)[4], uint32_t wave_steps, uint32_t live)
{
    add_wave_steps(acc[2], wave_steps);
    acc[3] += static_cast<double>(live);
}

// Every thread of the workgroup calls this once, after its last path (contains barriers).
template <int N, int ACC = MCAMD_FINISH_ACC>
__device__ __forceinline__ void finish_paths(double (&acc)[N], double *__restrict__ partials, const GridFinish &fin)
{
    block_sumN<kBlock, N>(acc);
    grid_finish<kBlock, N, ACC>(acc, partials, fin);
}

inline GridFinish grid_finish_of(const FinishSpec &fs) { return GridFinish{fs.out, fs.ticket, fs.n_value}; }

}  // namespace mcamd
