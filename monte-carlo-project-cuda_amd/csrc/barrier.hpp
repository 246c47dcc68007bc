// barrier.hpp — host-side interface of the single-barrier kernels (barrier.hip) for the C ABI (capi_pathdep.cpp).
//
// A barrier kernel walks the log-space paths of mcamd_price_paths (same Philox stream = global path id, same
// Exponents), keeps each path's survival weight w (include/mcamd.h, mcamd_price_barrier) and forms one undiscounted
// sample per path in fp64: w h(S_T) for a knock-out, (1 - w) h(S_T) for a knock-in.  Its block record is
// {sum y, sum y^2, wave-steps executed, lane-steps of paths not yet knocked}: 4 doubles.
#pragma once

#include "launch.hpp"

namespace mcamd {

constexpr int kBarrierRecord = 4;

struct BarrierJob {
    PathJob path;      // drift, vol, K, B, S_start = S0, n_sim = n_steps, seed, shard, precision (window, vr unused)
    bool up;           // the barrier lies above the spot (else below)
    bool out;          // knock-out (else knock-in)
    bool continuous;   // Brownian-bridge survival factors between the step ends (else the step ends alone)
    bool put;          // h(S) = (K - S)+ (else (S - K)+)
    double kq;         // 2 / (v^2 dt), natural-log units
    void *d_samples;   // nullable: n_local samples of the path precision
};

// Enqueues the kernel on a grid of one_path_per_thread_grid(n_local) workgroups.  finish.out: where the final record
// goes (device memory, or pinned host memory the device can write); finish.ticket: the context's zeroed arrival
// counter; d_partials: grid x kBarrierRecord doubles.  With finish.n_value >= 0 (the enqueue form) the record is the
// 6-double statistics layout {sum, sumsq, 0, 0, 0, n}: it has no slot for the two step counters, which are then left
// out of the sum.
hipError_t launch_barrier(const BarrierJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                          hipStream_t stream);

}  // namespace mcamd
