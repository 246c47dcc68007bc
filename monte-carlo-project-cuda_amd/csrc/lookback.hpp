// lookback.hpp — host-side interface of the lookback kernels (lookback.hip) for the C ABI (capi_pathdep.cpp).
//
// A lookback kernel walks the log-space paths of mcamd_price_paths (same Philox stream = global path id, same
// Exponents), keeps the one running extremum E of X = ln(S / S0) the product needs (include/mcamd.h,
// mcamd_price_lookback) and forms one undiscounted sample per path in fp64 from S_T and S_E = S0 e^E.  Continuous
// monitoring draws one uniform per step from the same key and subsequence at Philox block 2^63 + k.  Its block record
// is {sum y, sum y^2, wave-steps executed, lane-steps that formed a bridge extremum}: 4 doubles.
#pragma once

#include "launch.hpp"

namespace mcamd {

constexpr int kLookbackRecord = 4;

struct LookbackJob {
    PathJob path;      // drift, vol, S_start = S0, n_sim = n_steps, seed, shard, precision (K, B, window, vr unused)
    bool maximum;      // the path tracks its maximum (floating put, fixed call), else its minimum
    bool fixed;        // fixed strike K (else floating: the strike is the extremum itself)
    bool put;
    bool continuous;   // the Brownian-bridge extremum between the step ends (else the step ends alone)
    double K;          // fixed strike
    double v2dt;       // v^2 dt, natural-log units squared
    void *d_samples;   // nullable: n_local samples of the path precision
};

// Enqueues the kernel on a grid of one_path_per_thread_grid(n_local) workgroups.  finish.out: where the final record
// goes (device memory, or pinned host memory the device can write); finish.ticket: the context's zeroed arrival
// counter; d_partials: grid x kLookbackRecord doubles.  With finish.n_value >= 0 (the enqueue form) the record is the
// 6-double statistics layout {sum, sumsq, 0, 0, 0, n}: it has no slot for the two step counters, which are then left
// out of the sum.
hipError_t launch_lookback(const LookbackJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                           hipStream_t stream);

}  // namespace mcamd
