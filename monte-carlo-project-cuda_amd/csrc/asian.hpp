// asian.hpp — host-side interface of the Asian (average-rate) kernels (asian.hip) for the C ABI (capi_pathdep.cpp).
//
// An Asian kernel walks the paths of mcamd_price_paths (same Philox stream = global path id, same Exponents) and keeps
// what the average needs (include/mcamd.h, mcamd_price_asian): for the arithmetic average the running price in the
// product form of the trajectory-store kernel and the fp64 sum of the step prices, for the geometric average the
// log-return X and the sum L of the X_i in the path precision.  One undiscounted sample per path is formed in fp64.
// The controlled arithmetic job carries both and also forms the geometric sample g of the same strike, payoff and
// include_spot, centred on its known mean.  Its block record is {sum y, sum y^2, sum c, sum c^2, sum y c, wave-steps
// executed}: 6 doubles (c = 0 without the control).
#pragma once

#include "launch.hpp"

namespace mcamd {

constexpr int kAsianRecord = 6;

struct AsianJob {
    PathJob path;        // drift, vol, S_start = S0, n_sim = n_steps, seed, shard, precision (K, B, window, vr unused)
    bool arithmetic;     // the sample averages the prices (else their logarithms: the geometric average)
    bool control;        // arithmetic only: also form the geometric sample, centred on control_mean
    bool floating;       // floating strike: the average is the strike (else the fixed strike K)
    bool put;
    bool include_spot;   // t = 0 is an averaging date
    double K;            // fixed strike
    double control_mean; // E[g]: e^{rT} x the geometric closed form
    void *d_samples;     // nullable: n_local samples of the path precision
};

// Enqueues the kernel on a grid of one_path_per_thread_grid(n_local) workgroups.  finish.out: where the final record
// goes (device memory, or pinned host memory the device can write); finish.ticket: the context's zeroed arrival
// counter; d_partials: grid x kAsianRecord doubles.  With finish.n_value >= 0 (the enqueue form) the record is the
// 6-double statistics layout {sum y, sum y^2, sum c, sum c^2, sum y c, n}: n takes the place of the step counter.
hipError_t launch_asian(const AsianJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                        hipStream_t stream);

}  // namespace mcamd
