// heston_barrier.hpp — host-side interface of the Heston single-barrier kernels (heston_barrier.hip) for the C ABI
// (capi_heston.cpp).
//
// A kernel walks mcamd_price_heston's paths (include/mcamd.h, mcamd_price_heston_barrier: the same two Philox streams,
// the same full-truncation step) and applies mcamd_price_barrier's hit tests, distances, survival weight and samples
// with b = ln(B / S0) in natural units and, in the bridge factor, the variance v+ the step was taken at.  Its block
// record: {sum y, sum y^2, live lane-steps, counted lane-steps entered with v < 0, sum of v+ over the counted
// lane-steps, wave-steps}.  The wave-steps sit last: the statistics layout of an enqueue keeps n there.
#pragma once

#include "barrier.hpp"
#include "heston.hpp"

namespace mcamd {

constexpr int kHestonBarrierRecord = 6;

struct HestonBarrierJob {
    HestonWalk walk;
    double S0, K, B;
    BarrierForm form;
    void *d_samples;    // nullable: n_local samples of the path precision
    void *d_state;       // nullable: 3 n_local values of the path precision: S_T, the raw v_n, w
};

// Enqueues the kernel on a grid of one_path_per_thread_grid(n_local) workgroups.  finish, d_partials: as
// launch_heston (grid x kHestonBarrierRecord doubles).
hipError_t launch_heston_barrier(const HestonBarrierJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                                 hipStream_t stream);

}  // namespace mcamd
