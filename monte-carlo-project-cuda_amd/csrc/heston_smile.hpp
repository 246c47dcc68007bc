// heston_smile.hpp — host-side interface of the Heston smile kernels (heston_smile.hip) for the C ABI (capi_heston.cpp).
//
// A Heston smile kernel walks mcamd_price_heston's paths (the step of heston_device.hpp on the same two Philox streams),
// stops at the expiry steps and there runs the strike phase of smile_device.hpp, so a path set serves n_e x n_K
// vanillas (include/mcamd.h, mcamd_price_heston_smile).  The nodes, the per-wavefront records, their sum
// (launch_smile_finish), the limits and the launch shape (smile_grid) are smile.hpp's.  A record holds node sums only:
// the scheme's diagnostics (truncated steps, average variance) are mcamd_price_heston's, on the same paths.
#pragma once

#include "heston.hpp"
#include "smile.hpp"

namespace mcamd {

struct HestonSmileJob {
    HestonWalk walk;     // dt = T / n_steps, over the WHOLE n_steps
    double S0;
    SmileNodes nodes;
    void *d_state;       // nullable: 2 n_expiries x n_local values of the path precision: the spots expiry-major, then
                         // the raw variances expiry-major
};

// Enqueues the walk on `grid` workgroups: d_partials receives grid x kSmileWavesPerBlock records of
// smile_record_doubles doubles, every entry written whatever the buffer held.
hipError_t launch_heston_smile(const HestonSmileJob &job, double *d_partials, uint32_t grid, hipStream_t stream);

}  // namespace mcamd
