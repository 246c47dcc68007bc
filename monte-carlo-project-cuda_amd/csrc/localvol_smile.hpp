// localvol_smile.hpp — host-side interface of the local-volatility smile kernels (localvol_smile.hip) for the C ABI
// (capi_localvol.cpp).
//
// A local-volatility smile kernel walks mcamd_price_localvol's paths without a barrier (the walk of
// localvol_device.hpp), stops at the expiry steps and there runs the strike phase of smile_device.hpp, so a path set
// serves n_e x n_K vanillas (include/mcamd.h, mcamd_price_localvol_smile).  The nodes, the per-wavefront records, their
// sum (launch_smile_finish), the limits and the launch shape (smile_grid) are smile.hpp's.
#pragma once

#include "localvol.hpp"
#include "smile.hpp"

namespace mcamd {

struct SmileJob {
    LocalVolWalk walk;
    double S0;
    SmileNodes nodes;
    void *d_spots;       // nullable: n_expiries x n_local spots of the path precision, expiry-major
};

// Enqueues the walk on `grid` workgroups (n_t n_x sizeof(VolPair) bytes of dynamic LDS): d_partials receives
// grid x kSmileWavesPerBlock records of smile_record_doubles doubles, every entry written whatever the buffer held.
hipError_t launch_localvol_smile(const SmileJob &job, double *d_partials, uint32_t grid, hipStream_t stream);

}  // namespace mcamd
