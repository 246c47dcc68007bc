// localvol_smile.hpp — host-side interface of the smile kernels (localvol_smile.hip) for the C ABI (capi_localvol.cpp).
//
// A smile kernel walks mcamd_price_localvol's paths without a barrier (the walk of localvol_device.hpp), stops at up to 32
// expiry steps and there turns the work a quarter-turn: every lane of a wavefront takes one strike and runs over the
// wavefront's 64 spots, so a path set serves n_e x n_K vanillas (include/mcamd.h, mcamd_price_localvol_smile).  Every
// wavefront owns a private record [m][k] of (sum h, sum h^2) pairs in global memory; a second kernel sums the records in
// wavefront order.
#pragma once

#include "localvol.hpp"

namespace mcamd {

constexpr uint32_t kSmileMaxStrikes = 64;    // one strike per lane of a wavefront
constexpr uint32_t kSmileMaxExpiries = 32;
constexpr uint32_t kSmileWavesPerBlock = kBlockThreads / 64;
// the per-wavefront records of one launch stay within this many bytes: 512 workgroups at 32 x 64 nodes
constexpr uint64_t kSmilePartialsBudget = 64ull << 20;

struct SmileJob {
    LocalVolWalk walk;
    double S0;
    bool put;            // h(S) = (K - S)+ at every node (else (S - K)+)
    uint32_t n_expiries, n_strikes;
    uint32_t expiry_steps[kSmileMaxExpiries];   // strictly ascending, 1 .. n_steps
    double strikes[kSmileMaxStrikes];
    void *d_spots;       // nullable: n_expiries x n_local spots of the path precision, expiry-major
};

// doubles of one wavefront's record
inline uint32_t smile_record_doubles(uint32_t n_expiries, uint32_t n_strikes) { return 2u * n_expiries * n_strikes; }

// Workgroups of a launch: one_path_per_thread_grid, capped so that the records stay within kSmilePartialsBudget, but
// never below one workgroup per compute unit (compute_units 0: 256).
inline uint32_t smile_grid(uint64_t n_local, uint32_t n_expiries, uint32_t n_strikes, uint32_t compute_units)
{
    const uint64_t per_block = static_cast<uint64_t>(kSmileWavesPerBlock) * smile_record_doubles(n_expiries, n_strikes) * 8;
    uint64_t cap = kSmilePartialsBudget / per_block;
    const uint64_t cus = compute_units ? compute_units : 256;
    if (cap < cus) cap = cus;
    const uint32_t want = one_path_per_thread_grid(n_local);
    return want < cap ? want : static_cast<uint32_t>(cap);
}

// Enqueues the walk on `grid` workgroups (n_t n_x sizeof(VolPair) bytes of dynamic LDS): d_partials receives
// grid x kSmileWavesPerBlock records of smile_record_doubles doubles, every entry written whatever the buffer held.
hipError_t launch_localvol_smile(const SmileJob &job, double *d_partials, uint32_t grid, hipStream_t stream);

// Enqueues the sum of the records in wavefront order: out[node] = sum, out[n_e n_K + node] = sum of squares, and with
// n_value >= 0 out[2 n_e n_K] = n_value.
hipError_t launch_smile_finish(const double *d_partials, uint32_t n_waves, uint32_t n_nodes, double *out, double n_value,
                               hipStream_t stream);

}  // namespace mcamd
