// cliquet.hpp — host-side interface of the cliquet kernels (cliquet.hip) for the C ABI (capi_localvol.cpp).
//
// A cliquet kernel walks mcamd_price_localvol's paths (localvol_device.hpp: the same surface, lookup, row carry,
// log-Euler move and normals) and accumulates a payoff from the log-returns between equally spaced reset dates
// (include/mcamd.h, mcamd_price_cliquet): a sum of locally clipped period returns, the compounded clipped returns, or the
// annualised realized variance.  One undiscounted sample per path, formed in fp64 and clipped by the global bounds.  Its
// block record: {sum y, sum y^2, paths on the global floor, paths on the global cap, wave-steps executed}.
#pragma once

#include "localvol.hpp"

namespace mcamd {

constexpr int kCliquetRecord = 5;
constexpr int kCliquetSum = 0, kCliquetCompound = 1, kCliquetVariance = 2;   // MCAMD_CLIQUET_*

struct CliquetJob {
    LocalVolWalk walk;
    int kind;                // kCliquet*
    uint32_t reset_every;    // steps per period; divides n_steps
    uint32_t first_period;   // 1 .. n_steps / reset_every: the first period that counts
    double local_lo, local_hi;     // SUM: the bounds of R_p; COMPOUND: ln(1 + bound), -inf / +inf included; VARIANCE: unread
    double global_lo, global_hi;   // the bounds of A, -inf / +inf: none
    double scale;            // VARIANCE: 1 / (P tau); unread otherwise
    void *d_samples;         // nullable: n_local samples of the path precision
};

// Enqueues the kernel on a grid of one_path_per_thread_grid(n_local) workgroups with n_t n_x sizeof(VolPair) bytes of
// dynamic LDS.  finish, d_partials: as launch_localvol (grid x kCliquetRecord doubles).
hipError_t launch_cliquet(const CliquetJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                          hipStream_t stream);

}  // namespace mcamd
