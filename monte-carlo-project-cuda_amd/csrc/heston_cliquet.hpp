// heston_cliquet.hpp — host-side interface of the Heston cliquet kernels (heston_cliquet.hip) for the C ABI
// (capi_heston.cpp).
//
// A Heston cliquet kernel walks mcamd_price_heston's paths (heston_device.hpp: the same step, the same two normals per
// step) and accumulates mcamd_price_cliquet's payoff from the log-returns between equally spaced reset dates
// (include/mcamd.h, mcamd_price_heston_cliquet): a sum of locally clipped period returns, the compounded clipped
// returns, or the annualised realized variance.  One undiscounted sample per path, formed in fp64 and clipped by the
// global bounds.  Its block record: {sum y, sum y^2, paths on the global floor, paths on the global cap, sum of the
// paths' average variance, lane-steps entered with v < 0}.  The truncation counter sits last because the statistics
// layout of an enqueue puts n into slot 5 (mc_device.hpp write_final).
#pragma once

#include "cliquet.hpp"
#include "heston.hpp"

namespace mcamd {

constexpr int kHestonCliquetRecord = 6;

struct HestonCliquetJob {
    HestonWalk walk;
    int kind;               // kCliquet*
    uint32_t reset_every;    // steps per period; divides n_steps
    uint32_t first_period;   // 1 .. n_steps / reset_every: the first period that counts
    double local_lo, local_hi;     // SUM: the bounds of R_p; COMPOUND: ln(1 + bound), -inf / +inf included; VARIANCE: unread
    double global_lo, global_hi;   // the bounds of A, -inf / +inf: none
    double scale;            // VARIANCE: 1 / (P tau); unread otherwise
    void *d_samples;         // nullable: n_local samples of the path precision
};

// Enqueues the kernel on a grid of one_path_per_thread_grid(n_local) workgroups, no dynamic LDS.  finish, d_partials:
// as launch_heston (grid x kHestonCliquetRecord doubles).
hipError_t launch_heston_cliquet(const HestonCliquetJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                                 hipStream_t stream);

}  // namespace mcamd
