// localvol_greeks.hpp — host-side interface of the local-volatility Greeks kernel (localvol_greeks.hip) for the C ABI.
//
// The kernel walks mcamd_price_localvol's barrier-less paths and, beside each, the first-order tangents of the walk to
// the spot, to a parallel and a bucketed shift of the surface and to the rate (include/mcamd.h,
// mcamd_price_localvol_greeks), forms 6 + n_buckets samples per path in fp64, and leaves the 28-double record
// {(sum, sumsq) of price, delta, gamma, vega, rho, rho_q; (sum, sumsq) of the eight buckets}.
#pragma once

#include "localvol.hpp"

namespace mcamd {

constexpr int kLvGreeks = 6;              // price, delta, gamma, vega, rho, rho_q
constexpr int kLvGreeksMaxBuckets = 8;
constexpr int kLvGreeksRecord = 2 * (kLvGreeks + kLvGreeksMaxBuckets);   // 28
constexpr int kLvGreeksStats = 32;        // the record, n, zeros

struct LocalVolGreeksJob {
    LocalVolWalk walk;
    double S0, K;
    double T;
    bool put;
    uint32_t n_buckets;   // 0 .. kLvGreeksMaxBuckets
    double gamma_bump;    // eta; 0: no gamma
    double *d_samples;    // nullable: (6 + n_buckets) x n_local doubles, estimator-major
};

// Enqueues the kernel on a grid of one_path_per_thread_grid(n_local) workgroups with n_t n_x sizeof(VolPair) bytes of
// dynamic LDS.  finish.out: the 32-double statistics record ([28] = n_local, [29..32) = 0), which the kernel writes
// itself whatever finish.n_value says; d_partials: grid x kLvGreeksRecord doubles.
hipError_t launch_localvol_greeks(const LocalVolGreeksJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                                  hipStream_t stream);

}  // namespace mcamd
