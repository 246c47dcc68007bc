// heston_greeks.hpp — host-side interface of the Heston Greeks kernel (heston_greeks.hip) for the C ABI
// (capi_heston.cpp).
//
// The kernel walks mcamd_price_heston's path and, on the same two normals of every step, two more (X, v) walks per
// requested model parameter: one at the parameter plus its bump, one at it minus the bump
// (include/mcamd_heston_greeks.h).  Each walk is a HestonWalk of its own, so each is mcamd_price_heston's path at that
// model, bit for bit.  It leaves the record
//     {sum y, sum y^2, sum d, sum d^2, sum (d - y)^2, sum g, sum g^2,
//      (sum c_p, sum c_p^2) per requested parameter in index order,
//      the base walk's lane-steps entered with v < 0, the base walk's sum of the paths' average variance}
// of 9 + 2 P doubles, and writes the path count behind it and zeros up to the 32 doubles of the statistics layout.
#pragma once

#include "heston.hpp"

namespace mcamd {

constexpr int kHestonGreeksMaxParams = 5;    // v0, kappa, theta, xi, rho
constexpr int kHestonGreeksMaxWalks = 1 + 2 * kHestonGreeksMaxParams;
constexpr int kHestonGreeksStats = 32;       // the record, n, zeros
constexpr int heston_greeks_record(int n_params) { return 9 + 2 * n_params; }
constexpr int heston_greeks_rows(int n_params) { return 3 + 2 * n_params; }

struct HestonGreeksJob {
    HestonWalk walk[kHestonGreeksMaxWalks];   // the base walk, then (+, -) per requested parameter in index order
    int n_params;        // P: 0 .. kHestonGreeksMaxParams
    double S0, K;
    bool put;
    double gamma_eta;    // 0: row 2 is all zeros
    void *d_samples;     // nullable: (3 + 2 P) n_local values of the path precision, row-major
};

// Enqueues the kernel on a grid of one_path_per_thread_grid(n_local) workgroups.  finish.out: the 32-double statistics
// record ([9 + 2 P] = n_local, zeros behind it), which the kernel writes itself whatever finish.n_value says;
// d_partials: grid x (9 + 2 P) doubles.  Every walk must share the base walk's paths, drift, step and scheme.
hipError_t launch_heston_greeks(const HestonGreeksJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                                hipStream_t stream);

}  // namespace mcamd
