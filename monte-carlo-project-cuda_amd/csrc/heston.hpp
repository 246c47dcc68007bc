// heston.hpp — host-side interface of the Heston kernels (heston.hip) for the C ABI (capi_heston.cpp).
//
// A Heston kernel walks full-truncation Euler paths of the log-price and its variance (include/mcamd.h,
// mcamd_price_heston), draws the log-price normals of mcamd_price_barrier and mcamd_price_localvol (same Philox stream =
// global path id, blocks 0, 1, ..) and the variance's own normals from blocks 2^63, 2^63 + 1, .. of the same stream, and
// forms one undiscounted European sample per path in fp64.  Its block record:
// {sum y, sum y^2, lane-steps entered with v < 0, sum of the paths' average variance}.
#pragma once

#include "launch.hpp"

namespace mcamd {

constexpr int kHestonRecord = 4;
constexpr int kHestonFullTruncation = 0;   // MCAMD_HESTON_FULL_TRUNCATION

// What every job that walks Heston paths carries: the paths, the drift, the step, the model and the scheme.
struct HestonWalk {
    PathRange paths;
    double mu;           // r - q
    double dt;           // T / n_steps
    double v0, kappa, theta, xi, rho;
    int scheme;          // kHestonFullTruncation
};
// what every launcher of these paths needs of the walk
inline bool heston_walk_ok(const HestonWalk &w)
{
    return w.scheme == kHestonFullTruncation && w.paths.n_steps != 0 && w.paths.n_local != 0;
}

struct HestonJob {
    HestonWalk walk;
    double S0, K;
    bool put;            // h(S) = (K - S)+ (else (S - K)+)
    void *d_samples;     // nullable: n_local samples of the path precision
    void *d_state;       // nullable: 2 n_local values of the path precision, S_T then the raw v_n
};

// Enqueues the kernel on a grid of one_path_per_thread_grid(n_local) workgroups.  finish, d_partials: as
// launch_localvol (grid x kHestonRecord doubles).
hipError_t launch_heston(const HestonJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                         hipStream_t stream);

}  // namespace mcamd
