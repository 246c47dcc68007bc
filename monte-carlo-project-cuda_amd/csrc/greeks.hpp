// greeks.hpp — host-side interface of the in-kernel Greeks (greeks.hip) for the C ABI (capi.cpp).
//
// A Greeks kernel simulates the same paths as mcamd_price_paths (same Philox stream = global path id, same
// arithmetic) and forms six undiscounted samples per path in fp64 — price, delta, gamma, vega, rho, theta — from the
// path-precision state, once per path.  Its block record is the sum and the sum of squares of each: 12 doubles.
// The statistics record a launch leaves behind is 16 doubles: [0..12) the six (sum, sumsq) pairs in that order,
// [12] = n, [13..16) = 0.
#pragma once

#include "launch.hpp"
#include "mcamd.h"

namespace mcamd {

constexpr int kGreeks = 6;                 // price, delta, gamma, vega, rho, theta
constexpr int kGreeksRecord = 2 * kGreeks; // block record: (sum, sumsq) of each
constexpr int kGreeksStats = 16;           // statistics record: the record, n, zeros

// The estimators' constants, in fp64 (host-computed once per call).  Notation of include/mcamd.h: S_s the start
// price of the simulated segment, T_h = n_sim dt the simulated horizon, L = ln(S_T / S_s).
struct GreeksConsts {
    double K, S_s, T, r, v;
    double T_h;         // n_sim * dt
    double mu_h;        // (r - v^2/2) T_h
    double nu_h;        // (r + v^2/2) T_h
    double gamma_pw;    // 1 / (S_s^2 v^2 T_h)
    double theta_mu;    // r - v^2/2
    double theta_mu_T;  // (r - v^2/2) T
    double inv_2T;      // 1 / (2 T)
    double inv_scale;   // natural log per exponent unit of the path precision (ln 2 for fp32, 1 / kExpScale for fp64)
    double sqrt_dt;
    double delta_lr;    // 1 / (S_s v sqrt(dt))
    double gamma_lr1;   // 1 / (S_s^2 v^2 dt)
    double gamma_lr2;   // 1 / (S_s^2 v sqrt(dt))
    int theta_on;       // pathwise theta is defined (Tk == 0 and dt == T / n_steps); the host reports NaN otherwise
};

struct GreeksJob {
    PathJob path;       // window, restart triple, seed, shard (vr = 0, logspace = true)
    GreeksConsts g;
    bool lr;            // likelihood-ratio kernel (else pathwise: window-less only)
};

// The estimator a Greeks request runs and whether its theta is defined.  AUTO is pathwise without a window and likelihood
// ratio with one; pathwise with a window, or an unknown method, is refused (method = 0).  Pathwise theta differentiates
// the whole horizon, so it is defined only from t = 0 (Tk == 0) with dt = T / n_steps; the host reports NaN otherwise.
struct GreeksRule {
    int method;
    int theta_defined;
};
inline GreeksRule greeks_rule(const mcamd_option &opt, int method)
{
    int used = 0;
    if (method == MCAMD_GREEKS_AUTO) used = opt.use_window ? MCAMD_GREEKS_LIKELIHOOD_RATIO : MCAMD_GREEKS_PATHWISE;
    else if (method == MCAMD_GREEKS_PATHWISE) used = opt.use_window ? 0 : MCAMD_GREEKS_PATHWISE;
    else if (method == MCAMD_GREEKS_LIKELIHOOD_RATIO) used = method;
    return {used, (used == MCAMD_GREEKS_PATHWISE && opt.Tk == 0 && opt.dt == 0.0) ? 1 : 0};
}

// Launch shape: the pathwise kernel takes price_grid's shape of the window-less pair-sum loop, the LR kernel that of
// one path per thread; both are capped at kFoldMaxRecords workgroups (they grid-stride beyond), so the kernel always
// finishes its own sum.
uint32_t greeks_grid(const GreeksJob &job);

// Enqueues the Greeks kernel.  out: where the final 16-double statistics record goes (device memory, or pinned host
// memory the device can write); ticket: the context's zeroed arrival counter; d_partials: grid x kGreeksRecord doubles.
hipError_t launch_greeks(const GreeksJob &job, double *d_partials, uint32_t grid, double *out, unsigned int *ticket,
                         hipStream_t stream);

}  // namespace mcamd
