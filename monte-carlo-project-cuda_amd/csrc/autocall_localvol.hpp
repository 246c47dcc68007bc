// autocall_localvol.hpp — host-side interface of the worst-of autocallable kernels under per-asset local-volatility
// surfaces (autocall_localvol.hip, autocall_localvol_f32.hip) for the C ABI (capi_localvol.cpp).
//
// A kernel steps d correlated log-performances per path (include/mcamd.h, mcamd_price_autocall_localvol): asset j looks
// its volatility up at its own X_j in its own surface table, exactly as a local-volatility kernel does, and moves by the
// log-Euler step of localvol.hip with the correlated normal w_j = sum_{k <= j} l_jk z_k in the place of z — the z of
// mcamd_price_basket's stream (Philox subsequence = the GLOBAL path id, normal i d + k).  The dates, levels, payments,
// knock-in modes, samples and the 7-double block record are those of autocall.hpp; everything is in NATURAL-log units.
#pragma once

#include "launch.hpp"
#include "autocall.hpp"
#include "localvol.hpp"

namespace mcamd {

// Everything in double and in natural-log units; the launcher narrows to the path precision.
struct AutocallLocalVolJob {
    PathRange paths;
    int d;                                 // assets, 1..kBasketMaxAssets
    double mu[kBasketMaxAssets];           // r - q_j
    double chol[kBasketMaxCoefs];          // the Cholesky factor of corr at [j (j + 1) / 2 + k], k <= j
    LocalVolGrid surface[kBasketMaxAssets];   // asset j's; sum_j n_t n_x <= kLocalVolMaxNodes
    AutocallSchedule schedule;             // its dt = T / n_steps is the step's as well
    void *d_samples;                       // nullable: n_local samples of the path precision
};

// Enqueues the kernel on a grid of one_path_per_thread_grid(n_local) workgroups with (sum_j n_t n_x) sizeof(VolPair)
// bytes of dynamic LDS.  finish, d_partials: as launch_autocall (grid x kAutocallRecord doubles).
hipError_t launch_autocall_localvol(const AutocallLocalVolJob &job, double *d_partials, uint32_t grid,
                                    const FinishSpec &finish, hipStream_t stream);
// the two precisions, one translation unit each (the job has been checked by launch_autocall_localvol)
hipError_t launch_autocall_localvol_f64(const AutocallLocalVolJob &job, double *d_partials, uint32_t grid,
                                        const FinishSpec &finish, hipStream_t stream);
hipError_t launch_autocall_localvol_f32(const AutocallLocalVolJob &job, double *d_partials, uint32_t grid,
                                        const FinishSpec &finish, hipStream_t stream);

}  // namespace mcamd
