// localvol.hpp — host-side interface of the local-volatility kernels (localvol.hip) for the C ABI (capi_localvol.cpp).
//
// A local-volatility kernel walks log-Euler paths whose volatility is looked up per step, per lane, in a surface table
// held in LDS (include/mcamd.h, mcamd_price_localvol), draws the normals of mcamd_price_barrier (same Philox stream =
// global path id) and forms one undiscounted sample per path in fp64: h(S_T), or the knock-out / knock-in sample of the
// barrier kernels with the step's own volatility in the bridge factor.  Its block record is the barrier kernels':
// {sum y, sum y^2, wave-steps executed, lane-steps of paths not yet knocked}.
#pragma once

#include "barrier.hpp"

namespace mcamd {

constexpr int kLocalVolRecord = 4;
constexpr uint32_t kLocalVolMaxNodes = 2048;   // n_t n_x: 32 KiB of fp64 pairs beside the 20 KiB of fast64 tables

// One table entry as the kernels read it: one 8-byte (fp32) or 16-byte (fp64) LDS read per step and lane.
template <typename T>
struct alignas(2 * sizeof(T)) VolPair {
    T sigma;   // sigma_k
    T slope;   // sigma_{k+1} - sigma_k (0 at a row's last node, which is never read)
};

// A surface as a job carries it: the grid and the pair table of the job's path precision.
struct LocalVolGrid {
    uint32_t n_t, n_x;
    double x_min, x_max;
    const void *d_table;   // n_t n_x VolPair of the path precision, device memory, 16-byte aligned
};

// What every job that walks one surface carries: the paths, the drift, the step and the surface.
struct LocalVolWalk {
    PathRange paths;
    double mu;           // r - q
    double dt;           // T / n_steps
    LocalVolGrid surface;
};

struct LocalVolJob {
    LocalVolWalk walk;
    double S0, K, B;     // B read with a barrier only
    bool barrier;        // knock-out / knock-in at B (else European: of form, put alone is read)
    BarrierForm form;    // continuous: with the step's frozen volatility in the bridge factor
    void *d_samples;     // nullable: n_local samples of the path precision
};

// Enqueues the kernel on a grid of one_path_per_thread_grid(n_local) workgroups with n_t n_x sizeof(VolPair) bytes of
// dynamic LDS.  finish, d_partials: as launch_barrier (grid x kLocalVolRecord doubles).
hipError_t launch_localvol(const LocalVolJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                           hipStream_t stream);

}  // namespace mcamd
