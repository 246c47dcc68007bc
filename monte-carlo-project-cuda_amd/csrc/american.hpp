// american.hpp — host-side interface of the least-squares Monte Carlo kernels (american.hip) for the C ABI (capi_american.cpp).
//
// Training: the trajectory store (launch_store, step-major) and then M launches of the backward sweep on the context's
// stream, with no host synchronisation in between.  Launch j (j = M-1 .. 0) solves date j+1's normal equations from
// the record launch j+1 finished, applies date j+1's exercise decision to V, and accumulates date j's record (j == 0:
// the in-sample sums of V).  Pricing: one kernel on the job's shard that re-simulates each path in registers and
// stops it at the first date whose rule says exercise.
#pragma once

#include "launch.hpp"

namespace mcamd {

constexpr int kAmMaxBasis = 4;
constexpr uint32_t kAmMaxDates = 4096;
constexpr int kAmRow = 8;          // coefficient-table row of a date: beta[0..4), regressed flag, d_j, 0, 0
constexpr int kAmRecord = 12;      // sweep record: power sums P_0..P_6 of u, cross sums sum V u^q (q < 4), |I_j|
constexpr int kAmRecordSlot = 16;  // doubles a record slot spans in the workspace
constexpr int kAmPriceRecord = 5;  // pricing record: sum y, sum y^2, n_early, sum t_exercise, n

struct AmJob {
    PathJob path;        // the pricing shard (product form, no window); drift / vol / K / S_start shared with training
    int put;             // MCAMD_PAYOFF_PUT
    int n_basis;         // 2..4
    uint32_t k;          // exercise every k steps
    uint32_t M;          // dates (n_steps / k)
    double r;
    double dt;           // T / n_steps
    uint64_t n_train;    // training paths (stored by launch_store before the sweep)
};

// Workspace sections (byte offsets from a 256-byte aligned base; see mcamd_american_workspace_bytes)
struct AmLayout {
    uint64_t traj, V, table, partials, total;
};
AmLayout american_layout(uint64_t n_train, uint32_t n_steps, uint32_t M, int precision);

// Both passes run on one_path_per_thread_grid (launch.hpp): of n_train the sweep, of n_local the pricing kernel.
// The M sweep launches.  traj: n_steps x n_train stored rows; V: n_train doubles; table: (M + 1) x kAmRow doubles;
// records: two record slots (kAmRecordSlot doubles each; launch j writes slot j & 1, launch 0's is the in-sample
// {sum V, sum V^2}); partials: grid x kAmRecord doubles; ticket: the context's zeroed arrival counter.
hipError_t launch_american_sweep(const AmJob &job, const void *traj, double *V, double *table, double *records,
                                 double *partials, uint32_t grid, unsigned int *ticket, hipStream_t stream);

// The pricing kernel: reads the table the sweep wrote; out receives the kAmPriceRecord doubles (device memory or pinned
// host memory the device can write); d_partials: grid x kAmPriceRecord doubles.
hipError_t launch_american_price(const AmJob &job, const double *table, double *d_partials, uint32_t grid, double *out,
                                 unsigned int *ticket, hipStream_t stream);

}  // namespace mcamd
