// american_dual.hpp — host-side interface of the Andersen-Broadie dual (upper) bound kernels (american_dual.hip) for the
// C ABI (capi_american.cpp).
//
// The shard's outer paths are stored by launch_store (step-major, product form).  The continuation kernel then prices
// every point (p, j), j = 0..M-1, by n_inner paths that follow the fitted rule from S_{p,j} on, and the scan kernel
// walks each outer path through its dates, forms the martingale and the dual sample, and finishes the sums.
#pragma once

#include "american.hpp"

namespace mcamd {

constexpr int kAmContRecord = 2;   // continuation record: wave-steps executed, lane-steps of paths still live
constexpr int kAmDualRecord = 4;   // scan record: sum u, sum u^2, sum Q_0, n

struct AmDualJob {
    PathJob path;         // the OUTER shard (product form, no window); seed = outer seed
    int put;
    int n_basis;          // 2..4
    uint32_t k;           // exercise every k steps
    uint32_t M;           // dates
    uint32_t n_inner;     // continuation paths per point
    uint64_t inner_seed;
};

// Workspace sections (byte offsets from a 256-byte aligned base; see mcamd_american_dual_workspace_bytes)
struct AmDualLayout {
    uint64_t traj, cont, table, partials, total;
};
AmDualLayout american_dual_layout(uint64_t n_local, uint32_t n_steps, uint32_t M, int precision);

uint32_t american_cont_grid(uint64_t n_points);   // one workgroup per point, capped: the workgroups stride
// (the scan runs on one_path_per_thread_grid(n_local))

// Q[j * n_local + p], j = 0..M-1: the mean of the n_inner continuation samples of point (p, j).  traj: the stored
// outer rows (n_steps x n_local); table: (M + 1) x kAmRow doubles (rows 1..M: beta, flag, d_j, t_j); out receives the
// kAmContRecord doubles; d_partials: grid x kAmContRecord doubles; ticket: the context's zeroed arrival counter.
hipError_t launch_american_cont(const AmDualJob &job, const void *traj, const double *table, double *Q,
                                double *d_partials, uint32_t grid, double *out, unsigned int *ticket,
                                hipStream_t stream);

// The per-path martingale scan: out receives the kAmDualRecord doubles; d_partials: grid x kAmDualRecord doubles.
hipError_t launch_american_dual_scan(const AmDualJob &job, const void *traj, const double *table, const double *Q,
                                     double *d_partials, uint32_t grid, double *out, unsigned int *ticket,
                                     hipStream_t stream);

}  // namespace mcamd
