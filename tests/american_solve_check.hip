// american_solve_check.hip — test helper (built by tests/american_solve_harness.py with the library's own compile
// flags): runs the SHIPPED solver and decision functions of csrc/american_device.hpp, one thread per case, so that
// tests/test_gpu_american_solver.py can compare each call with an exact reference — the arithmetic the GPU runs
// (hipcc's contraction default, the device's division and square root), not a host restatement.  Not part of the
// product.  All pointers are device memory; launchers return the hipDeviceSynchronize status.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "american_device.hpp"

using namespace mcamd;

namespace {

constexpr int kThreads = 256;
constexpr int kRecord = 12;   // the sweep record: P_0..P_6, sum V u^q (q < 4), |I|
constexpr int kBeta = 4;      // row stride of beta, whatever m

inline dim3 grid_for(uint64_t n) { return dim3(static_cast<uint32_t>((n + kThreads - 1) / kThreads)); }

// beta[i][q >= MB] is left as the caller filled it
template <int MB>
__global__ void k_solve(uint64_t n, const double *records, double pivot_min, double *beta, int32_t *ok)
{
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    double b[MB];
#pragma unroll
    for (int q = 0; q < MB; ++q) b[q] = 0.0;
    // pivot_min < 0: the shipped call, with the default threshold; else the same solver under that threshold
    ok[i] = (pivot_min < 0.0 ? am_solve<MB>(records + i * kRecord, b) : am_solve<MB>(records + i * kRecord, b, pivot_min))
                ? 1 : 0;
#pragma unroll
    for (int q = 0; q < MB; ++q) beta[i * kBeta + q] = b[q];
}

// exercised[i]: am_exercise's return; y[i]: what it left in y, started at -1 (untouched when h(S) = 0);
// continuation[i]: am_continuation at u = S / K - 1, evaluated whether or not h(S) > 0
template <int MB>
__global__ void k_decide(uint64_t n, const double *beta, const double *disc, const double *K, int put, const double *S,
                         int32_t *exercised, double *y, double *continuation)
{
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    double b[MB];
#pragma unroll
    for (int q = 0; q < MB; ++q) b[q] = beta[i * kBeta + q];
    double yy = -1.0;
    exercised[i] = am_exercise<MB>(b, disc[i], K[i], put != 0, S[i], yy) ? 1 : 0;
    y[i] = yy;
    continuation[i] = am_continuation<MB>(b, S[i] / K[i] - 1.0);
}

}  // namespace

extern "C" {

int as_solve(uint64_t n, int m, const double *records, double pivot_min, double *beta, int32_t *ok)
{
    if (n == 0) return 0;
    switch (m) {
    case 2: hipLaunchKernelGGL(k_solve<2>, grid_for(n), dim3(kThreads), 0, 0, n, records, pivot_min, beta, ok); break;
    case 3: hipLaunchKernelGGL(k_solve<3>, grid_for(n), dim3(kThreads), 0, 0, n, records, pivot_min, beta, ok); break;
    case 4: hipLaunchKernelGGL(k_solve<4>, grid_for(n), dim3(kThreads), 0, 0, n, records, pivot_min, beta, ok); break;
    default: return -1;
    }
    return static_cast<int>(hipDeviceSynchronize());
}

int as_decide(uint64_t n, int m, const double *beta, const double *disc, const double *K, int put, const double *S,
              int32_t *exercised, double *y, double *continuation)
{
    if (n == 0) return 0;
    switch (m) {
    case 2:
        hipLaunchKernelGGL(k_decide<2>, grid_for(n), dim3(kThreads), 0, 0, n, beta, disc, K, put, S, exercised, y,
                           continuation);
        break;
    case 3:
        hipLaunchKernelGGL(k_decide<3>, grid_for(n), dim3(kThreads), 0, 0, n, beta, disc, K, put, S, exercised, y,
                           continuation);
        break;
    case 4:
        hipLaunchKernelGGL(k_decide<4>, grid_for(n), dim3(kThreads), 0, 0, n, beta, disc, K, put, S, exercised, y,
                           continuation);
        break;
    default: return -1;
    }
    return static_cast<int>(hipDeviceSynchronize());
}

}  // extern "C"
