// neg2log_1k_check.hip — test helper (built by tests/neg2log_1k_harness.py with the library's own compile flags): runs
// f64::neg2log_1k on the device exactly as the pair-sum kernels reach it — the 1024-entry table in LDS, copied by
// MathCtx<double>::init<true>() — for arguments the test supplies, so tests/test_gpu_neg2log_1k.py can compare the
// bits with the host build of the same header.  Not part of the product.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mc_device.hpp"

using namespace mcamd;

namespace {

constexpr int kThreads = 256;

// every thread of the workgroup calls init (it holds a barrier) before the bounds check
__global__ void k_neg2log_1k(uint64_t n, const double *u, double *a)
{
    const MathCtx<double> m = MathCtx<double>::init<true>();
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    a[i] = f64::neg2log_1k(u[i], m.t.log_tab);
}

}  // namespace

extern "C" int n1k_eval(uint64_t n, const double *u, double *a)
{
    const dim3 grid(static_cast<uint32_t>((n + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(k_neg2log_1k, grid, dim3(kThreads), 0, 0, n, u, a);
    return static_cast<int>(hipDeviceSynchronize());
}
