// smile.hip — the sum of a smile's per-wavefront records, for gfx950: the second kernel of every smile call, whatever
// model walked the paths (localvol_smile.hip, heston_smile.hip).  The records are smile_device.hpp's.
#include "smile.hpp"
#include "smile_device.hpp"

namespace mcamd {

// One thread per node: the node's entries over the wavefronts, in index order (adjacent threads read adjacent entries).
__global__ __launch_bounds__(kBlock) void smile_finish_kernel(const SmileEntry *__restrict__ rec, uint32_t n_waves,
                                                              uint32_t n_nodes, double *__restrict__ out, double n_value)
{
    const uint32_t node = blockIdx.x * kBlock + threadIdx.x;
    if (node >= n_nodes) return;
    double sum = 0.0, sumsq = 0.0;
#pragma unroll 8
    for (uint32_t w = 0; w < n_waves; ++w) {
        const SmileEntry e = rec[static_cast<uint64_t>(w) * n_nodes + node];
        sum += e.sum;
        sumsq += e.sumsq;
    }
    out[node] = sum;
    out[n_nodes + node] = sumsq;
    if (node == 0 && n_value >= 0.0) out[2 * n_nodes] = n_value;
}

hipError_t launch_smile_finish(const double *d_partials, uint32_t n_waves, uint32_t n_nodes, double *out, double n_value,
                               hipStream_t stream)
{
    if (!d_partials || !out || n_waves == 0 || n_nodes == 0) return hipErrorInvalidValue;
    const uint32_t grid = (n_nodes + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(smile_finish_kernel, dim3(grid), dim3(kBlock), 0, stream,
                       reinterpret_cast<const SmileEntry *>(d_partials), n_waves, n_nodes, out, n_value);
    return hipGetLastError();
}

}  // namespace mcamd
