// finish_check.hip — test helper (built by tests/finish_harness.py with the library's own compile flags and linked
// against the built library): runs the SHIPPED record finish — wave_sum / block_sumN / block_sum2, small_final_sum,
// finish_paths (block sum, release, ticket, acquire, last workgroup's sum), write_final of csrc/mc_device.hpp and
// csrc/path_frame.hpp, and the library's launch_small_final, launch_final_reduce, launch_smile_finish — on records the
// test supplies, so tests/test_gpu_finish.py can compare every sum with tests/finish_restate.py.  Nothing here walks a
// path.  Not part of the product.
//
// Every launcher returns the first HIP error it met (0: none) after synchronising its stream.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "launch.hpp"
#include "mc_device.hpp"
#include "path_frame.hpp"
#include "smile.hpp"

using namespace mcamd;

namespace {

#define FC_TRY(expr)                       \
    do {                                   \
        const hipError_t e_ = (expr);      \
        if (e_ != hipSuccess) return static_cast<int>(e_); \
    } while (0)

// ---- 1. block sums: workgroup b sums in[b][BLOCK][N]; ONEHOT: only thread b of workgroup b holds vals[b][.] ----------
template <int BLOCK, int N, bool SUM2, bool ONEHOT>
__global__ __launch_bounds__(BLOCK) void k_block_sum(const double *__restrict__ in, double *__restrict__ out)
{
    double v[N];
    const uint64_t at = ONEHOT ? blockIdx.x : static_cast<uint64_t>(blockIdx.x) * BLOCK + threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (!ONEHOT || threadIdx.x == blockIdx.x) ? in[at * N + k] : 0.0;
    if constexpr (SUM2) {
        static_assert(N == 2, "block_sum2 sums a pair");
        block_sum2<BLOCK>(v[0], v[1]);
    } else {
        block_sumN<BLOCK, N>(v);
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) out[static_cast<uint64_t>(blockIdx.x) * N + k] = v[k];
    }
}

template <int BLOCK, int N, bool SUM2 = false>
void block_sum_launch(uint32_t n_blocks, bool onehot, const double *in, double *out, hipStream_t s)
{
    if (onehot)
        hipLaunchKernelGGL((k_block_sum<BLOCK, N, SUM2, true>), dim3(BLOCK), dim3(BLOCK), 0, s, in, out);
    else
        hipLaunchKernelGGL((k_block_sum<BLOCK, N, SUM2, false>), dim3(n_blocks), dim3(BLOCK), 0, s, in, out);
}

// ---- 2. small_final_sum: workgroup b sums the first counts[b] records of rec ------------------------------------------
template <int N, int ACC>
__global__ __launch_bounds__(kBlock) void k_small_final(const double *__restrict__ rec, const uint32_t *__restrict__ counts,
                                                        double *__restrict__ out)
{
    double v[N];
    small_final_sum<kBlock, N, ACC>(rec, counts[blockIdx.x], v);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) out[static_cast<uint64_t>(blockIdx.x) * N + k] = v[k];
    }
}

// ---- 3. the hand-off: thread b % 256 of workgroup b holds rec[b][.] + round_add, every other thread 0; the eight
// workgroups (first_late + j) % grid, j = 0..7, sleep a fixed 1 + j times ~1 us before they publish ---------------------
template <int N, int ACC>
__global__ __launch_bounds__(kBlock) void k_handoff(const double *__restrict__ rec, double round_add, uint32_t first_late,
                                                    double *__restrict__ partials, GridFinish fin)
{
    double acc[N];
    const bool hot = threadIdx.x == blockIdx.x % kBlock;
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = hot ? rec[static_cast<uint64_t>(blockIdx.x) * N + k] + round_add : 0.0;
    const uint32_t j = (blockIdx.x + gridDim.x - first_late % gridDim.x) % gridDim.x;
    if (j < 8)
        for (uint32_t it = 0; it <= j; ++it) __builtin_amdgcn_s_sleep(32);   // 32 x 64 clocks; no condition on memory
    finish_paths<N, ACC>(acc, partials, fin);
}

template <int N, int ACC>
void handoff_launch(uint32_t grid, const double *rec, double round_add, uint32_t first_late, double *partials,
                    const GridFinish &fin, hipStream_t s)
{
    hipLaunchKernelGGL((k_handoff<N, ACC>), dim3(grid), dim3(kBlock), 0, s, rec, round_add, first_late, partials, fin);
}

// ---- 4. write_final, by one thread ------------------------------------------------------------------------------------
__global__ void k_write_final(const double *__restrict__ v, int n, double n_value, double *__restrict__ out)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) write_final(out, v, n, n_value);
}

struct Stream {
    hipStream_t s = nullptr;
    hipError_t made;
    Stream() : made(hipStreamCreate(&s)) {}
    ~Stream()
    {
        if (s) (void)hipStreamDestroy(s);
    }
    int done() { return static_cast<int>(hipStreamSynchronize(s)); }
};

}  // namespace

extern "C" {

// in: [n_blocks][block][n] (onehot: [block][n], one workgroup per hot lane); out: [n_blocks or block][n]; sum2: block_sum2
int fc_block_sum(int block, int n, int sum2, int onehot, uint32_t n_blocks, const double *in, double *out)
{
    Stream st;
    FC_TRY(st.made);
    const bool oh = onehot != 0;
    const int key = block * 100 + n + (sum2 ? 50 : 0);
    switch (key) {
    case 25602: block_sum_launch<256, 2>(n_blocks, oh, in, out, st.s); break;
    case 25652: block_sum_launch<256, 2, true>(n_blocks, oh, in, out, st.s); break;
    case 25603: block_sum_launch<256, 3>(n_blocks, oh, in, out, st.s); break;
    case 25604: block_sum_launch<256, 4>(n_blocks, oh, in, out, st.s); break;
    case 25605: block_sum_launch<256, 5>(n_blocks, oh, in, out, st.s); break;
    case 25606: block_sum_launch<256, 6>(n_blocks, oh, in, out, st.s); break;
    case 25607: block_sum_launch<256, 7>(n_blocks, oh, in, out, st.s); break;
    case 25612: block_sum_launch<256, 12>(n_blocks, oh, in, out, st.s); break;
    case 25628: block_sum_launch<256, 28>(n_blocks, oh, in, out, st.s); break;
    case 102402: block_sum_launch<1024, 2>(n_blocks, oh, in, out, st.s); break;
    case 102404: block_sum_launch<1024, 4>(n_blocks, oh, in, out, st.s); break;
    case 102405: block_sum_launch<1024, 5>(n_blocks, oh, in, out, st.s); break;
    default: return static_cast<int>(hipErrorInvalidValue);
    }
    FC_TRY(hipGetLastError());
    return st.done();
}

// out[b][n] = small_final_sum<256, n, acc> of the first counts[b] records of rec, one workgroup per count
int fc_small_final_sum(int n, int acc, const double *rec, const uint32_t *counts, uint32_t n_counts, double *out)
{
    Stream st;
    FC_TRY(st.made);
    const dim3 g(n_counts), b(kBlock);
    switch (n * 10 + acc) {
    case 24: hipLaunchKernelGGL((k_small_final<2, 4>), g, b, 0, st.s, rec, counts, out); break;
    case 44: hipLaunchKernelGGL((k_small_final<4, 4>), g, b, 0, st.s, rec, counts, out); break;
    case 54: hipLaunchKernelGGL((k_small_final<5, 4>), g, b, 0, st.s, rec, counts, out); break;
    case 64: hipLaunchKernelGGL((k_small_final<6, 4>), g, b, 0, st.s, rec, counts, out); break;
    case 74: hipLaunchKernelGGL((k_small_final<7, 4>), g, b, 0, st.s, rec, counts, out); break;
    case 124: hipLaunchKernelGGL((k_small_final<12, 4>), g, b, 0, st.s, rec, counts, out); break;
    case 281: hipLaunchKernelGGL((k_small_final<28, 1>), g, b, 0, st.s, rec, counts, out); break;
    default: return static_cast<int>(hipErrorInvalidValue);
    }
    FC_TRY(hipGetLastError());
    return st.done();
}

// `rounds` launches of k_handoff<n, acc> back to back on one stream, no host synchronisation between them, all on one
// partials array and one ticket: launch r adds r * add_unit to every record, delays the workgroups (3 r + j) % grid and
// writes its final record to row r (row_doubles apart) of `rows` — device memory, or with pinned != 0 pinned host memory
// of this call's own (through its device pointer), copied to the HOST buffer `rows` after the one synchronisation.
int fc_handoff(int n, int acc, uint32_t grid, uint32_t rounds, const double *rec, double add_unit, double n_value,
               double *partials, unsigned int *ticket, double *rows, uint32_t row_doubles, int pinned)
{
    if (grid == 0 || grid > kFoldMaxRecords || rounds == 0 || row_doubles < static_cast<uint32_t>(n < 6 ? 6 : n))
        return static_cast<int>(hipErrorInvalidValue);
    Stream st;
    FC_TRY(st.made);
    const size_t bytes = sizeof(double) * row_doubles * rounds;
    double *h_rows = nullptr, *d_rows = rows;
    if (pinned) {
        FC_TRY(hipHostMalloc(reinterpret_cast<void **>(&h_rows), bytes, hipHostMallocDefault));
        memcpy(h_rows, rows, bytes);   // the caller's poison
        const hipError_t e = hipHostGetDevicePointer(reinterpret_cast<void **>(&d_rows), h_rows, 0);
        if (e != hipSuccess) {
            (void)hipHostFree(h_rows);
            return static_cast<int>(e);
        }
    }
    hipError_t err = hipSuccess;
    for (uint32_t r = 0; r < rounds && err == hipSuccess; ++r) {
        const GridFinish fin{d_rows + static_cast<size_t>(r) * row_doubles, ticket, n_value};
        const double add = static_cast<double>(r) * add_unit;
        switch (n * 10 + acc) {
        case 24: handoff_launch<2, 4>(grid, rec, add, 3 * r, partials, fin, st.s); break;
        case 44: handoff_launch<4, 4>(grid, rec, add, 3 * r, partials, fin, st.s); break;
        case 54: handoff_launch<5, 4>(grid, rec, add, 3 * r, partials, fin, st.s); break;
        case 64: handoff_launch<6, 4>(grid, rec, add, 3 * r, partials, fin, st.s); break;
        case 281: handoff_launch<28, 1>(grid, rec, add, 3 * r, partials, fin, st.s); break;
        default: err = hipErrorInvalidValue; break;
        }
        if (err == hipSuccess) err = hipGetLastError();
    }
    const hipError_t sync = hipStreamSynchronize(st.s);
    if (err == hipSuccess) err = sync;
    if (pinned) {
        if (err == hipSuccess) memcpy(rows, h_rows, bytes);
        (void)hipHostFree(h_rows);
    }
    return static_cast<int>(err);
}

// out (8 doubles the caller poisoned) after write_final(out, v, n, n_value)
int fc_write_final(const double *v, int n, double n_value, double *out)
{
    Stream st;
    FC_TRY(st.made);
    hipLaunchKernelGGL(k_write_final, dim3(1), dim3(64), 0, st.s, v, n, n_value, out);
    FC_TRY(hipGetLastError());
    return st.done();
}

// which: 0 launch_small_final, 1 launch_final_reduce.  One launch per counts[c] on one stream, the first counts[c]
// records of rec into out + c * row_doubles; *status: what the launcher returned for the first count (all alike).
// After a refused width the same stream takes a launch of width 2 into `after` (8 doubles), which must succeed.
int fc_library_sum(int which, const double *rec, const uint32_t *counts, uint32_t n_counts, int width, double n_value,
                   double *out, uint32_t row_doubles, int *status, double *after)
{
    Stream st;
    FC_TRY(st.made);
    *status = 0;
    for (uint32_t c = 0; c < n_counts; ++c) {
        double *o = out + static_cast<size_t>(c) * row_doubles;
        const hipError_t e = which == 0 ? launch_small_final(rec, counts[c], width, o, st.s, n_value)
                                        : launch_final_reduce(rec, counts[c], width, o, st.s, n_value);
        if (e != hipSuccess) {
            *status = static_cast<int>(e);
            break;
        }
    }
    if (*status != 0 && after != nullptr) {
        FC_TRY(which == 0 ? launch_small_final(rec, counts[0], 2, after, st.s, -1.0)
                          : launch_final_reduce(rec, counts[0], 2, after, st.s, -1.0));
    }
    return st.done();
}

// launch_smile_finish on partials [n_waves][n_nodes] (sum, sumsq) entries, 16-byte aligned
int fc_smile_finish(const double *partials, uint32_t n_waves, uint32_t n_nodes, double *out, double n_value, int *status)
{
    Stream st;
    FC_TRY(st.made);
    *status = static_cast<int>(launch_smile_finish(partials, n_waves, n_nodes, out, n_value, st.s));
    return st.done();
}

}  // extern "C"
