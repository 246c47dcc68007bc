// heston_smile.hip — a strike-by-expiry set of vanillas on one set of Heston paths, for gfx950 (both path precisions).
//
// Definitions (include/mcamd.h, mcamd_price_heston_smile): the paths are mcamd_price_heston's — the same step
// (heston_device.hpp's heston_move) on the same two Philox streams of the path's subsequence, blocks 0, 1, .. for the
// log-price and 2^63, 2^63 + 1, .. for the variance — stopped at the expiry steps s_0 < s_1 < ...; the spot of expiry m
// is S_m = exp_of_logreturn(S0, X_{s_m} exp_scale), as heston.hip forms S_T, and the variance of expiry m is the raw
// v_{s_m}.
//
// Walk phase: one path per lane.  The next expiry step is wave-uniform and lives in a scalar
// register; a block of the walk (two Philox blocks, two Box-Muller fills, as in heston.hip) that holds no expiry runs the
// plain unrolled steps, one that holds an expiry (or the end) tests every step.
// Strike phase (smile_device.hpp, shared by every model's smile kernel): at an expiry the wavefront holds 64 spots, one
// per lane; lane k holds strike k, runs over the wavefront's valid paths and adds sum h and sum h^2 of node (m, k) to
// its own 16-byte entry of the wavefront's private record [m][k] in global memory.
// Finish: smile.hip's smile_finish_kernel.  The record holds node sums only: the truncated steps and the
// average variance of these paths are mcamd_price_heston's to report.
#include "heston_smile.hpp"
#include "heston_device.hpp"
#include "smile_device.hpp"

namespace mcamd {

template <typename T>
struct HestonSmileArgs {
    HestonConsts<T> c;
    T exp_scale;              // exponent units per natural-log unit (log2 e in fp32, 65536 / ln 2 in fp64)
    T v0;
    T S0;
    int put;
    uint32_t n_expiries, n_strikes;
    uint32_t last_step;       // expiry_steps[n_expiries - 1]: the walk ends there
    PathShard shard;
    T *state;                 // nullable: S_m at [m n_local + i], the raw v_{s_m} at [(n_e + m) n_local + i]
    uint32_t expiry_steps[kSmileMaxExpiries];
    T strikes[kSmileMaxStrikes];
};

template <typename T>
__global__ __launch_bounds__(kBlock) void heston_smile_kernel(HestonSmileArgs<T> args, double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(args.shard.seed);
    const HestonConsts<T> c = heston_resident(args.c);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t wave = blockIdx.x * (kBlock / kWave) + wave_in_block;
    const uint32_t n_e = args.n_expiries, n_K = args.n_strikes;
    const uint64_t n_local = args.shard.n_local;
    const bool has_node = lane < n_K;
    const SmileLane<T> ln = smile_lane(args.strikes, args.put, lane, has_node);
    // the wavefront's record: n_e rows of n_K entries
    SmileEntry *rec = reinterpret_cast<SmileEntry *>(partials) + static_cast<uint64_t>(wave) * n_e * n_K;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    const uint32_t last = args.last_step;
    const uint32_t n_blocks = (last + NB - 1) / NB;
    bool first = true;   // wave-uniform: this trip writes the record, later ones add to it
    for (uint64_t i0 = static_cast<uint64_t>(wave) * kWave; first || i0 < n_local; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool valid = i < n_local;
        // the valid lanes are a prefix (path ids grow with the lane): their number is the strike loop's trip count
        const uint32_t count = static_cast<uint32_t>(__builtin_popcountll(__builtin_amdgcn_ballot_w64(valid)));
        if (count == 0) {
            // only a wavefront's first trip can be empty: its record is all zeros (smile_device.hpp)
            if (has_node)
                for (uint32_t mi = 0; mi < n_e; ++mi) rec[mi * n_K + lane] = SmileEntry{0.0, 0.0};
            first = false;
            continue;
        }
        // lanes past the end walk a path nobody reads: the strike phase needs the whole wavefront
        const uint64_t subsequence = args.shard.path_offset + i;
        T X = T(0);               // ln(S / S0), natural units
        T v = args.v0;            // the raw variance
        uint32_t mi = 0;          // the next expiry, wave-uniform
        uint32_t next = args.expiry_steps[0];
        HestonNormals<T> nz;
        auto expiry = [&]() {
            const T S = exp_of_logreturn(args.S0, X * args.exp_scale, m);
            if (args.state && valid) {
                args.state[static_cast<uint64_t>(mi) * n_local + i] = S;
                args.state[static_cast<uint64_t>(n_e + mi) * n_local + i] = v;
            }
            smile_strike_phase(S, count, ln, has_node, first, rec + mi * n_K + lane);
            ++mi;
            next = mi < n_e ? args.expiry_steps[mi] : 0xFFFFFFFFu;
        };
        for (uint32_t kb = 0; kb < n_blocks; ++kb) {
            nz.fill(m, key, subsequence, kb);
            const uint32_t base = kb * NB;
            if (next > base + NB) {   // no expiry inside this block, hence a full one
#pragma unroll
                for (int j = 0; j < NB; ++j) heston_move(X, v, nz.z.z[j], nz.zv.z[j], c);
            } else {
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    if (base + j < last) {
                        heston_move(X, v, nz.z.z[j], nz.zv.z[j], c);
                        if (base + j + 1 == next) expiry();
                    }
                }
            }
        }
        first = false;
    }
}

template <typename T>
static hipError_t launch_heston_smile_t(const HestonSmileJob &j, double *d_partials, uint32_t grid, hipStream_t stream)
{
    HestonSmileArgs<T> a;
    heston_walk_args<T>(a, j.walk);
    a.S0 = static_cast<T>(j.S0);
    smile_node_args<T>(a, j.nodes);
    a.state = static_cast<T *>(j.d_state);
    hipLaunchKernelGGL((heston_smile_kernel<T>), dim3(grid), dim3(kBlock), 0, stream, a, d_partials);
    return hipGetLastError();
}

hipError_t launch_heston_smile(const HestonSmileJob &job, double *d_partials, uint32_t grid, hipStream_t stream)
{
    if (!d_partials || grid == 0 || grid > kFoldMaxRecords) return hipErrorInvalidValue;
    if (!heston_walk_ok(job.walk)) return hipErrorInvalidValue;
    if (!smile_nodes_ok(job.nodes, job.walk.paths.n_steps)) return hipErrorInvalidValue;
    return dispatch_precision(job.walk.paths.precision, [&](auto p) {
        return launch_heston_smile_t<typename decltype(p)::type>(job, d_partials, grid, stream);
    });
}

}  // namespace mcamd
