// localvol_smile.hip — a strike-by-expiry set of vanillas on one set of local-volatility paths, for gfx950 (both path
// precisions).
//
// Definitions (include/mcamd.h, mcamd_price_localvol_smile): the paths are mcamd_price_localvol's without a barrier —
// the same step (localvol_device.hpp: the table in dynamic LDS, the lookup, the carried row, the move) on the same
// Philox subsequence — stopped at the expiry steps s_0 < s_1 < ...; the spot of expiry m is
// S_m = exp_of_logreturn(S0, X_{s_m} exp_scale), as localvol.hip forms S_T.
//
// Walk phase: one path per lane.  The next expiry step is wave-uniform and lives in a scalar register; a Philox block
// that holds no expiry runs the plain unrolled steps, one that holds an expiry (or the end) tests every step.
// Strike phase (smile_device.hpp, shared with heston_smile.hip): at an expiry the wavefront holds 64 spots, one per lane;
// lane k holds strike k, runs over the wavefront's valid paths and adds sum h and sum h^2 of node (m, k) to its own
// 16-byte entry of the wavefront's private record [m][k] in global memory.
// Finish: smile.hip's smile_finish_kernel, one thread per node, sums the entries over the wavefronts in index order.
#include "localvol_smile.hpp"
#include "localvol_device.hpp"
#include "smile_device.hpp"

namespace mcamd {

template <typename T>
struct SmileArgs {
    LvSurface<T> surf;
    T mu_dt, half_dt, sqrt_dt;
    T exp_scale;              // exponent units per natural-log unit (log2 e in fp32, 65536 / ln 2 in fp64)
    T S0;
    int put;
    uint32_t n_expiries, n_strikes;
    uint32_t last_step;       // expiry_steps[n_expiries - 1]: the walk ends there
    uint64_t seed;
    uint64_t path_offset;
    uint64_t n_local;
    T *spots;                 // nullable
    uint32_t expiry_steps[kSmileMaxExpiries];
    T strikes[kSmileMaxStrikes];
};

template <typename T>
__global__ __launch_bounds__(kBlock) void smile_kernel(SmileArgs<T> args, double *__restrict__ partials)
{
    constexpr int NB = Normals<T>::kPerBlock;
    VolPair<T> *tab = reinterpret_cast<VolPair<T> *>(lv_table_lds);
    lv_copy_table(tab, 0, args.surf.table, args.surf.rows.n_entries);
    __syncthreads();
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(args.seed);
    const LvAxis<T> axis = lv_resident(args.surf.axis);
    const T mu_dt = resident_t(args.mu_dt), half_dt = resident_t(args.half_dt), sqrt_dt = resident_t(args.sqrt_dt);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t wave = blockIdx.x * (kBlock / kWave) + wave_in_block;
    const uint32_t n_e = args.n_expiries, n_K = args.n_strikes;
    const bool has_node = lane < n_K;
    const SmileLane<T> ln = smile_lane(args.strikes, args.put, lane, has_node);
    // the wavefront's record: n_e rows of n_K entries
    SmileEntry *rec = reinterpret_cast<SmileEntry *>(partials) + static_cast<uint64_t>(wave) * n_e * n_K;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    const uint32_t last = args.last_step;
    const uint32_t n_blocks = (last + NB - 1) / NB;
    bool first = true;   // wave-uniform: this trip writes the record, later ones add to it
    for (uint64_t i0 = static_cast<uint64_t>(wave) * kWave; first || i0 < args.n_local; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool valid = i < args.n_local;
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
        const uint64_t subsequence = args.path_offset + i;
        T X = T(0);               // ln(S / S0), natural units
        LvRow row{0, 0};
        uint32_t mi = 0;          // the next expiry, wave-uniform
        uint32_t next = args.expiry_steps[0];
        Normals<T> nz;
        auto step = [&](T z) {
            const T s = lv_sigma(X, axis, args.surf.rows, tab, row);
            lv_move(X, s, z, sqrt_dt, half_dt, mu_dt);
        };
        auto expiry = [&]() {
            const T S = exp_of_logreturn(args.S0, X * args.exp_scale, m);
            if (args.spots && valid) args.spots[static_cast<uint64_t>(mi) * args.n_local + i] = S;
            smile_strike_phase(S, count, ln, has_node, first, rec + mi * n_K + lane);
            ++mi;
            next = mi < n_e ? args.expiry_steps[mi] : 0xFFFFFFFFu;
        };
        for (uint32_t kb = 0; kb < n_blocks; ++kb) {
            nz.fill(m, key, subsequence, kb);
            const uint32_t base = kb * NB;
            if (next > base + NB) {   // no expiry inside this block, hence a full one
#pragma unroll
                for (int j = 0; j < NB; ++j) step(nz.z[j]);
            } else {
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    if (base + j < last) {
                        step(nz.z[j]);
                        if (base + j + 1 == next) expiry();
                    }
                }
            }
        }
        first = false;
    }
}

template <typename T>
static hipError_t launch_smile_t(const SmileJob &j, double *d_partials, uint32_t grid, hipStream_t stream)
{
    SmileArgs<T> a;
    lv_walk_args<T>(a, j.walk);
    a.S0 = static_cast<T>(j.S0);
    smile_node_args<T>(a, j.nodes);
    a.spots = static_cast<T *>(j.d_spots);
    const size_t lds_bytes = static_cast<size_t>(a.surf.rows.n_entries) * sizeof(VolPair<T>);
    hipLaunchKernelGGL((smile_kernel<T>), dim3(grid), dim3(kBlock), lds_bytes, stream, a, d_partials);
    return hipGetLastError();
}

hipError_t launch_localvol_smile(const SmileJob &job, double *d_partials, uint32_t grid, hipStream_t stream)
{
    if (!d_partials || grid == 0 || grid > kFoldMaxRecords) return hipErrorInvalidValue;
    if (!lv_grid_ok(job.walk.surface, job.walk.paths.n_steps)) return hipErrorInvalidValue;
    if (!smile_nodes_ok(job.nodes, job.walk.paths.n_steps)) return hipErrorInvalidValue;
    return job.walk.paths.precision == 32 ? launch_smile_t<float>(job, d_partials, grid, stream)
                               : launch_smile_t<double>(job, d_partials, grid, stream);
}

}  // namespace mcamd
