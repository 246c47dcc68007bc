// smile.hpp — host-side interface of "a smile", whatever model walks the paths: the nodes of a job, the limits, the shape
// of a launch, and the sum of the per-wavefront records (smile.hip) for the C ABI (capi_smile.cpp).
//
// A smile kernel (one file per model, each with a header of its own that includes this one) walks its model's paths,
// stops at up to 32 expiry steps and there turns the work a quarter-turn: every lane of a wavefront takes one strike and
// runs over the wavefront's 64 spots (smile_device.hpp), so a path set serves n_e x n_K vanillas.  Every wavefront owns
// a private record [m][k] of (sum h, sum h^2) pairs in global memory; a second kernel sums the records in wavefront
// order.
#pragma once

#include "launch.hpp"

namespace mcamd {

constexpr uint32_t kSmileMaxStrikes = 64;    // one strike per lane of a wavefront
constexpr uint32_t kSmileMaxExpiries = 32;
constexpr uint32_t kSmileWavesPerBlock = kBlockThreads / 64;
// the per-wavefront records of one launch stay within this many bytes: 512 workgroups at 32 x 64 nodes
constexpr uint64_t kSmilePartialsBudget = 64ull << 20;

// The nodes as a job of either model carries them.
struct SmileNodes {
    bool put;            // h(S) = (K - S)+ at every node (else (S - K)+)
    uint32_t n_expiries, n_strikes;
    uint32_t expiry_steps[kSmileMaxExpiries];   // strictly ascending, 1 .. n_steps
    double strikes[kSmileMaxStrikes];
};

// what a launcher re-checks of the nodes: the counts in range, the expiry steps strictly ascending in 1 .. n_steps
inline bool smile_nodes_ok(const SmileNodes &n, uint32_t n_steps)
{
    if (n.n_expiries < 1 || n.n_expiries > kSmileMaxExpiries || n.n_strikes < 1 || n.n_strikes > kSmileMaxStrikes)
        return false;
    for (uint32_t m = 0; m < n.n_expiries; ++m) {
        const uint32_t lo = m ? n.expiry_steps[m - 1] : 0;
        if (n.expiry_steps[m] <= lo || n.expiry_steps[m] > n_steps) return false;
    }
    return true;
}

// The nodes as a kernel's Args<T> carry them (its members put, n_expiries, n_strikes, last_step, expiry_steps[] and
// strikes[], wherever they lie in it): the walk ends at the last expiry; the expiry steps past n_expiries are 0xFFFFFFFF,
// which no step reaches, and the strikes past n_strikes 0.
template <typename T, typename Args>
inline void smile_node_args(Args &a, const SmileNodes &n)
{
    a.put = n.put ? 1 : 0;
    a.n_expiries = n.n_expiries;
    a.n_strikes = n.n_strikes;
    a.last_step = n.expiry_steps[n.n_expiries - 1];
    for (uint32_t m = 0; m < kSmileMaxExpiries; ++m) a.expiry_steps[m] = m < n.n_expiries ? n.expiry_steps[m] : 0xFFFFFFFFu;
    for (uint32_t k = 0; k < kSmileMaxStrikes; ++k) a.strikes[k] = k < n.n_strikes ? static_cast<T>(n.strikes[k]) : T(0);
}

// doubles of one wavefront's record
inline uint32_t smile_record_doubles(uint32_t n_expiries, uint32_t n_strikes) { return 2u * n_expiries * n_strikes; }

// Workgroups of a launch: one_path_per_thread_grid, capped so that the records stay within kSmilePartialsBudget, but
// never below one workgroup per compute unit (compute_units 0: 256).
inline uint32_t smile_grid(uint64_t n_local, uint32_t n_expiries, uint32_t n_strikes, uint32_t compute_units)
{
    const uint64_t per_block = static_cast<uint64_t>(kSmileWavesPerBlock) * smile_record_doubles(n_expiries, n_strikes) * 8;
    uint64_t cap = kSmilePartialsBudget / per_block;
    const uint64_t cus = compute_units ? compute_units : 256;
    if (cap < cus) cap = cus;
    const uint32_t want = one_path_per_thread_grid(n_local);
    return want < cap ? want : static_cast<uint32_t>(cap);
}

// Enqueues the sum of the records in wavefront order: out[node] = sum, out[n_e n_K + node] = sum of squares, and with
// n_value >= 0 out[2 n_e n_K] = n_value.
hipError_t launch_smile_finish(const double *d_partials, uint32_t n_waves, uint32_t n_nodes, double *out, double n_value,
                               hipStream_t stream);

}  // namespace mcamd
