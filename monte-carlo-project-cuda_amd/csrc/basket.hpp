// basket.hpp — host-side interface of the multi-asset kernels (basket.hip) for the C ABI (capi_multi.cpp).
//
// A basket kernel steps d correlated log-prices per path (include/mcamd.h, mcamd_price_basket): step i of asset j is
// x_j = drift_j + sum_{k <= j} coef_jk z_{i,k}, a chain of fused multiply-adds in ascending k that starts from the
// drift, with z_{i,k} normal number i d + k of the path's Philox subsequence (the GLOBAL path id) in the order of
// Normals<T>::z.  The aggregate of the d prices is arithmetic, geometric, their best or their worst; best and worst may
// carry a barrier that is tested at the step ends in log space.  One undiscounted sample per path is formed in fp64.
// Its block record is {sum y, sum y^2, wave-steps executed, lane-steps of paths not yet hit}: 4 doubles.
#pragma once

#include <type_traits>

#include "launch.hpp"

namespace mcamd {

constexpr int kBasketRecord = 4;
constexpr int kBasketMaxAssets = 8;
constexpr int kBasketMaxCoefs = kBasketMaxAssets * (kBasketMaxAssets + 1) / 2;

// The kernels of d correlated assets take d as a template argument: f(std::integral_constant<int, D>{}) with D = d.
template <typename F>
hipError_t dispatch_assets(int d, F f)
{
    switch (d) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return hipErrorInvalidValue;
    }
}
static_assert(kBasketMaxAssets == 8, "dispatch_assets lists the asset counts");

enum BasketKind { kBasketArithmetic = 0, kBasketGeometric = 1, kBasketBestOf = 2, kBasketWorstOf = 3 };

// Everything in double and in natural-log units; the launcher narrows to the path precision and its exponent units.
struct BasketJob {
    PathJob path;                    // n_sim = n_steps, seed, shard, precision (the single-asset fields are unused)
    int d;                           // assets, 1..kBasketMaxAssets
    int kind;                        // BasketKind
    bool put;
    bool monitored, up, out;         // a barrier on the aggregate (best-of / worst-of only), its side and its effect
    double drift[kBasketMaxAssets];  // (r - v_j^2 / 2) dt
    double coef[kBasketMaxCoefs];    // v_j sqrt(dt) L_jk at [j (j + 1) / 2 + k], k <= j: the lower Cholesky factor's rows
    double S0[kBasketMaxAssets];     // arithmetic: the spots
    double w[kBasketMaxAssets];      // arithmetic and geometric: the weights
    double log_w[kBasketMaxAssets];  // best-of / worst-of: ln(w_j S0_j); geometric: [0] = sum_j w_j ln S0_j
    double K;
    double logB;                     // ln B (monitored)
    void *d_samples;                 // nullable: n_local samples of the path precision
};

// Enqueues the kernel on a grid of one_path_per_thread_grid(n_local) workgroups.  finish.out: where the final record
// goes (device memory, or pinned host memory the device can write); finish.ticket: the context's zeroed arrival
// counter; d_partials: grid x kBasketRecord doubles.  With finish.n_value >= 0 (the enqueue form) the record is the
// 6-double statistics layout {sum, sumsq, 0, 0, 0, n}: it has no slot for the two step counters, which are then left
// out of the sum.
hipError_t launch_basket(const BasketJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                         hipStream_t stream);

}  // namespace mcamd
