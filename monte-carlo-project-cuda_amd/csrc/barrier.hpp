// barrier.hpp — host-side interface of the single-barrier kernels (barrier.hip) for the C ABI (capi_pathdep.cpp), and
// what every model's barrier launcher shares: the form of a barrier job, its dispatch to template arguments and the
// units of the bridge factor.
//
// A barrier kernel walks the log-space paths of mcamd_price_paths (same Philox stream = global path id, same
// Exponents), keeps each path's survival weight w (barrier_device.hpp) and forms one undiscounted sample per path in
// fp64: w h(S_T) for a knock-out, (1 - w) h(S_T) for a knock-in.  Its block record is
// {sum y, sum y^2, wave-steps executed, lane-steps of paths not yet knocked}: 4 doubles.
#pragma once

#include "launch.hpp"

#include <type_traits>

namespace mcamd {

constexpr int kBarrierRecord = 4;

// What a barrier job is beside its model: as BarrierJob, LocalVolJob and HestonBarrierJob carry it.
struct BarrierForm {
    bool up;           // the barrier lies above the spot (else below)
    bool out;          // knock-out (else knock-in)
    bool continuous;   // Brownian-bridge survival factors between the step ends (else the step ends alone)
    bool put;          // h(S) = (K - S)+ (else (S - K)+)
};

// The barrier kernels take the side, the monitoring and the kind as template arguments:
// f(up, continuous, out) with three std::integral_constant<bool, ..> values.
template <typename F>
auto dispatch_bool(bool b, F f)
{
    return b ? f(std::true_type{}) : f(std::false_type{});
}
template <typename F>
auto dispatch_barrier_form(const BarrierForm &form, F f)
{
    return dispatch_bool(form.up, [&](auto up) {
        return dispatch_bool(form.continuous, [&](auto continuous) {
            return dispatch_bool(form.out, [&](auto out) { return f(up, continuous, out); });
        });
    });
}

// The units of the bridge factor's q (barrier_device.hpp): the natural log per unit of q (the fp32 factor is
// 1 - 2^-q, the fp64 one 1 - e^-q) and the cut Q = 18 (fp32) or 38 (fp64) in that unit.
struct BridgeUnits {
    double q_unit, q_cut;
};
template <typename T>
inline BridgeUnits bridge_units()
{
    const double q_unit = sizeof(T) == 4 ? kLn2 : 1.0;
    return {q_unit, (sizeof(T) == 4 ? 18.0 : 38.0) / q_unit};
}

struct BarrierJob {
    PathJob path;      // drift, vol, K, B, S_start = S0, n_sim = n_steps, seed, shard, precision (window, vr unused)
    BarrierForm form;
    double kq;         // 2 / (v^2 dt), natural-log units
    void *d_samples;   // nullable: n_local samples of the path precision
};

// Enqueues the kernel on a grid of one_path_per_thread_grid(n_local) workgroups.  finish.out: where the final record
// goes (device memory, or pinned host memory the device can write); finish.ticket: the context's zeroed arrival
// counter; d_partials: grid x kBarrierRecord doubles.  With finish.n_value >= 0 (the enqueue form) the record is the
// 6-double statistics layout {sum, sumsq, 0, 0, 0, n}: it has no slot for the two step counters, which are then left
// out of the sum.
hipError_t launch_barrier(const BarrierJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                          hipStream_t stream);

}  // namespace mcamd
