// autocall.hpp — host-side interface of the worst-of autocallable kernels (autocall.hip) for the C ABI (capi_multi.cpp).
//
// An autocall kernel steps d correlated log-performances per path exactly as a basket kernel does (include/mcamd.h,
// mcamd_price_autocall: same Philox subsequence = the GLOBAL path id, same blocks and slots, same chain of fused
// multiply-adds from the drift) and keeps l = min_j X_j, the log of the worst performance.  At the observation dates
// (every observe_every steps) a path whose l has reached the date's autocall level redeems and is paid pay_q, a double
// from the host's table; a path never called pays 1, or min(A_n, 1) once knocked in.  One sample per path, in maturity
// money.  Its block record is {sum y, sum y^2, paths called, sum of their call times, paths not called and knocked in,
// wave-steps executed, lane-steps of paths not yet called}: 7 doubles.
#pragma once

#include "launch.hpp"
#include "basket.hpp"

namespace mcamd {

constexpr int kAutocallRecord = 7;
constexpr int kAutocallMaxDates = 64;

// The note's terms as both autocall kernels (here and autocall_localvol.hpp) take them, in double and natural-log units.
struct AutocallSchedule {
    uint32_t observe_every;                // steps between observation dates
    uint32_t n_dates;                      // M = n_steps / observe_every, 1..kAutocallMaxDates
    uint32_t first_call_date;              // 1..M: dates before it are not tested
    double log_level[kAutocallMaxDates];   // ln L_q at [q - 1]
    double pay[kAutocallMaxDates];         // pay_q at [q - 1]
    double dt;                             // T / n_steps: t_q = (q observe_every) dt
    bool ki, ki_every_step;                // a knock-in, and whether every step end is monitored (else maturity alone)
    double log_ki;                         // ln ki_level (with a knock-in)
};

// What the launchers refuse: the kernels index the date tables by a counter that these rules bound.
inline bool autocall_schedule_ok(const AutocallSchedule &s, uint32_t n_steps)
{
    return s.observe_every != 0 && s.n_dates != 0 && s.n_dates <= static_cast<uint32_t>(kAutocallMaxDates) &&
           static_cast<uint64_t>(s.n_dates) * s.observe_every == n_steps && s.first_call_date != 0;
}

// Everything in double and in natural-log units; the launcher narrows to the path precision and its exponent units.
struct AutocallJob {
    PathJob path;                          // n_sim = n_steps, seed, shard, precision (the single-asset fields are unused)
    int d;                                 // assets, 1..kBasketMaxAssets
    double drift[kBasketMaxAssets];        // (r - v_j^2 / 2) dt
    double coef[kBasketMaxCoefs];          // v_j sqrt(dt) L_jk at [j (j + 1) / 2 + k], k <= j
    AutocallSchedule schedule;
    void *d_samples;                       // nullable: n_local samples of the path precision
};

// Enqueues the kernel on a grid of one_path_per_thread_grid(n_local) workgroups.  finish.out: where the final record
// goes (device memory, or pinned host memory the device can write); finish.ticket: the context's zeroed arrival
// counter; d_partials: grid x kAutocallRecord doubles.  With finish.n_value >= 0 (the enqueue form) the record is the
// 6-double statistics layout {sum, sumsq, n_called, sum_t_call, n_knocked_in, n}: it has no slot for the two step
// counters, which are then left out.
hipError_t launch_autocall(const AutocallJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                           hipStream_t stream);

}  // namespace mcamd
