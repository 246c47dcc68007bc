// localvol_device.hpp — everything a kernel needs to walk one local-volatility surface, shared by localvol.hip,
// localvol_smile.hip, autocall_localvol_impl.hpp and localvol_greeks.hip: the surface's constants and the host function
// that builds them, the table's copy into dynamic LDS, the lookup with its row carry (and, for the Greeks, the lookup
// that hands back the cell's slope as well), and the log-Euler move.
//
// Definitions (include/mcamd.h, mcamd_price_localvol): X = ln(S / S0) in NATURAL-log units (the surface's axis).  Step
// i looks its volatility up at X in row(i) = floor(i n_t / n) of the surface, s = fma(f, slope_k, sigma_k) with
// u = clamp((X - x_min) / dx, 0, n_x - 1), k = min(floor u, n_x - 2), f = u - k, and moves
// X += fma(s sqrt(dt), z, fma(-s^2, dt / 2, mu dt)).  row(i) is carried, not divided out: the row base grows by
// (n_t / n) n_x and a remainder counter carries one more row when it passes n (both wave-uniform, scalar unit).
//
// Why this walk can be shared where the constant-volatility walks are not: every fused operation here is an explicit
// fma_t, and the remaining products, sums and differences feed a clamp, a conversion, an fma_t operand or X itself, so
// there is no a * b + c for the compiler to contract one way in one kernel and another way in the next.
#pragma once

#include "localvol.hpp"
#include "path_consts.hpp"

namespace mcamd {

// The floating-point constants of a surface: in fp32 they go to vector registers once per kernel (lv_resident).
template <typename T>
struct LvAxis {
    T x_min, inv_dx;   // node 0 and 1 / dx
    T u_max;           // n_x - 1
};

// The integer constants: wave-uniform, they stay in scalar registers.
struct LvRows {
    uint32_t k_max;          // n_x - 2
    uint32_t n_x, n_entries; // n_entries = n_t n_x
    uint32_t row_whole_nx;   // (n_t / n_steps) n_x: what the row base grows by at every step
    uint32_t row_rem;        // n_t % n_steps
    uint32_t row_thr;        // n_steps - row_rem: the remainder counter carries when it reaches this
};

template <typename T>
struct LvSurface {
    LvAxis<T> axis;
    LvRows rows;
    const VolPair<T> *table;   // global memory
};

// a grid a kernel can walk in n_steps steps (sum the nodes of several tables before comparing with kLocalVolMaxNodes)
inline bool lv_grid_ok(const LocalVolGrid &g, uint32_t n_steps)
{
    return g.d_table && n_steps != 0 && g.n_x >= 2 && g.n_t >= 1 &&
           static_cast<uint64_t>(g.n_t) * g.n_x <= kLocalVolMaxNodes;
}

template <typename T>
inline LvSurface<T> lv_surface(const LocalVolGrid &g, uint32_t n_steps)
{
    const double dx = (g.x_max - g.x_min) / static_cast<double>(g.n_x - 1);
    LvSurface<T> s;
    s.axis.x_min = static_cast<T>(g.x_min);
    s.axis.inv_dx = static_cast<T>(1.0 / dx);
    s.axis.u_max = static_cast<T>(g.n_x - 1);
    s.rows.k_max = g.n_x - 2;
    s.rows.n_x = g.n_x;
    s.rows.n_entries = g.n_t * g.n_x;
    s.rows.row_whole_nx = (g.n_t / n_steps) * g.n_x;
    s.rows.row_rem = g.n_t % n_steps;
    s.rows.row_thr = n_steps - s.rows.row_rem;
    s.table = static_cast<const VolPair<T> *>(g.d_table);
    return s;
}

// exponent units per natural-log unit (log2 e in fp32, 65536 / ln 2 in fp64): make_consts' literals
template <typename T>
inline T lv_exp_scale()
{
    return static_cast<T>(sizeof(T) == 4 ? 1.4426950408889634 : f64::kExpScale);
}

// What the argument structs of the single-surface kernels (LocalVolArgs, CliquetArgs, LvGreeksArgs, SmileArgs) have in
// common, from the walk of their job.  The structs share no sub-struct for these: each kernel's scalar loads are
// compiled against its own layout.  The one-path-per-thread kernels add their PathShard; lv_walk_args adds the three
// shard fields as the smile kernel carries them.
template <typename T, typename Args>
inline void lv_step_args(Args &a, const LocalVolWalk &w)
{
    a.surf = lv_surface<T>(w.surface, w.paths.n_steps);
    a.mu_dt = static_cast<T>(w.mu * w.dt);
    a.half_dt = static_cast<T>(0.5 * w.dt);
    a.sqrt_dt = static_cast<T>(std::sqrt(w.dt));
    a.exp_scale = lv_exp_scale<T>();
}
template <typename T, typename Args>
inline void lv_walk_args(Args &a, const LocalVolWalk &w)
{
    lv_step_args<T>(a, w);
    a.seed = w.paths.seed;
    a.path_offset = w.paths.path_offset;
    a.n_local = w.paths.n_local;
}

__device__ __forceinline__ float lv_min(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double lv_min(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ float lv_max(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double lv_max(double a, double b) { return __builtin_fmax(a, b); }

// Where the axis' floating-point constants live: where resident_t (mc_device.hpp) keeps the step's.
template <typename T>
__device__ __forceinline__ LvAxis<T> lv_resident(const LvAxis<T> &a)
{
    return {resident_t(a.x_min), resident_t(a.inv_dx), resident_t(a.u_max)};
}

// The tables of a workgroup, back to back in dynamic LDS (entries of VolPair<T>).
extern __shared__ __attribute__((aligned(16))) unsigned char lv_table_lds[];

// Every thread of the workgroup copies its share of one table to entry `offset` of the LDS tables.  The caller copies
// all its tables, then takes one __syncthreads(); after it the tables are read-only.
template <typename T>
__device__ __forceinline__ void lv_copy_table(VolPair<T> *tab, uint32_t offset, const VolPair<T> *table,
                                              uint32_t n_entries)
{
    for (uint32_t e = threadIdx.x; e < n_entries; e += kBlock) tab[offset + e] = table[e];
}

// Where a path stands in its surface, wave-uniform: base = (the table's offset in LDS) + row(i) n_x,
// phase = (i row_rem) mod n_steps.
struct LvRow {
    uint32_t base, phase;
};

// The volatility of step i at X, and the row of step i + 1.
template <typename T>
__device__ __forceinline__ T lv_sigma(T X, const LvAxis<T> &ax, const LvRows &r, const VolPair<T> *tab, LvRow &row)
{
    T u = (X - ax.x_min) * ax.inv_dx;
    u = lv_min(lv_max(u, T(0)), ax.u_max);   // a NaN lands on node 0: the index stays inside the table
    uint32_t k = static_cast<uint32_t>(u);
    k = k < r.k_max ? k : r.k_max;
    const T f = u - static_cast<T>(k);
    const VolPair<T> p = tab[row.base + k];
    const T s = fma_t(f, p.slope, p.sigma);
    // row(i + 1)
    row.base += r.row_whole_nx;
    if (row.phase >= r.row_thr) {
        row.phase -= r.row_thr;
        row.base += r.n_x;
    } else {
        row.phase += r.row_rem;
    }
    return s;
}

// lv_sigma for a kernel that differentiates the walk (localvol_greeks.hip): the same u, k, f and s at the row a caller
// holds, with the cell's slope and whether X lies strictly inside the axis (before the clamp: outside it the surface
// is flat and the walk has no slope; a NaN is outside).  The row is not advanced, so several walks can look the same
// step up; lv_next_row then carries it exactly as lv_sigma does.
template <typename T>
struct LvLookup {
    T s;           // fma(f, slope_k, sigma_k)
    T slope;       // slope_k
    bool inside;   // 0 < (X - x_min) (1 / dx) < n_x - 1
};

template <typename T>
__device__ __forceinline__ LvLookup<T> lv_sigma_slope(T X, const LvAxis<T> &ax, const LvRows &r, const VolPair<T> *tab,
                                                      const LvRow &row)
{
    const T u_raw = (X - ax.x_min) * ax.inv_dx;
    const T u = lv_min(lv_max(u_raw, T(0)), ax.u_max);
    uint32_t k = static_cast<uint32_t>(u);
    k = k < r.k_max ? k : r.k_max;
    const T f = u - static_cast<T>(k);
    const VolPair<T> p = tab[row.base + k];
    return {fma_t(f, p.slope, p.sigma), p.slope, u_raw > T(0) && u_raw < ax.u_max};
}

__device__ __forceinline__ void lv_next_row(const LvRows &r, LvRow &row)
{
    row.base += r.row_whole_nx;
    if (row.phase >= r.row_thr) {
        row.phase -= r.row_thr;
        row.base += r.n_x;
    } else {
        row.phase += r.row_rem;
    }
}

// The log-Euler move of one step at volatility s with the normal z (the correlated w_j of a multi-asset kernel).
// Returns s^2, which the bridge factor of a continuously monitored barrier divides by.
template <typename T>
__device__ __forceinline__ T lv_move(T &X, T s, T z, T sqrt_dt, T half_dt, T mu_dt)
{
    const T s2 = s * s;
    X += fma_t(s * sqrt_dt, z, fma_t(-s2, half_dt, mu_dt));
    return s2;
}

}  // namespace mcamd
