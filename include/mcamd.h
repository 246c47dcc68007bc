/*
 * mcamd.h — C ABI of the MI355X (gfx950) Monte Carlo option-pricing engine.
 *
 * This is the drop-in boundary for the hot path of amauryrlm/Monte-Carlo-Project-CUDA.
 * The reference has no FFI: its "API" is the header-level C++ surface of inc/wrappers.cuh,
 * inc/tool.cuh, inc/testing.cuh and inc/BlackandScholes.hpp called from hello.cu / testing.cu.
 * Each entry point below names the reference interface (file:line under the reference root)
 * it replaces; include/wrappers.hpp and friends re-expose the reference's own names on top of
 * this ABI.  Plain C types only: pointers, sizes, POD structs, int status codes.
 *
 * Conventions
 *  - every function returns MCAMD_OK (0) or an MCAMD_ERR_* code and never calls exit()
 *    (the reference's testCUDA / CHECK_MALLOC exit the process: inc/tool.cuh:47-53,92-100);
 *    mcamd_last_error() returns the calling thread's last message;
 *  - "d_" pointers are device (HBM) pointers on the context's device, owned by the caller;
 *  - calls are synchronous on the context's stream (as the reference's wrappers are:
 *    cudaDeviceSynchronize at inc/wrappers.cuh:48,79,115,157,233,297) unless named *_enqueue; a
 *    context is not thread-safe, distinct contexts are independent;
 *  - option parameters travel in the structs passed to each call; there is no global
 *    __constant__ symbol to upload first (reference: hello.cu:22, inc/trajectories.cuh:12);
 *  - random numbers: counter-based Philox4x32-10 held in registers, key = seed,
 *    subsequence = GLOBAL path id, i.e. exactly rocrand_init(seed, path_id, 0) followed by
 *    rocrand_normal4 (fp32, 4 steps per block) / rocrand_normal_double2 (fp64, 2 steps per
 *    block).  There is no RNG state array and no setup kernel (replaces setup_kernel,
 *    inc/tool.cuh:192-195, and init_rng_kernel, inc/testing.cuh:95-98).  Results therefore
 *    do not depend on how paths are sharded over GPUs, blocks or threads;
 *  - payoff sums are accumulated in fp64 whatever the path precision;
 *  - the in-register kernels carry ln(St/S0) through the step loop and exponentiate where the price is
 *    needed; MCAMD_FLAG_PRODUCT_FORM asks for the reference's recurrence St *= exp(...) as written
 *    (same draws, same scheme, ~1e-14 relative apart in fp64).
 */
#ifndef MCAMD_H
#define MCAMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCAMD_ABI_VERSION 5

/* status codes */
#define MCAMD_OK 0
#define MCAMD_ERR_INVALID 1   /* bad argument (null pointer, zero steps, shape mismatch ...) */
#define MCAMD_ERR_HIP 2       /* a HIP runtime call or kernel launch failed */
#define MCAMD_ERR_NODEVICE 3  /* no usable gfx950 device */
#define MCAMD_ERR_NOMEM 4     /* device or host allocation failed */

/* arithmetic type of the simulated paths */
#define MCAMD_F32 32
#define MCAMD_F64 64

/* trajectory / point-array layouts */
#define MCAMD_STEP_MAJOR 0 /* a[step * n_paths_local + path]  — coalesced, the engine's native layout */
#define MCAMD_PATH_MAJOR 1 /* a[path * n_steps + step]        — the reference's layout
                              (inc/trajectories.cuh:304-305, inc/testing.cuh:69) */

/* nested-MC strategies; all give the same per-point prices up to fp64 summation order (the third reference strategy,
 * the fused single launch, is mcamd_nmc_fused and equals WAVE_PER_POINT bit for bit) */
#define MCAMD_NMC_WAVE_PER_POINT 0  /* replaces compute_nmc_optimal, inc/nmc.cuh:280-386.  The fast one: with a window,
                                       wavefronts refill lanes whose path is over instead of waiting for the last */
#define MCAMD_NMC_BLOCK_PER_POINT 1 /* replaces compute_nmc_one_block_per_point, inc/nmc.cuh:12-108: one workgroup per point;
                                       with a window each of its wavefronts compacts its share of the point's paths */
#define MCAMD_NMC_BLOCK_PER_POINT_PLAIN 2 /* the same without lane compaction (path j on thread j mod 256, a wavefront waits
                                       for its last lane): the independent implementation the compacting kernels are
                                       fuzzed against (tools/fuzz_nmc.py); 2-3x slower with the reference's window */

/* mcamd_sim.flags */
#define MCAMD_FLAG_LOG_SPACE 1 /* accepted for compatibility and redundant: it names what the in-register kernels do by
                                  default (ABI <= 4 had it as an opt-in).  They carry ln(St/S0) through the step loop
                                  instead of St — one add (window-less) or one fma and a compare (barrier window) per step
                                  instead of an exponential and a multiply; every step still draws its normal, and the price
                                  is exponentiated where it is needed.  The same scheme (the exact GBM step,
                                  inc/trajectories.cuh:146) with the product of the step factors re-associated into the
                                  exponential of their sum; rounding differs at ~1e-14 relative in fp64 (measured: 17 % /
                                  21 % less time for window-less pricing in fp64 / fp32 with the pair sums of
                                  csrc/mc_device.hpp, 12 % for the nested-MC inner stage; same oracle tolerances). */
#define MCAMD_FLAG_PRODUCT_FORM 16 /* mcamd_price_paths, mcamd_nmc_inner, mcamd_nmc_fused: carry the price itself,
                                  St *= exp(...) every step — the reference's recurrence as written — and test the barrier
                                  on it.  Keeps the in-register terminal price the same BITS as the last row
                                  mcamd_simulate_trajectories stores for the same path, and the barrier counts the same
                                  integers as the stored ones.  (The store and array-driven kernels always run this form:
                                  they need St at every step.)  Not combinable with MCAMD_FLAG_LOG_SPACE. */

#define MCAMD_FLAG_ANTITHETIC 2 /* opt-in (mcamd_price_paths): a sample is the antithetic pair (G, -G) of one path's
                                  normals; its payoff is the pair's mean; n counts pairs.  New capability. */
#define MCAMD_FLAG_CONTROL_VARIATE 4 /* opt-in (mcamd_price_paths): S_T as control variate (E[S_T] = S e^{rT} is
                                  known); the call also returns the three cross sums and the finalized price uses the
                                  sample-optimal beta (mcamd_finalize_cv).  New capability. */

#define MCAMD_FLAG_SEPARATE_REDUCE 8 /* diagnostic (mcamd_price_paths[_enqueue]): sum the block records with a separate
                                  one-workgroup launch even where the simulation kernel would finish the sum itself (jobs
                                  of up to 8192 workgroups: its last workgroup to arrive does it).  Same summation order,
                                  same bits; exists so that a test can show exactly that. */

/* reduce variants: names follow the reference's ReductionType (inc/testing.cuh:100-106) */
#define MCAMD_REDUCE_SEQUENTIAL 3
#define MCAMD_REDUCE_FIRST_ADD 4
#define MCAMD_REDUCE_UNROLL_LAST 5
#define MCAMD_REDUCE_GRID_STRIDE 6

typedef struct mcamd_ctx mcamd_ctx;

/* Option parameters: the reference's OptionData (inc/tool.cuh:13-26) in double precision,
 * plus the restart triple the bullet kernels accept (inc/trajectories.cuh:116-117,140-143). */
typedef struct mcamd_option {
    double S0;          /* spot */
    double T;           /* maturity */
    double K;           /* strike */
    double r;           /* risk-free rate */
    double v;           /* volatility */
    double B;           /* barrier level (bullet option) */
    int32_t P1, P2;     /* payoff only if P1 <= #steps{B > St} <= P2 */
    int32_t use_window; /* 0: European call (no barrier test at all); 1: bullet window */
    int32_t Ik;         /* restart: initial barrier count */
    double Sk;          /* restart: initial price; 0 means S0 (inc/trajectories.cuh:141) */
    int32_t Tk;         /* restart: steps already elapsed; n_steps - Tk are simulated */
    int32_t reserved;
    double dt;          /* time step of the multi-step kernels, the reference's OptionData.step
                           (inc/tool.cuh:25, read at inc/trajectories.cuh:131, inc/nmc.cuh:28); 0 = T / n_steps.
                           The discount stays exp(-r T), as in the reference (inc/wrappers.cuh:85). */
} mcamd_option;

/* Simulation shape. The job has n_paths paths; this call simulates the shard
 * [path_offset, path_offset + n_paths_local) of it.  A single-GPU caller passes
 * path_offset = 0, n_paths_local = n_paths.  n_paths_local == 0 is a legal empty shard
 * (all-zero statistics, nothing launched). */
typedef struct mcamd_sim {
    uint64_t n_paths;
    uint64_t path_offset;
    uint64_t n_paths_local;
    uint32_t n_steps;       /* N_STEPS; dt = T / n_steps; 1 = the exact one-step pricer */
    uint32_t n_paths_inner; /* N_PATHS_INNER (nested MC only) */
    uint64_t seed;          /* the reference hard-codes 1234 / 1235 (inc/wrappers.cuh:41,163) */
    int32_t precision;      /* MCAMD_F32 or MCAMD_F64 */
    int32_t flags;          /* OR of MCAMD_FLAG_* (0 = the reference's plain estimator) */
} mcamd_sim;

/* Result of a pricing call. sum/sumsq/n are the shard's raw fp64 statistics (what a multi-GPU
 * caller all-reduces); price..ci_hi are finalized from them as if the shard were the whole job
 * (see mcamd_finalize). */
typedef struct mcamd_result {
    double sum;        /* sum of undiscounted payoffs */
    double sumsq;      /* sum of squared undiscounted payoffs */
    uint64_t n;        /* paths in the shard */
    double price;      /* exp(-rT) * sum / n              (inc/wrappers.cuh:51,85,118) */
    double std_err;    /* exp(-rT) * sqrt(s^2 / n)        (new: the reference has no variance) */
    double ci_lo;      /* price -/+ 1.96 std_err */
    double ci_hi;
    float kernel_ms;   /* HIP-event time of the simulation kernel alone, on the context's stream */
    float total_ms;    /* HIP-event time of the whole call's device work (kernel + final reduce + D2H; equal to kernel_ms
                          when the kernel finishes its own sum: MCAMD_FLAG_SEPARATE_REDUCE) */
    uint32_t grid;     /* launch shape the engine chose (threadsPerBlock / number_of_blocks of the */
    uint32_t block;    /* reference wrappers are accepted by the shim and ignored) */
    /* control variate (MCAMD_FLAG_CONTROL_VARIATE), zero otherwise: c = S_T - E[S_T] per sample */
    double sum_c;      /* sum of c */
    double sum_cc;     /* sum of c^2 */
    double sum_yc;     /* sum of payoff * c */
    double cv_beta;    /* sample-optimal coefficient cov(y, c) / var(c) used in price */
    double cv_rho;     /* sample correlation of payoff and control; variance shrinks by 1 - rho^2 */
    /* nested MC (mcamd_nmc_inner / mcamd_nmc_fused), zero otherwise: inner path-steps the kernel executed, counted as
     * 64 lanes x the steps each wavefront ran (a wavefront leaves a point's step loop as soon as every lane's barrier
     * count is beyond P2, where the payoff can no longer be non-zero): the work figure for throughput / roofline */
    double work_steps;
    /* of those, the lane-steps taken by paths whose window was still open (live_steps / work_steps = how full the
     * wavefronts ran; equal to work_steps without a window) */
    double live_steps;
} mcamd_result;

/* Device report: replaces getDeviceProperty (inc/tool.cuh:56-88) and the free/total memory
 * print of get_max_blocks (inc/tool.cuh:176-188). */
typedef struct mcamd_device_info {
    char name[256];
    char arch[64];
    uint64_t total_mem, free_mem;
    int32_t compute_units, wavefront_size, max_threads_per_block, clock_khz, mem_clock_khz, mem_bus_bits;
    int32_t lds_per_block, regs_per_block, l2_bytes, device_index, device_count, reserved;
} mcamd_device_info;

int mcamd_abi_version(void);
const char *mcamd_last_error(void);
/* 16-hex-digit hash of the kernel sources and compile flags this library was built from; profiles/valu_slots.json
 * (the ISA issue-slot counts bench.py prices the VALU roofline with) carries the same id when it describes this build */
const char *mcamd_build_id(void);
int mcamd_device_count(int *count);

/* hip_stream: a hipStream_t to launch on (e.g. the caller framework's current stream), or NULL
 * to let the context create its own non-blocking stream.  Note that the legacy default stream's handle IS
 * NULL (torch.cuda.current_stream().cuda_stream == 0 unless a stream was made current): to share the default
 * stream pass hipStreamLegacy, or — as bench.py does — make an explicit stream current and pass that.
 * Scratch buffers are owned by the context and reused. */
int mcamd_ctx_create(int device, void *hip_stream, mcamd_ctx **ctx);
int mcamd_ctx_destroy(mcamd_ctx *ctx);
int mcamd_get_device_info(mcamd_ctx *ctx, mcamd_device_info *info);

/* Device memory helpers so that a host program needs nothing but this library (the reference's
 * wrappers call cudaMalloc / cudaMemcpy / cudaFree directly: inc/wrappers.cuh:39,49,55).
 * Copies are synchronous with respect to the context's stream. */
int mcamd_device_malloc(mcamd_ctx *ctx, uint64_t bytes, void **d_ptr);
int mcamd_device_free(mcamd_ctx *ctx, void *d_ptr);
int mcamd_memcpy_to_host(mcamd_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes);
int mcamd_memcpy_to_device(mcamd_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes);

/* In-register Monte Carlo: RNG -> GBM steps -> payoff -> fp64 (sum, sumsq); nothing is stored.
 * Replaces the kernel + host tail of
 *   wrapper_gpu_option_vanilla          inc/wrappers.cuh:33-57   (n_steps = 1)
 *     simulateOptionPriceMultipleBlockGPUwithReduce  inc/trajectories.cuh:54-113
 *   wrapper_gpu_bullet_option[_atomic]  inc/wrappers.cuh:59-125  (use_window = 1)
 *     simulateBulletOptionPriceMultipleBlockGPU[atomic]  inc/trajectories.cuh:115-271
 * and is the multi-step European pricer of BASELINE configs 2 and 5 (use_window = 0).
 * The library picks the kernel: window jobs of millions of paths (plain estimator) run the lane-compacting kernel, other
 * window jobs one path per thread, window-less jobs the pair-sum loop (two paths per thread: ln(S_T/S_0) from the sum of
 * the path's normals, a Box-Muller pair contributing sqrt2 r sin(a + pi/4)); a path's payoff does not depend on which
 * (same Philox stream, same arithmetic), so any sharding of a job gives the same sums up to fp64 summation order.
 * Jobs of up to 8192 workgroups are ONE launch: the kernel's last workgroup sums the block records in a fixed order
 * (see MCAMD_FLAG_SEPARATE_REDUCE). */
int mcamd_price_paths(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, mcamd_result *res);

/* Asynchronous form of mcamd_price_paths: enqueues the simulation kernel (and, for large grids, the final reduction) on
 * the context's stream and returns without waiting.  d_stats (device, >= 6 doubles) receives {sum, sumsq, sum_c, sum_cc, sum_yc, n}
 * (the cross sums are zero without MCAMD_FLAG_CONTROL_VARIATE).  The caller orders later work on the same stream —
 * typically ONE all-reduce of d_stats over the ranks — and finalizes after synchronising (mcamd_finalize_stats), so
 * a multi-step driver pays no host round trip per step.  New (the reference is fully synchronous).
 *   Overlap: a job whose block records need the separate final reduction (more than 8192 workgroups; fp64 without a
 * window: 4.2M paths and up) runs its simulation kernel on one of two non-blocking streams the context owns, into a
 * scratch buffer of that stream, and only the reduction into d_stats on the context's stream, behind the kernel.
 * Consecutive such jobs take the two streams in turn, so the next job's kernel fills the chip while this one's last
 * workgroups drain.  What holds as before: d_stats is written on the context's stream, after everything enqueued there
 * before the call and before everything enqueued after it, and any later call on the context starts after the
 * simulation kernels of all earlier ones.  What is new: such a job's simulation kernel may START before earlier work
 * on the context's stream has finished; it reads no memory of the caller's.  A stream that is being captured into a
 * graph, a failure to create the internal streams, and MCAMD_ENQUEUE_OVERLAP=0 in the environment when the context
 * is created keep every job in order on the context's stream. */
int mcamd_price_paths_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, double *d_stats);
/* HIP-event times (ms) of the simulation kernels of the last n_last (<= 64) enqueued calls, oldest first.
 * Synchronises the stream (and the context's internal streams).  An overlapped job (mcamd_price_paths_enqueue) that
 * follows another is charged the part of its kernel's interval after the earlier job's kernel ended,
 * end_N - max(start_N, end_{N-1}), never less than 0, where "earlier" is taken in the order in which the kernels of the
 * run ended (two kernels that share the device may end in either order): the times of a run of overlapped jobs are
 * disjoint parts of the time the device was busy with them.  Every other call's time is its kernel's own
 * start-to-end interval. */
int mcamd_enqueued_kernel_ms(mcamd_ctx *ctx, uint32_t n_last, float *ms);
/* Host: finalize a (possibly all-reduced) 6-double stats record copied back from the device. */
int mcamd_finalize_stats(const double stats[6], double r, double T, int control_variate, mcamd_result *res);

/* Trajectory store: as above, and every St (and, if d_counts != NULL, every running barrier
 * count) is written to HBM.  d_traj: n_sim_steps * n_paths_local elements of the path precision
 * (n_sim_steps = n_steps - Tk); d_counts: same shape, int32, or NULL; d_payoffs: n_paths_local
 * undiscounted payoffs of the path precision, or NULL.
 * Replaces simulateOptionPriceMultipleBlockGPU (trajectory overload) inc/testing.cuh:46-73 and
 * simulate_outer_trajectories inc/trajectories.cuh:273-351. */
int mcamd_simulate_trajectories(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int layout,
                                void *d_traj, int32_t *d_counts, void *d_payoffs, mcamd_result *res);

/* Diagnostic: mcamd_simulate_trajectories' launch shape and store stream (step-major rows, one 16-byte non-temporal
 * store per lane per step, then the payoff row if d_payoffs != NULL) with nothing simulated: the HBM write ceiling of
 * this access pattern on this device, measured beside the real kernel (bench.py roofline_store.same_run_ceiling).
 * Requirements of the vector store path: n_paths_local a multiple of 4 (fp32) / 2 (fp64), 16-byte aligned buffers.
 * kernel_ms: HIP-event time of the kernel.  The buffers are overwritten with a counter pattern. */
int mcamd_diag_store_pattern(mcamd_ctx *ctx, uint64_t n_paths_local, uint32_t n_steps, int precision, void *d_traj,
                             void *d_payoffs, float *kernel_ms);

/* Array-driven pricer: normals are an input, d_normals[path * n_sim_steps + step] (the reference's
 * layout; a row holds the n_sim_steps = n_steps - Tk simulated steps, so the buffer has
 * n_paths_local * n_sim_steps elements), precision per sim->precision; d_payoffs (nullable):
 * n_paths_local payoffs.
 * Replaces simulateOptionPriceGPU / simulateOptionPriceMultipleBlockGPU (array overloads)
 * inc/trajectories.cuh:14-52; CPU twin inc/testing.cuh:75-91. */
int mcamd_price_from_normals(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const void *d_normals,
                             void *d_payoffs, mcamd_result *res);

/* Bulk N(0,1) fill of d_out[0..n): one Philox sequence (subsequence 0) consumed front to back,
 * 4 floats / 2 doubles per block.  Replaces generate_random_array's curandGenerateNormal,
 * inc/testing.cuh:17-24. */
int mcamd_generate_normals(mcamd_ctx *ctx, uint64_t seed, uint64_t n, int precision, void *d_out, float *kernel_ms);

/* Sum of d_in[0..n) (fp32 or fp64 elements) accumulated in fp64.  variant selects the schedule
 * named after the reference's reduce3..reduce6 (inc/reduce.cuh:9-227); *sum is the complete sum
 * for every variant (the reference leaves a per-block array for the caller to finish,
 * inc/testing.cuh:227-234). */
int mcamd_reduce_sum(mcamd_ctx *ctx, const void *d_in, uint64_t n, int precision, int variant, double *sum,
                     float *kernel_ms);

/* As mcamd_reduce_sum, but with the reference's launch shape and result shape: the schedule runs on n_blocks workgroups
 * and h_partials (HOST, n_blocks doubles) receives one partial sum per workgroup, as reduce3..6 leave one float per
 * block in g_odata for the caller to finish (inc/reduce.cuh:9-227; Simulation::test_reduction copies them back,
 * inc/testing.cuh:185-235).  Unlike reduce3..5 — whose blocks cover 2 * blockDim elements each and nothing beyond
 * n_blocks of those — every element is covered for any n_blocks (blocks stride over the array), so the partials
 * always add up to the complete sum.  1 <= n_blocks <= 2^20. */
int mcamd_reduce_partials(mcamd_ctx *ctx, const void *d_in, uint64_t n, int precision, int variant, uint32_t n_blocks,
                          double *h_partials, float *kernel_ms);

/* Nested Monte Carlo, inner stage: for every stored point (step, path) of the shard, n_paths_inner
 * continuation paths of n_steps - 1 - step steps from (d_prices, d_counts), windowed payoff, mean,
 * discount exp(-rT).  d_prices / d_counts are what mcamd_simulate_trajectories wrote (same layout
 * argument); d_point_prices receives one value of the path precision per point in that layout.
 * Inner stream: seed = sim->seed, subsequence = global_point_id * n_paths_inner + j with
 * global_point_id = global_path * n_steps + step (global_path = path_offset + local path): a shard of a job prices
 * its points from the same streams as the whole job.  WAVE_PER_POINT pools the continuation paths of 8 outer paths
 * whose GLOBAL ids share id / 8, so a point's price is bit-identical under any sharding wherever its pool lies
 * inside the shard, and differs by fp64 summation order only in a shard's partial first / last pool;
 * BLOCK_PER_POINT and the window-less job are bit-identical under any sharding.
 * Replaces compute_nmc_one_block_per_point / compute_nmc_optimal, inc/nmc.cuh:12-108,280-386.
 * res->sum / n: sum and count of the per-point prices (the wrappers' scalar diagnostic,
 * inc/wrappers.cuh:185-189,316-321). */
int mcamd_nmc_inner(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int layout, int variant,
                    const void *d_prices, const int32_t *d_counts, void *d_point_prices, mcamd_result *res);

/* Nested Monte Carlo, outer + inner stage fused in ONE launch: the wavefronts of a persistent grid first simulate and
 * store the outer paths, 64 at a time from a device-scope queue (seed = outer_seed), publish them (release / acquire
 * across the device's L2s), then price the points exactly as mcamd_nmc_inner(MCAMD_NMC_WAVE_PER_POINT) does (inner
 * seed = sim->seed).  d_prices / d_counts / d_point_prices are OUTPUTS here (same shapes and layout rule as above; d_counts may be NULL for
 * use_window = 0).  Results are bit-identical to mcamd_simulate_trajectories + mcamd_nmc_inner with the same
 * two seeds.  Replaces compute_nmc_one_block_per_point_with_outter, inc/nmc.cuh:113-275
 * (wrapper_gpu_bullet_option_nmc_one_kernel, inc/wrappers.cuh:209-266). */
int mcamd_nmc_fused(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, uint64_t outer_seed, int layout,
                    void *d_prices, int32_t *d_counts, void *d_point_prices, mcamd_result *res);

/* Asynchronous forms of the trajectory store and the nested-MC calls, as mcamd_price_paths_enqueue: the simulation
 * kernel and the final reduction are enqueued on the context's stream, nothing waits on the host.  d_stats (device,
 * >= 6 doubles) receives
 *   store:      {sum, sumsq, 0, 0, 0, n}                              -> mcamd_finalize_stats
 *   nested MC:  {sum of point prices, sum of their squares, wave-steps executed, live lane-steps, 0, n points}
 *                                                                     -> mcamd_finalize_nmc_stats
 * so ONE all-reduce of 6 doubles carries a shard whichever call produced it.  The output arrays are complete when
 * the stream reaches the point after the call.  mcamd_enqueued_kernel_ms covers these calls too.  New (the
 * reference is fully synchronous). */
int mcamd_simulate_trajectories_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int layout,
                                        void *d_traj, int32_t *d_counts, void *d_payoffs, double *d_stats);
int mcamd_nmc_inner_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int layout, int variant,
                            const void *d_prices, const int32_t *d_counts, void *d_point_prices, double *d_stats);
int mcamd_nmc_fused_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, uint64_t outer_seed,
                            int layout, void *d_prices, int32_t *d_counts, void *d_point_prices, double *d_stats);
/* Host: sum / sumsq / n / price (= mean point price) / work_steps / live_steps of a (possibly all-reduced) nested-MC
 * statistics record copied back from the device. */
int mcamd_finalize_nmc_stats(const double stats[6], mcamd_result *res);

/* ---- single-process multi-GPU (the shape of the reference's own main(): one host process) ----
 * A group owns one context per device and an RCCL communicator clique over them (ncclCommInitAll; RCCL is loaded
 * with dlopen on first use).  mcamd_group_price_paths splits [path_offset, path_offset + n_paths_local) of the job
 * into contiguous per-device shards, runs them concurrently (mcamd_price_paths_enqueue on every device), sums the
 * 6-double statistics records with ONE ncclAllReduce over xGMI and finalizes.  Because a path's random numbers
 * depend only on its global id, the result equals the single-device result up to fp64 summation order.
 * devices == NULL: devices 0..n_devices-1; n_devices <= 0: all visible devices.  The reference has no multi-GPU
 * code.  One-process-per-GPU hosts use mcamd_price_paths_enqueue + their own collective (bench.py). */
typedef struct mcamd_group mcamd_group;
int mcamd_group_create(int n_devices, const int *devices, mcamd_group **group);
int mcamd_group_destroy(mcamd_group *group);
int mcamd_group_size(mcamd_group *group, int *n_devices);
int mcamd_group_price_paths(mcamd_group *group, const mcamd_option *opt, const mcamd_sim *sim, mcamd_result *res);

/* The other two shards of SURVEY 8e: "trajectory-store mode shards the [step][path] buffer by path columns per GPU; no
 * exchange" and "NMC shards by outer path; per-point prices stay on the owning GPU".  The reference's store and
 * nested-MC hosts are single-process C++ (inc/trajectories.cuh:273-351, inc/wrappers.cuh:128-340), which is the shape
 * these calls serve.  Device i of the group works on the shard mcamd_group_shard reports for it (contiguous global
 * path ids, sizes differing by at most one) and writes into the caller's buffers ON THAT DEVICE: d_traj[i], d_counts[i],
 * d_payoffs[i], d_prices[i], d_point_prices[i] are arrays of n_devices device pointers, each sized for its own shard
 * (shape rules of the single-device calls with n_paths_local = the shard's; a NULL array = the single-device call's
 * NULL; entries of empty shards are ignored).  mcamd_group_ctx hands out device i's context for mcamd_device_malloc /
 * mcamd_memcpy_*.  All devices run concurrently (the *_enqueue forms); the only exchange is ONE ncclAllReduce of the
 * 6-double statistics record; res is finalized from the reduced record (store: price / SE / CI of the whole job;
 * nested MC: sum / mean / count of all point prices, executed and live lane-steps), kernel_ms = the slowest device's
 * simulation kernel.  Results equal the single-device call's: stored columns and per-point prices as documented at
 * mcamd_nmc_inner (bit-identical outside a shard's partial edge pools), statistics up to fp64 summation order. */
int mcamd_group_ctx(mcamd_group *group, int i, mcamd_ctx **ctx);
int mcamd_group_shard(mcamd_group *group, const mcamd_sim *sim, int i, uint64_t *path_offset, uint64_t *n_paths_local);
int mcamd_group_simulate_trajectories(mcamd_group *group, const mcamd_option *opt, const mcamd_sim *sim, int layout,
                                      void *const *d_traj, int32_t *const *d_counts, void *const *d_payoffs,
                                      mcamd_result *res);
int mcamd_group_nmc_inner(mcamd_group *group, const mcamd_option *opt, const mcamd_sim *sim, int layout, int variant,
                          const void *const *d_prices, const int32_t *const *d_counts, void *const *d_point_prices,
                          mcamd_result *res);
int mcamd_group_nmc_fused(mcamd_group *group, const mcamd_option *opt, const mcamd_sim *sim, uint64_t outer_seed,
                          int layout, void *const *d_prices, int32_t *const *d_counts, void *const *d_point_prices,
                          mcamd_result *res);

/* ---- Greeks: in-kernel sensitivities of the call price ----
 * One call simulates the job's paths once and returns the price and five sensitivities with their standard errors:
 * every path contributes one undiscounted sample of each (formed once per path, in fp64 from the path-precision state),
 * the kernel sums them and their squares in fp64, and value = D * mean, std_err = D * sqrt(s^2 / n) with
 * D = exp(-r T) (the full T, as everywhere in the engine).  The paths are mcamd_price_paths' (same Philox stream =
 * global path id, same arithmetic), so the price sample is the same payoff and any sharding gives the same sums up to
 * fp64 summation order; a finite difference of mcamd_price_paths calls with the same seed (common random numbers)
 * is an independent check.  New (the reference has no sensitivities).
 * Notation: S_s = Sk if Sk > 0 else S0 (start of the simulated segment), T_h = (n_steps - Tk) dt the simulated
 * horizon, L = ln(S_T / S_s), z_i the path's normals.  Sensitivities are with respect to S_s, v, r and — theta —
 * the maturity (theta = -dV/dT).
 *   MCAMD_GREEKS_PATHWISE (European, use_window = 0, only): the pair-sum loop of mcamd_price_paths plus an epilogue.
 *     delta 1{S_T>K} S_T / S_s;  gamma (mixed pathwise-LR) 1{S_T>K} K (L - (r - v^2/2) T_h) / (S_s^2 v^2 T_h);
 *     vega 1{S_T>K} S_T (L - (r + v^2/2) T_h) / v;  rho -T (S_T-K)+ + 1{S_T>K} S_T T_h;
 *     theta r (S_T-K)+ - 1{S_T>K} S_T ((r - v^2/2) + (L - (r - v^2/2) T) / (2T)), defined only when Tk == 0 and
 *     opt->dt == 0 (the simulated horizon is the maturity); NaN otherwise.
 *   MCAMD_GREEKS_LIKELIHOOD_RATIO (any payoff; y the payoff, the bullet window included — its payoff is discontinuous
 *     in the barrier count, which makes pathwise estimators wrong there):
 *     delta y z_1 / (S_s v sqrt(dt));  gamma y ((z_1^2 - 1) / (S_s^2 v^2 dt) - z_1 / (S_s^2 v sqrt(dt)));
 *     vega y sum_i ((z_i^2 - 1) / v - z_i sqrt(dt));  rho y (sum_i z_i sqrt(dt) / v - T);  theta NaN.
 *     The LR variance grows as the step shrinks (gamma like 1 / dt): prefer pathwise wherever it applies.  A bullet
 *     job runs one path per thread without lane compaction (its wavefronts still stop once every window is closed).
 *   MCAMD_GREEKS_AUTO: pathwise without a window, likelihood ratio with one.
 * Requirements: v > 0; sim->flags 0 or MCAMD_FLAG_LOG_SPACE (MCAMD_FLAG_ANTITHETIC, _CONTROL_VARIATE, _PRODUCT_FORM
 * and _SEPARATE_REDUCE are MCAMD_ERR_INVALID for now); MCAMD_GREEKS_PATHWISE with use_window = 1 is MCAMD_ERR_INVALID.
 * Other argument checks are mcamd_price_paths'.  An empty shard returns an all-zero record. */
#define MCAMD_GREEKS_AUTO 0
#define MCAMD_GREEKS_PATHWISE 1
#define MCAMD_GREEKS_LIKELIHOOD_RATIO 2

#define MCAMD_GREEK_PRICE 0
#define MCAMD_GREEK_DELTA 1
#define MCAMD_GREEK_GAMMA 2
#define MCAMD_GREEK_VEGA 3
#define MCAMD_GREEK_RHO 4
#define MCAMD_GREEK_THETA 5

typedef struct mcamd_greeks {
    double value[6];    /* D * mean, indexed MCAMD_GREEK_*; theta NaN where it is not defined */
    double std_err[6];  /* D * sqrt(s^2 / n) */
    double sum[6];      /* the shard's raw fp64 sums of the undiscounted samples (what a multi-GPU caller all-reduces) */
    double sumsq[6];    /* and of their squares */
    uint64_t n;         /* paths */
    int32_t method;     /* MCAMD_GREEKS_PATHWISE or MCAMD_GREEKS_LIKELIHOOD_RATIO: the estimator actually used */
    float kernel_ms;    /* HIP-event time of the kernel (it finishes its own sum: the whole call's device work) */
    float total_ms;
    uint32_t grid;      /* launch shape the engine chose */
    uint32_t block;
    int32_t reserved;
} mcamd_greeks;

int mcamd_price_greeks(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int method, mcamd_greeks *out);
/* Asynchronous form: d_stats (device, >= 16 doubles) receives [0..12) the (sum, sumsq) pairs of price, delta, gamma,
 * vega, rho, theta in that order, [12] = n, [13..16) = 0 — one all-reduce of 16 doubles carries a shard.  Until the
 * kernel has written it, the record reads NaN.  mcamd_enqueued_kernel_ms covers this call. */
int mcamd_price_greeks_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, int method,
                               double *d_stats);
/* Host: value / std_err / sums / n of a (possibly all-reduced) 16-double Greeks record; theta_defined = 0 reports
 * theta as NaN.  method, timings and launch shape are left 0. */
int mcamd_finalize_greeks_stats(const double stats[16], double r, double T, int theta_defined, mcamd_greeks *out);
/* The group form: shards as mcamd_group_price_paths, ONE all-reduce of the 16-double record. */
int mcamd_group_price_greeks(mcamd_group *group, const mcamd_option *opt, const mcamd_sim *sim, int method,
                             mcamd_greeks *out);
/* Host closed form (Black-Scholes call, exact erfc form): out = {price, N(d1), phi(d1) / (S v sqrt(T)),
 * S phi(d1) sqrt(T), K T e^{-rT} N(d2), -S phi(d1) v / (2 sqrt(T)) - r K e^{-rT} N(d2)} in MCAMD_GREEK_* order. */
int mcamd_bs_greeks_f64(double S0, double K, double T, double r, double v, double out[6]);

/* ---- American / Bermudan options: least-squares Monte Carlo (Longstaff and Schwartz, 2001) ----
 * A put or call on GBM that may be exercised every k-th step.  dt = T / n_steps; exercise dates j = 1..M at steps
 * s_j = j k (M = n_steps / k; date M is maturity), t_j = s_j dt, d_j = exp(-r t_j); S_{p,j} is path p after step s_j
 * (the product-form path of mcamd_simulate_trajectories, in the path precision; regression arithmetic is fp64 on
 * (double) S); h(S) = max(K - S, 0) for a put, max(S - K, 0) for a call; basis phi(S) = (1, u, .., u^(m-1)) with
 * u = S / K - 1, m = n_basis.
 *  1. Training (the backward sweep) on n_train paths of train_seed, global ids 0..n_train-1, stored whole on this
 *     context's device: V_p = d_M h(S_{p,M}); for j = M-1 .. 1, over I_j = {p : h(S_{p,j}) > 0}, solve
 *     (sum phi phi^T) beta_j = sum V_p phi by Cholesky of the Jacobi-scaled matrix; date j is not regressed (no
 *     exercise there) when |I_j| < 4 m or a scaled pivot is <= 1e-10; otherwise V_p = d_j h(S_{p,j}) for the p of
 *     I_j with d_j h(S_{p,j}) > phi(S_{p,j}) . beta_j.  The mean of V is the in-sample estimate (biased high).
 *  2. Pricing on the job's shard (sim->seed, global ids path_offset + i): a path's sample is d_j h(S) at the first
 *     regressed date j < M where h > 0 and d_j h(S) > phi(S) . beta_j, else d_M h(S_M).  The mean is the
 *     out-of-sample estimate (biased low: the rule is fitted on other paths); its SE is an honest one.
 *     mcamd_american_upper_bound turns the same rule into an estimate biased HIGH, whatever its inner sample size.
 * Both passes decide through one device function, so with train_seed == sim->seed and n_train == n_paths they
 * see the same paths and make the same decisions.  Samples are discounted where they are paid: the estimates are
 * plain means (no exp(-rT) factor).  Exercise at t = 0: where h(S0) exceeds an estimate, h(S0) is reported in its
 * place with std_err 0, and immediate_exercise is set.  Multi-GPU: every rank trains identically with the same
 * train_seed and prices its own shard; the raw sums (sum, sumsq, n, n_early, sum_t_exercise) add over shards.
 * Requirements (MCAMD_ERR_INVALID before any device work): payoff 0/1, n_basis in {0, 2, 3, 4}, k >= 1 with
 * n_steps % k == 0, reserved == 0, n_train >= 1, M <= 4096, use_window == 0, Tk == 0, Sk == 0, opt->dt == 0, v > 0,
 * sim->flags 0, MCAMD_FLAG_LOG_SPACE or MCAMD_FLAG_PRODUCT_FORM (the product form runs either way), d_work and
 * res non-NULL, work_bytes >= mcamd_american_workspace_bytes.  An empty pricing shard still trains and returns
 * n = 0.  New (the reference prices European-style claims only). */
#define MCAMD_PAYOFF_CALL 0
#define MCAMD_PAYOFF_PUT 1

typedef struct mcamd_american {
    int32_t payoff;            /* MCAMD_PAYOFF_* */
    uint32_t exercise_every;   /* k >= 1, n_steps % k == 0; k == n_steps: European exercise */
    uint32_t n_basis;          /* 2..4; 0 = 3 */
    uint32_t reserved;         /* must be 0 */
    uint64_t n_train;          /* training paths, simulated whole on this context's device */
    uint64_t train_seed;       /* may equal sim->seed (then the two passes see the same paths) */
} mcamd_american;

typedef struct mcamd_american_result {
    double price;              /* out-of-sample estimate sum / n (h(S0) where that is larger) */
    double std_err;            /* sqrt(s^2 / n) (0 where h(S0) was taken) */
    double ci_lo, ci_hi;       /* price -/+ 1.96 std_err */
    double sum, sumsq;         /* the shard's raw fp64 sums of the discounted samples */
    uint64_t n;                /* paths priced (the shard) */
    double in_sample_price;    /* mean of V over the training paths (h(S0) where that is larger) */
    double in_sample_std_err;
    double in_sample_sum, in_sample_sumsq;  /* sum of V and of V^2 */
    uint64_t n_train;
    uint64_t n_early;          /* paths of the shard exercised before maturity */
    double sum_t_exercise;     /* sum of their exercise times t_j */
    uint32_t n_dates;          /* M */
    uint32_t n_regressed;      /* dates 1..M-1 with a fitted exercise rule */
    int32_t immediate_exercise;/* 1: h(S0) exceeded an estimate and replaced it */
    float train_ms;            /* HIP-event times: trajectory store + backward sweep */
    float price_ms;            /* pricing kernel */
    float total_ms;            /* the whole call's device work */
    uint32_t grid;             /* pricing kernel's launch shape */
    uint32_t block;
    uint32_t train_grid;       /* backward sweep's workgroups per launch */
    int32_t reserved;
} mcamd_american_result;

/* Bytes of the caller-owned device workspace of mcamd_price_american: with A(x) = x rounded up to 256,
 *   256 + A(n_steps n_train sizeof(path precision))   stored training trajectories (step-major)
 *       + A(8 n_train)                                  V
 *       + A(8 (8 (M + 1) + 32))                          coefficient table (8 doubles per date) + two records
 *       + A(8 max(2 G_store, 12 G_sweep))                block records
 * G_store = min(max(ceil(ceil(n_train / V) / 256), 1), 2^20) with V = 4 (fp32) / 2 (fp64), G_sweep = min(ceil(n_train /
 * 256), 8192).  Any alignment of d_work is accepted (the leading 256 bytes absorb it). */
int mcamd_american_workspace_bytes(const mcamd_american *am, const mcamd_sim *sim, uint64_t *bytes);
/* h_coeffs (nullable, host): M rows of n_basis + 1 doubles, row j-1 = beta_j then 1 (regressed) or 0; rows of dates
 * without a rule (and row M, maturity) hold NaN coefficients and 0. */
int mcamd_price_american(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_american *am,
                         void *d_work, uint64_t work_bytes, double *h_coeffs, mcamd_american_result *res);

/* ---- The dual (upper) bound of a fitted exercise rule: Andersen and Broadie (2004), after Rogers and Haugh-Kogan ----
 * Additive to ABI version 5: first carried by the build that ships csrc/american_dual.hip (no struct of an earlier
 * call changed, so MCAMD_ABI_VERSION stays 5; a caller finds out with dlsym).
 * mcamd_price_american's out-of-sample estimate is biased LOW.  This call turns the same rule into an estimate that
 * is biased HIGH, with an honest standard error, so that the two bracket the price.  Notation as above, plus date 0:
 * t = 0, S_{p,0} = S0, d_0 = 1.  Everything is discounted to t = 0.
 *   Z_{p,j} = d_j h(S_{p,j}), j = 1..M, on the shard's OUTER paths (sim->seed, global ids path_offset + p; the
 *       product-form paths of mcamd_simulate_trajectories in the path precision).
 *   e_{p,j}, the rule says stop: for 1 <= j < M, date j is flagged regressed and d_j h(S) > phi(S) . beta_j with
 *       h(S) > 0 — the one device function both passes of mcamd_price_american decide with; e_{p,M} = 1.
 *   Point (p, j), j = 0..M-1: n_inner continuation paths start at S_{p,j}, run the remaining n_steps - s_j steps and
 *       are each paid d_i h(S) at the first date i > j where the rule says stop.  Q_{p,j} is the mean of the n_inner
 *       samples (summed in a fixed order: the same bits in every run and under any sharding).  Streams: seed =
 *       inner_seed, Philox subsequence ((path_offset + p) M + j) n_inner + i for continuation path i, from block 0
 *       (the convention of mcamd_nmc_inner: a shard draws what the whole job would).
 *   L_{p,j} = Z_{p,j} where e_{p,j}, else Q_{p,j};  pi_{p,0} = 0, pi_{p,j} = pi_{p,j-1} + L_{p,j} - Q_{p,j-1}.
 *   Dual sample u_p = max_{1 <= j <= M} (Z_{p,j} - pi_{p,j}); where e_{p,j} holds the term is evaluated as
 *       Q_{p,j-1} - pi_{p,j-1}, which it equals (so with one date, u_p is Q_{p,0} bit for bit).
 *   upper = mean of u_p over the shard, std_err = sqrt(s^2 / n).
 * Every Q is conditionally unbiased, so pi is a martingale and upper is biased HIGH whatever n_inner is: inner noise
 * only loosens the bound.  sum_q0 / n is a second LOW-biased estimate from the same rule.  The outer paths must be
 * independent of the paths the rule was fitted on (another seed than train_seed): the rule must not have seen their
 * future.  This is NOT enforced.  Exercise at t = 0: where h(S0) exceeds upper it is reported in its place with
 * std_err 0 and immediate_exercise set.  Multi-GPU: every rank bounds its shard; sum, sumsq, n and sum_q0 add.
 * sim describes the OUTER job (n_paths, path_offset, n_paths_local, seed, n_steps, precision); am->payoff,
 * exercise_every and n_basis as for mcamd_price_american, n_train and train_seed are ignored.  h_coeffs (host) is the
 * rule in exactly the layout mcamd_price_american returns: M rows of n_basis + 1 doubles, beta_j then 1 or 0; the
 * coefficients of a row flagged 0 are not read, and row M's flag is ignored (maturity always pays).
 * Requirements (MCAMD_ERR_INVALID before any device work): those of mcamd_price_american on opt, sim, payoff,
 * exercise_every, n_basis and am->reserved, plus n_inner >= 1, dual->reserved == 0, h_coeffs non-NULL, every flag
 * exactly 0 or 1, finite coefficients in every row flagged 1, (path_offset + n_paths_local) M n_inner < 2^64.  An
 * empty shard returns zeros and launches nothing. */
typedef struct mcamd_american_dual {
    uint32_t n_inner;      /* continuation paths per point, >= 1 */
    uint32_t reserved;     /* must be 0 */
    uint64_t inner_seed;   /* should differ from sim->seed */
} mcamd_american_dual;

typedef struct mcamd_american_dual_result {
    double upper;              /* sum / n (h(S0) where that is larger) */
    double std_err;            /* sqrt(s^2 / n) (0 where h(S0) was taken) */
    double ci_hi;              /* upper + 1.96 std_err */
    double sum, sumsq;         /* the shard's raw fp64 sums of u_p: what a multi-GPU caller all-reduces */
    uint64_t n;                /* outer paths (the shard) */
    double sum_q0;             /* sum of Q_{p,0}: a second lower-bound estimate from the same rule */
    double work_steps;         /* continuation kernel: 64 x the steps each wavefront ran */
    double live_steps;         /* continuation kernel: lane-steps of paths that had not stopped yet */
    uint32_t n_dates;          /* M */
    int32_t immediate_exercise;/* 1: h(S0) exceeded the estimate and replaced it */
    float outer_ms;            /* HIP-event times: store of the outer paths */
    float inner_ms;            /* continuation kernel */
    float scan_ms;             /* martingale scan */
    float total_ms;            /* the whole call's device work */
    uint32_t grid;             /* continuation kernel's launch shape */
    uint32_t block;
} mcamd_american_dual_result;

/* Bytes of the caller-owned device workspace of mcamd_american_upper_bound: with A(x) = x rounded up to 256 and
 * n = sim->n_paths_local,
 *   256 + A(n_steps n sizeof(path precision))        stored outer trajectories (step-major)
 *       + A(8 M n)                                     Q (used when d_cont is NULL)
 *       + A(8 8 (M + 1))                               coefficient table (8 doubles per date, dates 0..M)
 *       + A(8 max(2 G_store, 2 G_cont, 4 G_scan))      block records
 * G_store = min(max(ceil(ceil(n / V) / 256), 1), 2^20) with V = 4 (fp32) / 2 (fp64), G_cont = min(max(M n, 1), 8192),
 * G_scan = min(max(ceil(n / 256), 1), 8192).  Any alignment of d_work is accepted. */
int mcamd_american_dual_workspace_bytes(const mcamd_american *am, const mcamd_sim *sim,
                                        const mcamd_american_dual *dual, uint64_t *bytes);
/* d_cont (nullable, device): receives Q, M x n_paths_local doubles, Q_{p,j} at [j * n_paths_local + p]. */
int mcamd_american_upper_bound(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                               const mcamd_american *am, const mcamd_american_dual *dual, const double *h_coeffs,
                               void *d_work, uint64_t work_bytes, double *d_cont, mcamd_american_dual_result *res);

/* ---- Single-barrier options: down / up, knock-out / knock-in, call / put, discrete or continuous monitoring ----
 * Additive to ABI version 5: first carried by the build that ships csrc/barrier.hip (no struct of an earlier call
 * changed, so MCAMD_ABI_VERSION stays 5; a caller finds out with dlsym).  opt->B is the barrier level.
 * Notation of mcamd_price_paths: dt = T / n_steps; x_i = (r - v^2/2) dt + v sqrt(dt) z_i with z_i the path's normals
 * (Philox subsequence = the GLOBAL path id; the exponents are the ones mcamd_price_paths steps with); X_0 = 0,
 * X_i = X_{i-1} + x_i; S_T = S0 e^{X_n}; b = ln(B / S0).
 *   Hit test at step end i = 1..n:  down  b > X_i  (the comparison the bullet count makes, strict: the two agree path
 *       for path);  up  X_i > b.
 *   Distance:  d_i = X_i - b (down) or b - X_i (up);  d_0 = |b|.
 *   Survival weight w:
 *       MCAMD_MONITOR_DISCRETE    w = prod_i 1{no hit at i}
 *       MCAMD_MONITOR_CONTINUOUS  w = prod_i 1{no hit at i} f_i,  f_i = 1 - exp(-q_i),  q_i = 2 d_{i-1} d_i / (v^2 dt),
 *           and f_i is DEFINED as exactly 1 where q_i >= Q, Q = 38 (fp64) / 18 (fp32) in natural-log units: there
 *           e^{-q} is below 2^-54 / 2^-25 and 1 - e^{-q} rounds to 1 anyway.  The rule is part of the definition, so a
 *           restatement skips the same factors the kernel skips.
 *   h(S) = (S - K)+ for MCAMD_PAYOFF_CALL, (K - S)+ for MCAMD_PAYOFF_PUT.
 *   Sample:  knock-out  y = w h(S_T);  knock-in  y = (1 - w) h(S_T).  No rebate.
 *   price = exp(-rT) mean(y), std_err as in mcamd_finalize.
 * f_i is the probability that the Brownian bridge between two step ends stays on the live side, so the continuous w is
 * the conditional survival probability given the skeleton: nothing extra is drawn, and the sample is unbiased for the
 * continuously monitored barrier at EVERY n_steps (n_steps = 1 included).  The discrete sample prices the barrier
 * monitored at the n step ends.  Discrete DOWN_OUT / DOWN_IN calls are the bullet window's P1 = P2 = 0 and
 * P1 = 1, P2 = n_steps, sample for sample.
 * d_samples (nullable, device): n_paths_local values of the path precision; [local path] receives y.
 * res: sum / sumsq / n / price / std_err / ci_*, kernel_ms / total_ms / grid / block; work_steps = 64 x the steps each
 * wavefront ran (a knock-out wavefront leaves the step loop once every lane is knocked; a knock-in runs to maturity:
 * it needs S_T), live_steps = the lane-steps of paths not yet knocked; the other fields are 0.
 * The enqueue form leaves {sum, sumsq, 0, 0, 0, n} in d_stats (device, >= 6 doubles): mcamd_finalize_stats and one
 * all-reduce of 6 doubles serve it unchanged, and mcamd_enqueued_kernel_ms covers it.
 * Requirements (MCAMD_ERR_INVALID before any device work and before the context is looked at): opt, sim, barrier, res
 * non-NULL; kind, payoff, monitoring in range; reserved == 0; B > 0; S0 strictly on the live side (down: S0 > B, up:
 * S0 < B); use_window, P1, P2, Ik, Sk, Tk and opt->dt all 0; v > 0; sim->flags 0 or MCAMD_FLAG_LOG_SPACE; and what
 * mcamd_price_paths refuses on sim.  An empty shard returns zeros and launches nothing.
 * There is no mcamd_group_* form and no shim name: the reference has no such product.  Multi-GPU: every rank prices
 * its shard (a path's sample depends on its global id alone); the 6-double records add.  New. */
#define MCAMD_BARRIER_DOWN_OUT 0
#define MCAMD_BARRIER_DOWN_IN 1
#define MCAMD_BARRIER_UP_OUT 2
#define MCAMD_BARRIER_UP_IN 3

#define MCAMD_MONITOR_DISCRETE 0
#define MCAMD_MONITOR_CONTINUOUS 1

typedef struct mcamd_barrier {
    int32_t kind;        /* MCAMD_BARRIER_* */
    int32_t payoff;      /* MCAMD_PAYOFF_* */
    int32_t monitoring;  /* MCAMD_MONITOR_* */
    int32_t reserved;    /* must be 0 */
} mcamd_barrier;

int mcamd_price_barrier(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_barrier *barrier,
                        void *d_samples, mcamd_result *res);
int mcamd_price_barrier_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                const mcamd_barrier *barrier, void *d_samples, double *d_stats);
/* Host closed form of the CONTINUOUSLY monitored barrier, all eight kind x payoff cases, rebate 0, no dividends
 * (Reiner and Rubinstein 1991; Merton 1973).  MCAMD_ERR_INVALID for an S0 on the knocked side (or on the barrier),
 * non-positive S0, K, B, T or v, or a bad enum. */
int mcamd_barrier_price_f64(double S0, double K, double B, double T, double r, double v, int kind, int payoff,
                            double *price);

/* ---- Lookback options: floating or fixed strike, call or put, discrete or continuous monitoring ----
 * Additive to ABI version 5: first carried by the build that ships csrc/lookback.hip (no struct of an earlier call
 * changed, so MCAMD_ABI_VERSION stays 5; a caller finds out with dlsym).
 * Notation of mcamd_price_barrier: dt = T / n_steps; x_i = (r - v^2/2) dt + v sqrt(dt) z_i with z_i the path's normals
 * (Philox subsequence = the GLOBAL path id, blocks 0, 1, ...; the exponents are the ones mcamd_price_paths steps
 * with); X_0 = 0, X_i = X_{i-1} + x_i; S_T = S0 e^{X_n}.  The option is newly issued: E_0 = 0, so the extremum
 * includes S0.  A call on floating strike and a put on fixed strike need the minimum of X, the other two the maximum;
 * a path tracks only the extremum it needs, S_E = S0 e^{E_n} (S_max or S_min).
 *   MCAMD_MONITOR_DISCRETE    E_i = max(E_{i-1}, X_i)  (min for the minimum)
 *   MCAMD_MONITOR_CONTINUOUS  for the maximum:  E^ = max(E_{i-1}, X_i),  q_i = 2 (E^ - X_{i-1})(E^ - X_i) / (v^2 dt);
 *       where q_i < Q:  m_i = (X_{i-1} + X_i + sqrt(x_i^2 - 2 v^2 dt ln U_i)) / 2  and  E_i = max(E^, m_i);
 *       elsewhere E_i = E^.  For the minimum:  E^ = min(E_{i-1}, X_i),  q_i = 2 (X_{i-1} - E^)(X_i - E^) / (v^2 dt),
 *       the root enters m_i with a minus sign and E_i = min(E^, m_i).
 *       Q = 22.25 (fp32) / 36.75 (fp64) in natural-log units, just above 32 ln 2 / 53 ln 2 = -ln of the smallest
 *       uniform the generator produces.  m_i lies beyond E^ exactly when U_i < e^{-q_i}, so above Q no U that can
 *       be drawn moves the extremum and the rule changes no sample; it is part of the definition all the same, so
 *       that the kernel may skip the logarithm and the root there and a restatement skips the same steps.
 *   The uniforms come from the same key and subsequence as the normals, at Philox block 2^63 + k with k the normal
 *   block of the step (n_steps is 32-bit: the normals never get there).  fp32: word j of that block serves step
 *   4k + j, U = fma(word, 2^-32, 2^-32) in float (rocRAND's float uniform; it may round to 1, which is harmless).
 *   fp64: words (x, y) serve step 2k and (z, w) step 2k + 1, U = ((x ^ (y << 21)) + 1) 2^-53 (rocRAND's double
 *   uniform).  A shard therefore draws exactly what the whole job would.
 *   Sample, formed once per path in fp64 from the path-precision S_T and S_E (both through the same exponential, so a
 *   floating-strike path whose extremum is its last point pays exactly 0):
 *       MCAMD_LOOKBACK_FLOATING  call  y = S_T - S_min     put  y = S_max - S_T      (opt->K is ignored)
 *       MCAMD_LOOKBACK_FIXED     call  y = (S_max - K)+    put  y = (K - S_min)+
 *   price = exp(-rT) mean(y), std_err as in mcamd_finalize.
 * m_i is a draw from the law of the maximum of the Brownian bridge between the two step ends (its distribution
 * function inverted at U_i), and the bridges of different steps are independent given the step ends, so the continuous
 * sample is unbiased for the continuously monitored lookback at EVERY n_steps (n_steps = 1 included).  The discrete
 * sample prices the lookback monitored at t = 0 and the n step ends.
 * d_samples (nullable, device): n_paths_local values of the path precision; [local path] receives y.
 * res: sum / sumsq / n / price / std_err / ci_*, kernel_ms / total_ms / grid / block; work_steps = 64 x the steps each
 * wavefront ran (there is no early exit), live_steps = the lane-steps that formed m_i (continuous) or 0 (discrete);
 * the other fields are 0.
 * The enqueue form leaves {sum, sumsq, 0, 0, 0, n} in d_stats (device, >= 6 doubles): mcamd_finalize_stats and one
 * all-reduce of 6 doubles serve it unchanged, and mcamd_enqueued_kernel_ms covers it.
 * Requirements (MCAMD_ERR_INVALID before any device work and before the context is looked at): opt, sim, lookback, res
 * non-NULL; strike, payoff, monitoring in range; reserved == 0; fixed strike: K finite and positive; use_window, P1,
 * P2, Ik, Sk, Tk and opt->dt all 0; v > 0; sim->flags 0 or MCAMD_FLAG_LOG_SPACE; and what mcamd_price_paths refuses on
 * sim.  opt->B is ignored.  An empty shard returns zeros and launches nothing.
 * There is no mcamd_group_* form and no shim name: the reference has no such product.  Multi-GPU: every rank prices
 * its shard (a path's sample depends on its global id alone); the 6-double records add.  New. */
#define MCAMD_LOOKBACK_FLOATING 0
#define MCAMD_LOOKBACK_FIXED 1

typedef struct mcamd_lookback {
    int32_t strike;      /* MCAMD_LOOKBACK_* */
    int32_t payoff;      /* MCAMD_PAYOFF_* */
    int32_t monitoring;  /* MCAMD_MONITOR_* */
    int32_t reserved;    /* must be 0 */
} mcamd_lookback;

int mcamd_price_lookback(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_lookback *lookback,
                         void *d_samples, mcamd_result *res);
int mcamd_price_lookback_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                 const mcamd_lookback *lookback, void *d_samples, double *d_stats);
/* Host closed form of the CONTINUOUSLY monitored, newly issued lookback without dividends (floating strike: Goldman,
 * Sosin and Gatto 1979; fixed strike: Conze and Viswanathan 1991).  K is ignored for MCAMD_LOOKBACK_FLOATING.
 * MCAMD_ERR_INVALID for a bad enum, a non-positive or non-finite S0, T or v (and K for a fixed strike), a non-finite r,
 * and r == 0: the formulas carry v^2 / (2r), and their limit at r = 0 is left out on purpose. */
int mcamd_lookback_price_f64(double S0, double K, double T, double r, double v, int strike, int payoff, double *price);

/* ---- Basket, spread and rainbow options on d = 1..8 correlated assets ----
 * Additive to ABI version 5: first carried by the build that ships csrc/basket.hip (no struct of an earlier call
 * changed, so MCAMD_ABI_VERSION stays 5; a caller finds out with dlsym).
 * r, T, K and the barrier level B come from opt; opt->S0 and opt->v are ignored (the assets' own are in *basket), and
 * opt->B is ignored without a barrier.  d = basket->n_assets; j, k = 0..d-1 index assets; dt = T / n_steps.
 *   Correlation.  L is the lower Cholesky factor of corr[:d, :d] (corr[8 j + k] = rho_jk), computed on the host in
 *       fp64.
 *   Step.  x_{j,i} = (r - v_j^2/2) dt + sum_{k <= j} (v_j sqrt(dt) L_jk) z_{i,k}, accumulated as a chain of fused
 *       multiply-adds in ascending k that starts from the drift.  The coefficients v_j sqrt(dt) L_jk and the drifts
 *       reach the kernel in the exponent units of the precision (log2 units in fp32, 2^-16 octaves in fp64), narrowed
 *       once on the host.
 *   Log-price.  X_{j,0} = 0, X_{j,i} = X_{j,i-1} + x_{j,i};  S_{j,i} = S0_j e^{X_{j,i}}.
 *   Normals.  z_{i,k} is normal number i d + k of the path's stream: Philox subsequence = the GLOBAL path id, block
 *       (i d + k) / NB, slot (i d + k) % NB in the order mcamd_generate_normals and the other products use (NB = 4 in
 *       fp32, 2 in fp64).  With d = 1 these are the normals mcamd_price_barrier and mcamd_price_lookback step with.
 *   Aggregate A_i of the prices after step i:
 *       MCAMD_BASKET_ARITHMETIC  A = sum_j w_j S_j      (w_j of any sign: spreads, exchange options)
 *       MCAMD_BASKET_GEOMETRIC   A = prod_j S_j^{w_j}   = exp(sum_j w_j (ln S0_j + X_j))
 *       MCAMD_BASKET_BEST_OF     A = max_j w_j S_j      = exp(max_j (ln(w_j S0_j) + X_j))   (w_j > 0; w_j = 1 / S0_j:
 *       MCAMD_BASKET_WORST_OF    A = min_j w_j S_j      = exp(min_j (ln(w_j S0_j) + X_j))    performances)
 *       Geometric, best-of and worst-of aggregate in log space in the path precision (the geometric sum is a chain of
 *       fused multiply-adds in ascending j that starts from sum_j w_j ln S0_j) and take one exponential per path;
 *       arithmetic takes d exponentials per path at maturity only, S_j in the path precision, and sums w_j S_j in
 *       fp64 in ascending j by fused multiply-adds from 0.
 *   Sample, formed once per path in fp64:  call  y = (A_n - K)+;  put  y = (K - A_n)+.
 *   Barrier (MCAMD_BASKET_BEST_OF and MCAMD_BASKET_WORST_OF only), monitored at the n_steps step ends only: the hit
 *       test compares the log aggregate with ln B in the path precision; "down" hits at A_i <= B, "up" at A_i >= B.
 *       Knock-out pays y if the path never hit, knock-in pays y if it hit.  No rebate.  There is no continuous
 *       monitoring, on purpose: the law of the extremum of a minimum (or maximum) over correlated Brownian bridges has
 *       no closed form to weight or sample a step with.
 *   price = exp(-rT) mean(y), std_err as in mcamd_finalize.
 * The sample is the exact law of correlated geometric Brownian motion at the step ends for every n_steps, so terminal
 * products are unbiased at n_steps = 1.
 * d_samples (nullable, device): n_paths_local values of the path precision; [local path] receives y.
 * res: sum / sumsq / n / price / std_err / ci_*, kernel_ms / total_ms / grid / block; work_steps = 64 x the steps each
 * wavefront ran (a knock-out wavefront leaves the step loop once every lane has hit), live_steps = the lane-steps of
 * paths not yet hit (0 without a barrier); the other fields are 0.
 * The enqueue form leaves {sum, sumsq, 0, 0, 0, n} in d_stats (device, >= 6 doubles): mcamd_finalize_stats and one
 * all-reduce of 6 doubles serve it unchanged, and mcamd_enqueued_kernel_ms covers it.
 * Requirements (MCAMD_ERR_INVALID before any device work and before the context is looked at): opt, sim, basket, res
 * non-NULL; n_assets in 1..MCAMD_BASKET_MAX_ASSETS; kind, payoff, barrier in range; reserved[0] == reserved[1] == 0;
 * every S0_j and v_j finite and positive; every w_j finite, and positive for best-of / worst-of, not all zero for
 * arithmetic / geometric; K finite and >= 0; corr with a diagonal of exactly 1, exactly symmetric, no entry beyond
 * +-1, and positive definite: every Cholesky pivot (the square of the diagonal entry of L) above 1e-12 — the rule is
 * arbitrary but fixed, and it refuses rho = +-1 (use fewer assets); a barrier needs best-of or worst-of, B > 0 and A_0
 * strictly on the live side (down: A_0 > B, up: A_0 < B); use_window, P1, P2, Ik, Sk, Tk and opt->dt all 0;
 * sim->flags 0 or MCAMD_FLAG_LOG_SPACE; and what mcamd_price_paths refuses on sim.  corr entries beyond n_assets
 * are ignored, as are S0, v and w beyond it.  An empty shard returns zeros and launches nothing.
 * There is no mcamd_group_* form and no shim name: the reference has no such product.  Multi-GPU: every rank prices
 * its shard (a path's sample depends on its global id alone); the 6-double records add.  New. */
#define MCAMD_BASKET_MAX_ASSETS 8
#define MCAMD_BASKET_ARITHMETIC 0
#define MCAMD_BASKET_GEOMETRIC 1
#define MCAMD_BASKET_BEST_OF 2
#define MCAMD_BASKET_WORST_OF 3

#define MCAMD_BASKET_NO_BARRIER 0
#define MCAMD_BASKET_DOWN_OUT 1
#define MCAMD_BASKET_DOWN_IN 2
#define MCAMD_BASKET_UP_OUT 3
#define MCAMD_BASKET_UP_IN 4

typedef struct mcamd_basket {
    int32_t n_assets;    /* d, 1..MCAMD_BASKET_MAX_ASSETS */
    int32_t kind;        /* MCAMD_BASKET_ARITHMETIC .. MCAMD_BASKET_WORST_OF */
    int32_t payoff;      /* MCAMD_PAYOFF_* */
    int32_t barrier;     /* MCAMD_BASKET_NO_BARRIER .. MCAMD_BASKET_UP_IN */
    int32_t reserved[2]; /* must be 0 */
    double S0[8];        /* spots */
    double v[8];         /* volatilities */
    double w[8];         /* weights */
    double corr[64];     /* correlations, row-major with stride 8 */
} mcamd_basket;

int mcamd_price_basket(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_basket *basket,
                       void *d_samples, mcamd_result *res);
int mcamd_price_basket_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                               const mcamd_basket *basket, void *d_samples, double *d_stats);
/* Host closed form of the geometric basket of any d, a lognormal: ln A_T is normal with mean
 * m = sum_j w_j (ln S0_j + (r - v_j^2/2) T) and variance s^2 = T w'(v o corr o v)w, so the call is
 * e^{-rT} (e^{m + s^2/2} N(d1) - K N(d1 - s)) with d1 = (m - ln K) / s + s (K = 0: the discounted forward).  kind,
 * barrier and reserved of *basket are not read; payoff is.  Refuses what mcamd_price_basket refuses of n_assets, payoff,
 * S0, v, w (not all zero), corr, K, T and r. */
int mcamd_basket_geometric_price_f64(const mcamd_basket *basket, double K, double T, double r, double *price);
/* Host closed form of the option to exchange b S2 for a S1, (a S1 - b S2)+ (Margrabe 1978), with a_S1 = a S1(0) and
 * b_S2 = b S2(0) both positive: a_S1 N(d1) - b_S2 N(d2), d1 = (ln(a_S1 / b_S2) + s^2 T / 2) / (s sqrt T),
 * d2 = d1 - s sqrt T, s^2 = v1^2 + v2^2 - 2 rho v1 v2.  The rate drops out.  It is mcamd_price_basket's arithmetic call
 * with w = (a, -b) and K = 0.  MCAMD_ERR_INVALID for non-finite or non-positive a_S1, b_S2, T, v1 or v2, or rho not
 * strictly inside (-1, 1). */
int mcamd_exchange_price_f64(double a_S1, double b_S2, double T, double v1, double v2, double rho, double *price);

/* ---- Asian (average-rate) options: arithmetic or geometric average, fixed or floating strike, call or put ----
 * Additive to ABI version 5: first carried by the build that ships csrc/asian.hip (no struct of an earlier call
 * changed, so MCAMD_ABI_VERSION stays 5; a caller finds out with dlsym).
 * Notation of mcamd_price_lookback: dt = T / n_steps; x_i is the exponent of step i, (r - v^2/2) dt + v sqrt(dt) z_i
 * with z_i the path's normals (Philox subsequence = the GLOBAL path id, blocks 0, 1, ...; the exponents are the ones
 * mcamd_price_paths steps with); X_0 = 0, X_i = X_{i-1} + x_i in the path precision.  The averaging dates are the step
 * ends i = 1..n and, with include_spot, t = 0: m = n + include_spot dates.
 *   MCAMD_ASIAN_ARITHMETIC  prices in the product form of the trajectory-store kernel: P_0 = S0, P_i = P_{i-1} e^{x_i},
 *       so P_i is bit for bit what mcamd_simulate_trajectories stores for that path.  Their sum is accumulated in fp64
 *       in ascending i from S0 (include_spot) or 0; A = sum / m in fp64; S_T = P_n.
 *   MCAMD_ASIAN_GEOMETRIC   L = sum_{i=1..n} X_i, accumulated in the path precision in ascending i (the spot
 *       contributes 0); G = S0 e^{L (1/m)} with 1/m narrowed once on the host, and S_T = S0 e^{X_n}, both through the
 *       exponential that ends a log-space path of mcamd_price_paths.  A floating-strike job with n = 1 and no spot
 *       therefore pays exactly 0.  No exponential is taken inside the step loop.
 *   Sample, formed once per path in fp64 (G in place of A for the geometric average):
 *       MCAMD_ASIAN_FIXED     call  y = (A - K)+      put  y = (K - A)+      (average price)
 *       MCAMD_ASIAN_FLOATING  call  y = (S_T - A)+    put  y = (A - S_T)+    (average strike; opt->K is ignored)
 *   price = exp(-rT) mean(y), std_err as in mcamd_finalize.
 *   MCAMD_ASIAN_CONTROL_GEOMETRIC (arithmetic jobs only): the kernel carries L beside the prices and forms g, the
 *       geometric sample of the same strike, payoff and include_spot exactly as the geometric job forms it in fp64;
 *       c = g - mu_g with mu_g = e^{rT} mcamd_asian_geometric_price_f64(...) computed on the host in fp64.  The call
 *       returns sum, sumsq, sum_c, sum_cc, sum_yc and finalizes as mcamd_finalize_cv does (cv_beta and cv_rho are
 *       filled).  The two payoffs correlate at 0.999 and more for usual inputs, which shrinks the standard error
 *       25 to 40 times.
 * The exponents are the exact law of geometric Brownian motion at the step ends, so the discrete average is sampled
 * without bias at every n_steps (n_steps = 1 included).
 * d_samples (nullable, device): n_paths_local values of the path precision; [local path] receives y, never the
 * control-adjusted value.
 * res: sum / sumsq / n / price / std_err / ci_*, kernel_ms / total_ms / grid / block; with the control also sum_c /
 * sum_cc / sum_yc / cv_beta / cv_rho; work_steps = 64 x the steps each wavefront ran (there is no early exit),
 * live_steps = 0; the other fields are 0.
 * The enqueue form leaves {sum y, sum y^2, sum c, sum c^2, sum y c, n} in d_stats (device, >= 6 doubles; the three
 * middle entries are 0 without the control): mcamd_finalize_stats (control_variate = 1 for a controlled job) and one
 * all-reduce of 6 doubles serve it unchanged, and mcamd_enqueued_kernel_ms covers it.
 * Requirements (MCAMD_ERR_INVALID before any device work and before the context is looked at): opt, sim, asian, res
 * non-NULL; average, strike, payoff, include_spot, control in range; reserved == 0; no control on a geometric job;
 * fixed strike: K finite and positive; use_window, P1, P2, Ik, Sk, Tk and opt->dt all 0; v > 0; sim->flags 0 or
 * MCAMD_FLAG_LOG_SPACE; and what mcamd_price_paths refuses on sim (a controlled job also needs S0 > 0, for mu_g).
 * opt->B is ignored.  An empty shard returns zeros and launches nothing; its enqueue form writes a zero record in
 * stream order.
 * There is no mcamd_group_* form and no shim name: the reference has no such product.  Multi-GPU: every rank prices
 * its shard (a path's sample depends on its global id alone); the 6-double records add.  New. */
#define MCAMD_ASIAN_ARITHMETIC 0
#define MCAMD_ASIAN_GEOMETRIC 1
#define MCAMD_ASIAN_FIXED 0      /* average price:  call (A - K)+,   put (K - A)+ */
#define MCAMD_ASIAN_FLOATING 1   /* average strike: call (S_T - A)+, put (A - S_T)+; opt->K ignored */
#define MCAMD_ASIAN_CONTROL_NONE 0
#define MCAMD_ASIAN_CONTROL_GEOMETRIC 1   /* arithmetic jobs only */

typedef struct mcamd_asian {
    int32_t average;       /* MCAMD_ASIAN_ARITHMETIC / MCAMD_ASIAN_GEOMETRIC */
    int32_t strike;        /* MCAMD_ASIAN_FIXED / MCAMD_ASIAN_FLOATING */
    int32_t payoff;        /* MCAMD_PAYOFF_* */
    int32_t include_spot;  /* 0 / 1: t = 0 is an averaging date */
    int32_t control;       /* MCAMD_ASIAN_CONTROL_* */
    int32_t reserved;      /* must be 0 */
} mcamd_asian;

int mcamd_price_asian(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_asian *asian,
                      void *d_samples, mcamd_result *res);
int mcamd_price_asian_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_asian *asian,
                              void *d_samples, double *d_stats);
/* Host closed form of the DISCRETE geometric average of the definitions above (a lognormal at every n_steps), no
 * dividends.  With mu = r - v^2/2:  M = ln S0 + mu dt n(n+1) / (2m),  s^2 = v^2 dt n(n+1)(2n+1) / (6 m^2);
 *   fixed call    e^{-rT} (e^{M + s^2/2} N(d1) - K N(d1 - s)),  d1 = (M - ln K) / s + s;
 *   floating call e^{-rT} (F1 N(d1) - F2 N(d1 - s_f)),  F1 = S0 e^{rT},  F2 = e^{M + s^2/2},
 *                 s_f^2 = v^2 T + s^2 - v^2 dt n(n+1) / m,  d1 = (ln(F1 / F2) + s_f^2 / 2) / s_f;  0 where s_f^2 <= 0
 *                 (n = 1 without the spot: the average is S_T itself);
 *   puts by parity: call - e^{-rT} (F2 - K), and call - e^{-rT} (F1 - F2).
 * N is the erfc form of mcamd_bs_call_f64.  K is ignored for MCAMD_ASIAN_FLOATING.  MCAMD_ERR_INVALID for a bad enum
 * or include_spot, n_steps == 0, a non-positive or non-finite S0, T or v (and K for a fixed strike) and a non-finite
 * r. */
int mcamd_asian_geometric_price_f64(double S0, double K, double T, double r, double v, uint32_t n_steps,
                                    int include_spot, int strike, int payoff, double *price);

/* ---- Worst-of autocallable notes on d = 1..8 correlated assets: early redemption, snowball coupon, knock-in put ----
 * Additive to ABI version 5: first carried by the build that ships csrc/autocall.hip (no struct of an earlier call
 * changed, so MCAMD_ABI_VERSION stays 5; a caller finds out with dlsym).
 * Notional 1; performances are relative to each asset's own spot, so there are no spots and no weights.  r and T come
 * from opt; opt->S0, opt->v, opt->K and opt->B are ignored.  d = autocall->n_assets; dt = T / n_steps.
 *   Log-returns.  X_{j,i} and the normals z_{i,k} are exactly those of mcamd_price_basket: the same Cholesky factor,
 *       drifts and coefficients in the exponent units of the path precision, the same chain of fused multiply-adds in
 *       ascending k from the drift, the same Philox subsequence (the GLOBAL path id), block and slot order.
 *       l_i = min_j X_{j,i} is the log of the worst performance after step i, in the path precision.
 *   Observation dates q = 1..M at the ends of steps s_q = q observe_every, M = n_steps / observe_every; t_q = s_q dt.
 *   Levels and payments, built on the host in fp64:  L_q = call_level - (q - 1) call_step_down, and ln L_q narrowed
 *       once to the path precision in exponent units;  pay_q = (1 + q coupon) e^{r (T - t_q)}, the redemption with its
 *       snowball coupon carried to maturity money, kept as a double.
 *   Autocall.  The path is called at the first date q >= first_call_date with l_{s_q} >= ln L_q (compared in the path
 *       precision); date M, maturity, is one of them.  A called path has y = pay_q exactly.
 *   Knock-in, compared in the path precision as the basket barrier is:
 *       MCAMD_AUTOCALL_KI_NONE         never;
 *       MCAMD_AUTOCALL_KI_AT_MATURITY  hit if l_n <= ln ki_level;
 *       MCAMD_AUTOCALL_KI_EVERY_STEP   hit if l_i <= ln ki_level at any step end i = 1..n.
 *   A path never called has y = min(A_n, 1) if knocked in and y = 1 otherwise, with A_n = e^{l_n} through the
 *       exponential that ends a log-space path, formed once in fp64.  At date M the call test comes first: a path
 *       called there is paid pay_M whatever its knock-in state.
 *   price = exp(-rT) mean(y), std_err as in mcamd_finalize: y is maturity money, so mcamd_finalize and
 *       mcamd_finalize_stats serve unchanged although the payment time differs from path to path.
 * No exponential is taken before maturity.  A wavefront whose lanes have all been called leaves the step loop at the
 * end of its step group (the steps that consume whole Philox blocks: 1, 2 or 4).
 * d_samples (nullable, device): n_paths_local values of the path precision; [local path] receives y, (float)pay_q for a
 * called path in fp32.
 * res: price / std_err / ci_* / sum / sumsq / n; n_called = the paths called, sum_t_call = the sum of their t_q,
 * n_knocked_in = the paths not called and knocked in; work_steps = 64 x the steps each wavefront ran, live_steps = the
 * lane-steps of paths not yet called (s_q of a called path, n_steps of any other); kernel_ms / total_ms / grid / block.
 * The enqueue form leaves {sum, sumsq, n_called, sum_t_call, n_knocked_in, n} in d_stats (device, >= 6 doubles):
 * mcamd_finalize_stats with control_variate = 0 and one all-reduce of 6 doubles serve it, and mcamd_enqueued_kernel_ms
 * covers it.
 * Requirements (MCAMD_ERR_INVALID before any device work and before the context is looked at): opt, sim, autocall, res
 * non-NULL; what mcamd_price_basket refuses of n_assets, v and corr, with the same Cholesky pivot rule; reserved[0] ==
 * reserved[1] == 0; ki_monitoring in range; observe_every >= 1, n_steps % observe_every == 0 and
 * 1 <= M <= MCAMD_AUTOCALL_MAX_DATES; 1 <= first_call_date <= M; coupon finite and >= 0; call_level finite;
 * call_step_down finite and >= 0; L_M > 0; with a knock-in 0 < ki_level <= 1 and ki_level < L_M (ki_level is ignored
 * without one); use_window, P1, P2, Ik, Sk, Tk and opt->dt all 0; sim->flags 0 or MCAMD_FLAG_LOG_SPACE; and what
 * mcamd_price_paths refuses on sim.  corr entries beyond n_assets are ignored, as is v beyond it.  An empty shard
 * returns zeros and launches nothing; its enqueue form writes a zero record in stream order.
 * Out of scope: memory or conditional coupons (the coupon is paid with the redemption only), continuous knock-in
 * (the minimum of correlated Brownian bridges has no closed-form law), Greeks, a mcamd_group_* form and a shim name
 * (the reference has no such product).  Multi-GPU: every rank prices its shard (a path's sample depends on its global
 * id alone); the 6-double records add.  New. */
#define MCAMD_AUTOCALL_MAX_DATES 64
#define MCAMD_AUTOCALL_KI_NONE 0
#define MCAMD_AUTOCALL_KI_AT_MATURITY 1
#define MCAMD_AUTOCALL_KI_EVERY_STEP 2

typedef struct mcamd_autocall {
    int32_t n_assets;         /* d, 1..MCAMD_BASKET_MAX_ASSETS */
    int32_t ki_monitoring;    /* MCAMD_AUTOCALL_KI_* */
    uint32_t observe_every;   /* steps between observation dates; divides n_steps */
    uint32_t first_call_date; /* 1..M: the first date the note can be called at */
    int32_t reserved[2];      /* must be 0 */
    double call_level;        /* L_1, as a performance (1 = the spots) */
    double call_step_down;    /* L_q = call_level - (q - 1) call_step_down */
    double coupon;            /* per date, snowball: a path called at date q receives 1 + q coupon */
    double ki_level;          /* as a performance, in (0, 1] and below L_M */
    double v[8];              /* volatilities */
    double corr[64];          /* correlations, row-major with stride 8 */
} mcamd_autocall;

typedef struct mcamd_autocall_result {
    double price;          /* exp(-rT) * sum / n */
    double std_err;
    double ci_lo;          /* price -/+ 1.96 std_err */
    double ci_hi;
    double sum;            /* sum of the samples (maturity money) */
    double sumsq;
    uint64_t n;            /* paths in the shard */
    uint64_t n_called;     /* of them, called at some date (maturity included) */
    double sum_t_call;     /* sum of t_q over the called paths: sum_t_call / n_called is the mean call time */
    uint64_t n_knocked_in; /* paths not called and knocked in */
    double work_steps;     /* 64 x the steps each wavefront ran */
    double live_steps;     /* lane-steps of paths not yet called */
    float kernel_ms;
    float total_ms;
    uint32_t grid;
    uint32_t block;
} mcamd_autocall_result;

int mcamd_price_autocall(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_autocall *autocall,
                         void *d_samples, mcamd_autocall_result *res);
int mcamd_price_autocall_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                 const mcamd_autocall *autocall, void *d_samples, double *d_stats);
/* Host closed form of the note on one asset with one date (d = 1, M = 1), for MCAMD_AUTOCALL_KI_NONE and
 * MCAMD_AUTOCALL_KI_AT_MATURITY.  With d2(x) = (-ln x + (r - v^2/2) T) / (v sqrt T), d1 = d2 + v sqrt T, L = call_level,
 * B = ki_level, c = coupon:
 *   price = e^{-rT} [(1 + c) N(d2(L)) + (N(d2(B)) - N(d2(L))) + e^{rT} N(-d1(B))]      (knock-in at maturity)
 *   price = e^{-rT} [(1 + c) N(d2(L)) + 1 - N(d2(L))]                                   (no knock-in)
 * N is the erfc form of mcamd_bs_call_f64.  Makes the refusals of mcamd_price_autocall that these arguments can meet:
 * T and v finite and positive, r finite, coupon finite and >= 0, call_level finite and positive, with a knock-in
 * 0 < ki_level <= 1 and ki_level < call_level; and refuses MCAMD_AUTOCALL_KI_EVERY_STEP, which has no closed form. */
int mcamd_autocall_single_date_price_f64(double T, double r, double v, double call_level, double coupon,
                                         double ki_level, int ki_monitoring, double *price);

/* ---- Local volatility: European and single-barrier options under a surface sigma(t, ln(S / S0)), dividend yield q ----
 * Additive to ABI version 5: first carried by the build that ships csrc/localvol.hip (no struct of an earlier call
 * changed, so MCAMD_ABI_VERSION stays 5; a caller finds out with dlsym).  The first model here that is not constant-
 * volatility geometric Brownian motion: log-Euler with the volatility frozen over each step, one normal per step from
 * the stream mcamd_price_barrier draws from, nothing else drawn.  All path arithmetic is in the path precision; the
 * sample is formed once per path in fp64.  opt->v is ignored (and may hold anything).
 *   Surface.  n_t time slices of n_x nodes; node k lies at x_k = x_min + k dx, dx = (x_max - x_min) / (n_x - 1), in
 *       x = ln(S / S0) with S0 = opt->S0 of the pricing call.  h_sigma: n_t rows of n_x doubles, [j * n_x + k] =
 *       sigma_j(x_k), every entry finite and > 0.  The slices divide [0, opt->T] equally and are chosen by step index:
 *       step i = 0..n-1 (from t_i to t_{i+1}, n = n_steps) uses row(i) = floor(i n_t / n), in 64-bit integers; n_t need
 *       not divide n and may exceed it (rows are then skipped).
 *   Interpolation in x (linear; flat outside [x_min, x_max], which is the clamp):
 *       u = min(max((X - x_min) (1 / dx), 0), n_x - 1),  k = min(floor(u), n_x - 2),  f = u - k,
 *       sigma = fma(f, slope_k, sigma_k),  slope_k = sigma_{k+1} - sigma_k.
 *       slope_k and 1 / dx are formed in double on the host and then narrowed to the path precision, as sigma_k and
 *       x_min are.
 *   Step.  dt = T / n, X_0 = 0;  s_{i+1} = sigma(row(i), X_i);
 *       X_{i+1} = X_i + (((r - q) - s_{i+1}^2 / 2) dt + s_{i+1} sqrt(dt) z_{i+1}),
 *       z the path's normals exactly as mcamd_price_barrier draws them (Philox subsequence = the GLOBAL path id, blocks
 *       0, 1, ...: 4 normals per block in fp32, 2 in fp64).  S_T = S0 e^{X_n}.
 *   h(S) = (S - K)+ for MCAMD_PAYOFF_CALL, (K - S)+ for MCAMD_PAYOFF_PUT.
 *   Barrier.  localvol->barrier is MCAMD_LOCALVOL_NO_BARRIER (y = h(S_T); monitoring is checked but plays no part) or
 *       MCAMD_BARRIER_DOWN_OUT .. MCAMD_BARRIER_UP_IN at the level opt->B.  With b = ln(B / S0), the hit tests, the
 *       distances d_i (d_0 = |b|), the survival weight w, the knock-out / knock-in samples and the cut Q (38 in fp64,
 *       18 in fp32) are exactly those of mcamd_price_barrier, with the step's own frozen volatility in the bridge factor:
 *           q_i = 2 d_{i-1} d_i / (s_i^2 dt).
 *       That factor is the exact conditional survival probability where sigma does not depend on x (a surface that
 *       varies in time only: the continuous sample is then unbiased at every n_steps); where sigma varies in x the
 *       bridge between two step ends is not Brownian with volatility s_i and the weight carries an O(dt) bias, on top of
 *       the O(dt) weak error of the Euler step itself.
 *   price = exp(-rT) mean(y), std_err as in mcamd_finalize.
 * A flat surface with q = 0 is mcamd_price_barrier sample for sample up to rounding; a surface that varies in time only
 * prices to Black-Scholes (mcamd_bs_price_f64) at the rms volatility at every n_steps.
 * A surface is an immutable object: mcamd_localvol_surface_create checks the grid and the table, builds the (sigma_k,
 * slope_k) pair tables in fp32 and fp64 (the slope of a row's last node is 0 and never read) and uploads both,
 * synchronously, into device memory the surface owns.  An enqueued call therefore never races a later upload.  Several
 * surfaces may be alive in one context; a surface serves the context it was created on and no other; destroy it once
 * the work enqueued with it has finished and before its context is destroyed.  mcamd_localvol_surface_destroy(NULL) is
 * MCAMD_OK.
 * d_samples (nullable, device): n_paths_local values of the path precision; [local path] receives y.
 * res: filled as mcamd_price_barrier fills it; work_steps = 64 x the steps each wavefront ran (a knock-out wavefront
 * leaves the step loop at the first Philox-block end where every lane is knocked), live_steps = the lane-steps of paths
 * not yet knocked (every lane-step without a barrier).  The enqueue form leaves {sum, sumsq, 0, 0, 0, n} in d_stats:
 * mcamd_finalize_stats serves it and mcamd_enqueued_kernel_ms covers it.
 * Requirements (MCAMD_ERR_INVALID before any device work; for the pricing calls before the context is looked at): no
 * NULL pointer (d_samples apart); grid: n_t >= 1, n_x >= 2, n_t n_x <= MCAMD_LOCALVOL_MAX_NODES, x_min and x_max finite,
 * x_min < x_max, every table entry finite and > 0; payoff, barrier, monitoring in range; reserved == 0; q finite; with a
 * barrier B > 0 and S0 strictly on the live side; use_window, P1, P2, Ik, Sk, Tk and opt->dt all 0; sim->flags 0 or
 * MCAMD_FLAG_LOG_SPACE; what mcamd_price_paths refuses on sim (its fp64 exponent-range bound taken at r - q and the
 * surface's largest entry); a surface created on another context.  An empty shard returns zeros and launches nothing.
 * There is no mcamd_group_* form and no shim name: the reference has no such model.  New. */
#define MCAMD_LOCALVOL_NO_BARRIER (-1)
#define MCAMD_LOCALVOL_MAX_NODES 2048   /* n_t n_x: the fp64 pair table is then 32 KiB of LDS per workgroup */

typedef struct mcamd_localvol_grid {
    uint32_t n_t;        /* time slices, >= 1 */
    uint32_t n_x;        /* nodes per slice, >= 2 */
    double x_min;        /* ln(S / S0) of node 0 */
    double x_max;        /* ln(S / S0) of node n_x - 1 */
} mcamd_localvol_grid;

typedef struct mcamd_localvol {
    int32_t payoff;      /* MCAMD_PAYOFF_* */
    int32_t barrier;     /* MCAMD_LOCALVOL_NO_BARRIER or MCAMD_BARRIER_* */
    int32_t monitoring;  /* MCAMD_MONITOR_* */
    int32_t reserved;    /* must be 0 */
    double q;            /* continuous dividend yield */
} mcamd_localvol;

typedef struct mcamd_localvol_surface mcamd_localvol_surface;

int mcamd_localvol_surface_create(mcamd_ctx *ctx, const mcamd_localvol_grid *grid, const double *h_sigma,
                                  mcamd_localvol_surface **surface);
int mcamd_localvol_surface_destroy(mcamd_localvol_surface *surface);
int mcamd_price_localvol(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_localvol *localvol,
                         const mcamd_localvol_surface *surface, void *d_samples, mcamd_result *res);
int mcamd_price_localvol_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                 const mcamd_localvol *localvol, const mcamd_localvol_surface *surface, void *d_samples,
                                 double *d_stats);
/* Host: the volatility step `step` (0 .. n_steps - 1) of a path standing at x = ln(S / S0) uses, by the definition
 * above evaluated in double.  Refuses what mcamd_localvol_surface_create refuses of grid and h_sigma, n_steps == 0,
 * step >= n_steps and a NaN x. */
int mcamd_localvol_sigma_f64(const mcamd_localvol_grid *grid, const double *h_sigma, uint32_t n_steps, uint32_t step,
                             double x, double *sigma);
/* Host closed form: Black-Scholes with a continuous dividend yield q (Merton 1973),
 *   call = S0 e^{-qT} N(d1) - K e^{-rT} N(d2),  put = K e^{-rT} N(-d2) - S0 e^{-qT} N(-d1),
 *   d1 = (ln(S0 / K) + (r - q + v^2/2) T) / (v sqrt T),  d2 = d1 - v sqrt T,  N the erfc form of mcamd_bs_call_f64.
 * Refuses non-finite arguments, S0, K, T or v <= 0 and a bad payoff. */
int mcamd_bs_price_f64(double S0, double K, double T, double r, double q, double v, int payoff, double *price);
/* Host: the inverse of mcamd_bs_price_f64 in v.  With F = S0 e^{(r-q)T} and D = e^{-rT} the price of a vanilla lies
 * strictly between lower = D max(+-(F - K), 0) (+ call, - put) and upper = S0 e^{-qT} (call) or K D (put), and grows
 * with v from one to the other.  Returns the v with mcamd_bs_price_f64(S0, K, T, r, q, v, payoff) = price, found by a
 * bracketed iteration — Newton steps kept inside the bracket, a bisection wherever a step would leave it or shrinks it
 * too slowly — with a capped iteration count: it terminates for every admissible input, also one ulp inside a bound.
 * Refuses (MCAMD_ERR_INVALID, *vol = NaN) non-finite arguments, S0, K or T <= 0, a bad payoff and a price that is not
 * strictly inside (lower, upper).  New. */
int mcamd_bs_implied_vol_f64(double S0, double K, double T, double r, double q, int payoff, double price, double *vol);

/* ---- Local-volatility smile: n_expiries x n_strikes vanillas priced on ONE set of local-volatility paths ----
 * Additive to ABI version 5: first carried by the build that ships csrc/localvol_smile.hip (MCAMD_ABI_VERSION stays 5;
 * a caller finds out with dlsym).  "smile" is the strike-by-expiry set of options; "grid" stays the surface's node grid.
 *   Paths.  Those of mcamd_price_localvol with MCAMD_LOCALVOL_NO_BARRIER, draw for draw and operation for operation:
 *       the same surface lookup with row(i) = floor(i n_t / n_steps) over the WHOLE n_steps, the same log-Euler step in
 *       the path precision with dt = T / n_steps, the same Philox subsequence (the GLOBAL path id).  Nothing else is
 *       drawn.  opt->v and opt->K are ignored (and may hold anything).
 *   Expiries.  h_expiry_steps[m], m = 0 .. n_expiries - 1, strictly ascending with 1 <= s_m <= n_steps.  Expiry m is the
 *       time t_m = s_m (T / n_steps); its spot is S_m = S0 e^{X_{s_m}}, evaluated exactly as mcamd_price_localvol
 *       evaluates S_T, in the path precision.  The last expiry need not be n_steps: the paths stop after the last
 *       expiry, but the rows are still chosen against n_steps.
 *   Nodes.  Node (m, k) pairs expiry m with the strike K_k = h_strikes[k], k = 0 .. n_strikes - 1, and has the
 *       undiscounted sample h = max(S_m - K_k, 0) (MCAMD_PAYOFF_CALL) or max(K_k - S_m, 0) (MCAMD_PAYOFF_PUT; one
 *       payoff for every node), formed in the path precision from K_k narrowed to the path precision, then widened
 *       to double.  sum[m n_strikes + k] = sum of h and sumsq[m n_strikes + k] = sum of h^2 over the shard's paths,
 *       both accumulated in fp64.
 *   h_stats: 2 n_expiries n_strikes doubles, all the sums first, then all the sums of squares.
 *   price[m][k] = e^{-r t_m} sum / n,  std_err[m][k] = e^{-r t_m} sqrt(s^2 / n) with mcamd_finalize's sample variance
 *       (mcamd_finalize_smile).  NOTE the discount runs to the node's OWN expiry t_m, not over the full T as in every
 *       other call of this header: node (m, k) is an option that expires at t_m.
 *   res: n, kernel_ms (the path kernel), total_ms (with the sum of the per-wavefront records), grid, block;
 *       work_steps = 64 x the steps each wavefront ran (s_last per wavefront that holds a path), live_steps = work_steps;
 *       sum, sumsq, price, std_err, ci_lo, ci_hi are those of the LAST node (last expiry, last strike), finalized with
 *       t of the last expiry.  Everything else in res is zero.
 *   d_spots (nullable, device): n_expiries x n_paths_local values of the path precision, expiry-major:
 *       [m n_paths_local + local path] receives S_m — for path-by-path tests, or for other European payoffs at those
 *       dates.
 *   The enqueue form leaves the same 2 n_expiries n_strikes doubles in d_stats, followed by one more double that holds
 *   n (the shard's paths): d_stats has room for 2 n_expiries n_strikes + 1 doubles.  Shards add element by element;
 *   mcamd_finalize_smile then serves the total.  mcamd_enqueued_kernel_ms covers the path kernel.  h_expiry_steps
 *   and h_strikes are read before the call returns.  Results do not depend on earlier calls, and two runs of one job
 *   give the same bits.
 * mcamd_finalize_smile (host): stats as above with n paths, opt->r and opt->T, n_steps and the expiry steps of the job;
 * h_price and h_std_err receive n_expiries x n_strikes doubles each, [m n_strikes + k].  Of *smile it reads n_expiries
 * and n_strikes alone (payoff, reserved and q may hold anything), so it serves mcamd_price_heston_smile's sums as well.
 * Requirements (MCAMD_ERR_INVALID before any device work; everything that needs neither the surface nor the context
 * comes before either is looked at): no NULL pointer (d_spots apart); payoff in range; reserved == 0; n_expiries in
 * 1 .. MCAMD_SMILE_MAX_EXPIRIES, n_strikes in 1 .. MCAMD_SMILE_MAX_STRIKES; expiry steps strictly ascending in
 * 1 .. n_steps; every strike finite and > 0; q finite; use_window, P1, P2, Ik, Sk, Tk and opt->dt all 0; sim->flags 0 or
 * MCAMD_FLAG_LOG_SPACE; what mcamd_price_paths refuses on sim (its fp64 exponent-range bound taken as
 * mcamd_price_localvol takes it, at r - q and the surface's largest entry); S0 > 0; then the surface, a surface created
 * on another context included; then the context.  An empty shard returns zeros and launches nothing.  There is no
 * mcamd_group_* form and no shim name.  Barriers, mixed call / put nodes and Greeks are not offered.  New. */
#define MCAMD_SMILE_MAX_STRIKES  64
#define MCAMD_SMILE_MAX_EXPIRIES 32

typedef struct mcamd_smile {
    int32_t  payoff;       /* MCAMD_PAYOFF_CALL or _PUT, for every node */
    uint32_t n_expiries;   /* 1 .. MCAMD_SMILE_MAX_EXPIRIES */
    uint32_t n_strikes;    /* 1 .. MCAMD_SMILE_MAX_STRIKES */
    int32_t  reserved;     /* must be 0 */
    double   q;            /* continuous dividend yield */
} mcamd_smile;

int mcamd_price_localvol_smile(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_smile *smile,
                               const uint32_t *h_expiry_steps, const double *h_strikes,
                               const mcamd_localvol_surface *surface, void *d_spots, double *h_stats, mcamd_result *res);
int mcamd_price_localvol_smile_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                       const mcamd_smile *smile, const uint32_t *h_expiry_steps, const double *h_strikes,
                                       const mcamd_localvol_surface *surface, void *d_spots, double *d_stats);
int mcamd_finalize_smile(const double *stats, uint64_t n, const mcamd_option *opt, uint32_t n_steps,
                         const mcamd_smile *smile, const uint32_t *h_expiry_steps, double *h_price, double *h_std_err);

/* ---- Worst-of autocallable notes under per-asset local-volatility surfaces, dividend yields q_j ----
 * Additive to ABI version 5: first carried by the build that ships csrc/autocall_localvol.hip (no struct of an earlier
 * call changed, so MCAMD_ABI_VERSION stays 5; a caller finds out with dlsym).  The note of mcamd_price_autocall, stepped
 * on d = autocall->n_assets correlated assets, asset j under surfaces[j] and the dividend yield q[j].  One normal per
 * asset per step from the stream mcamd_price_basket draws from; nothing else is drawn.  opt supplies r and T only:
 * opt->S0, opt->v, opt->K and opt->B are ignored.  n = n_steps, dt = T / n.  All path arithmetic is in the path
 * precision and in NATURAL-log units.
 *   Surfaces.  surfaces: a host array of d surface pointers (read before the call returns).  Asset j's surface is in
 *       x = ln(S_j / S_j,0), the asset's own log-performance.  The same surface may be passed for several assets (its
 *       nodes then count once per asset).  The lookup sigma_j(row, X), the slice rule row_j(i) = floor(i n_t,j / n), the
 *       clamp, and the narrowing of sigma_k, slope_k, x_min and 1 / dx are exactly those of mcamd_price_localvol, asset by
 *       asset, each with its own grid.
 *   Normals.  z_{i,k}, i = 0..n-1, k = 0..d-1, is normal number i d + k of the path's stream: Philox subsequence = the
 *       GLOBAL path id, block (i d + k) / NB, slot (i d + k) % NB, NB = 4 in fp32 and 2 in fp64 — mcamd_price_basket's
 *       layout.  The lower Cholesky factor l of corr[:d, :d] is the one mcamd_price_basket forms (same pivot rule),
 *       narrowed once to the path precision.  w_j = sum_{k <= j} l_jk z_{i,k}, evaluated as a chain of fused
 *       multiply-adds in ascending k starting from 0:  w <- fma(l_jk, z_{i,k}, w).  At j = 0 (l_00 = 1) this is z_{i,0}
 *       exactly.
 *   Step.  X_{j,0} = 0.  s_j = sigma_j(row_j(i), X_{j,i}), then
 *       X_{j,i+1} = X_{j,i} + fma(s_j sqrt(dt), w_j, fma(-s_j^2, dt / 2, (r - q_j) dt)),
 *       with (r - q_j) dt, dt / 2 and sqrt(dt) formed in double on the host and narrowed: the operation order of
 *       mcamd_price_localvol's step with z replaced by w_j, so d = 1 walks that call's path bit for bit.
 *       l_i = min_j X_{j,i}, the log of the worst performance after step i.
 *   Dates, levels and payments.  The observation dates q = 1..M at the ends of steps s_q = q observe_every, the levels
 *       L_q, the payments pay_q (doubles), the call test "first date q >= first_call_date with l_{s_q} >= ln L_q", the
 *       knock-in modes MCAMD_AUTOCALL_KI_*, the rule that at date M the call test comes first, the sample of a path never
 *       called (y = min(A_n, 1) if knocked in, 1 otherwise) and the two step counters are exactly those of
 *       mcamd_price_autocall — but ln L_q and ln ki_level are narrowed once to the path precision in NATURAL-log units,
 *       where that call narrows them in exponent units.  A_n = e^{l_n} through the exponential that ends a log-space
 *       path, exp_of_logreturn(1, l_n exp_scale) with exp_scale = log2 e (fp32) or 65536 / ln 2 (fp64) narrowed to the
 *       path precision, formed once per path and widened to fp64.
 *   price = exp(-rT) mean(y): mcamd_finalize and mcamd_finalize_stats serve unchanged.
 * Flat surfaces with q = 0 give the call dates and, up to rounding, the samples of mcamd_price_autocall at v_j = sigma_j.
 * A wavefront whose lanes have all been called leaves the step loop at the end of its step group, as there.  Two runs of
 * one job give the same bits.
 * d_samples, res (mcamd_autocall_result) and the enqueue form's d_stats = {sum, sumsq, n_called, sum_t_call,
 * n_knocked_in, n}: as mcamd_price_autocall; mcamd_enqueued_kernel_ms covers the enqueue form.
 * Requirements (MCAMD_ERR_INVALID before any device work).  First, in this order, everything that needs neither a
 * surface nor the context: opt, sim, autocall, res non-NULL; reserved[0] == reserved[1] == 0; what mcamd_price_basket
 * refuses of n_assets and corr, with the same Cholesky pivot rule; q[j] finite for j < d; observe_every >= 1,
 * n_steps % observe_every == 0 and 1 <= M <= MCAMD_AUTOCALL_MAX_DATES; 1 <= first_call_date <= M; the terms as
 * mcamd_price_autocall checks them (ki_monitoring, coupon, call_level, call_step_down, L_M > 0, ki_level); r finite;
 * use_window, P1, P2, Ik, Sk, Tk and opt->dt all 0; sim->flags 0 or MCAMD_FLAG_LOG_SPACE; what mcamd_price_paths refuses
 * on sim (its fp64 exponent-range bound at the drift r - q_j alone, asset by asset).  Then the surfaces: a NULL array or
 * entry; a surface created on another context; sum_j n_t,j n_x,j > MCAMD_LOCALVOL_MAX_NODES (the d pair tables share the
 * kernel's LDS); in fp64 the exponent-range bound of mcamd_price_localvol, asset by asset, at |r - q_j| and the largest
 * entry of surfaces[j].  Then the context.  q and corr beyond n_assets are ignored.  An empty shard returns zeros and
 * launches nothing; its enqueue form writes a zero record in stream order.
 * Out of scope: Greeks, continuous knock-in, lane compaction of the called paths, calibration of the surfaces, a
 * mcamd_group_* form and a shim name (the reference has no such product).  Multi-GPU: every rank prices its shard with
 * surfaces of its own context; the 6-double records add.  New. */
typedef struct mcamd_autocall_localvol {   /* 632 bytes: mcamd_autocall with q[] in the place of v[] */
    int32_t n_assets;         /* d, 1..MCAMD_BASKET_MAX_ASSETS */
    int32_t ki_monitoring;    /* MCAMD_AUTOCALL_KI_* */
    uint32_t observe_every;   /* steps between observation dates; divides n_steps */
    uint32_t first_call_date; /* 1..M: the first date the note can be called at */
    int32_t reserved[2];      /* must be 0 */
    double call_level;        /* L_1, as a performance (1 = the spots) */
    double call_step_down;    /* L_q = call_level - (q - 1) call_step_down */
    double coupon;            /* per date, snowball: a path called at date q receives 1 + q coupon */
    double ki_level;          /* as a performance, in (0, 1] and below L_M */
    double q[8];              /* continuous dividend yields */
    double corr[64];          /* correlations, row-major with stride 8 */
} mcamd_autocall_localvol;

int mcamd_price_autocall_localvol(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                  const mcamd_autocall_localvol *autocall, const mcamd_localvol_surface *const *surfaces,
                                  void *d_samples, mcamd_autocall_result *res);
int mcamd_price_autocall_localvol_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                          const mcamd_autocall_localvol *autocall,
                                          const mcamd_localvol_surface *const *surfaces, void *d_samples, double *d_stats);

/* ---- Local-volatility Greeks: price, delta, gamma, vega, bucketed vega, rho and dividend rho from ONE walk ----
 * Additive to ABI version 5: first carried by the build that ships csrc/localvol_greeks.hip (no struct of an earlier
 * call changed, so MCAMD_ABI_VERSION stays 5; a caller finds out with dlsym).  The pathwise derivative of the log-Euler
 * path is a first-order tangent recurrence, driven by the normal and the table entry the step loads anyway.
 *   Paths.  Those of mcamd_price_localvol with MCAMD_LOCALVOL_NO_BARRIER, draw for draw and operation for operation:
 *       X_0 = 0, the same lookup, row rule, step and Philox subsequence (the GLOBAL path id).  opt->v is ignored.
 *   Lookup and slope at step i = 0 .. n - 1 (n = n_steps):  k, f and s = fma(f, slope_k, sigma_k) exactly as there;
 *       u_raw = (X_i - x_min) (1 / dx) is the value before the clamp;
 *       s' = slope_k (1 / dx)  if 0 < u_raw < n_x - 1, strictly;  s' = 0 otherwise (a NaN gives 0).
 *       The surface is flat outside its range, so a clamped path has no slope.
 *   Tangents, in the path precision, with one factor per step:
 *       c_i = sqrt(dt) z_{i+1} - s dt          (two products and their difference: three roundings; dt = T / n narrowed)
 *       g_i = fma(s', c_i, 1)
 *       J_{i+1} = J_i g_i,            J_0 = 1   tangent to X_0: the spot moves, the surface stays where it is in
 *                                               absolute price
 *       U_{i+1} = fma(U_i, g_i, c_i), U_0 = 0   tangent to sigma -> sigma + theta at every node
 *       R_{i+1} = fma(R_i, g_i, dt),  R_0 = 0   tangent to r; the tangent to q is -R
 *       U^b: sigma -> sigma + theta on the steps of time bucket b only, bucket(i) = floor(i B / n) in 64-bit integers
 *            (the rule the rows use), B = n_vega_buckets in 0 .. 8; B need not divide n and may exceed it:
 *            U^b_{i+1} = fma(U^b_i, g_i, c_i) if bucket(i) = b,  U^b_i g_i otherwise,  U^b_0 = 0.
 *            A bucket that is empty or has not started is exactly 0.
 *       Every fused operation is written as fma above; every other product, sum and difference is one operation.
 *   Samples, formed once per path in fp64 (each product, quotient and difference one fp64 operation, left to right):
 *       y = h(S_T) as mcamd_price_localvol forms it; omega = +1 (call) or -1 (put); I = 1{omega (S_T - K) > 0} (= h > 0
 *       in the path precision); m = omega I S_T.
 *       price y;  delta m J_n / S0;  vega m U_n;  bucket b: m U^b_n;  rho m R_n - T y;  rho_q -(m R_n).
 *   Gamma.  The piecewise-linear surface has a slope that jumps at the nodes, and S0 often sits on a node, so a second
 *       pathwise derivative does not exist.  Gamma is a central common-random-number difference of the pathwise delta:
 *       with eta = gamma_bump, two more walks start at X_0 = +eta and X_0 = -eta (narrowed to the path precision) on the
 *       same normals, each with its own lookups and its own J.  With S^+- = S0 e^{+-eta} (fp64), S_T^+- = S0 e^{X_n^+-},
 *       delta^+- = m^+- J_n^+- / S^+-, the sample is (delta^+ - delta^-) / (S^+ - S^-).  eta = 0 skips the two walks:
 *       gamma's value and std_err are then NaN and its sums 0.
 *   On a node.  When X_0 lies exactly on a node, which cell floor(u) picks at step 0 depends on the rounding of 1 / dx in
 *       the path precision.  Only J_1, hence delta and gamma, sees that (U_1 = c_0 and R_1 = dt do not): delta is then a
 *       one-sided derivative, and the two path precisions may take different sides.
 *   value = e^{-rT} mean, std_err as mcamd_finalize computes it.  Vega and the buckets are per unit of volatility, rho
 *   and rho_q per unit of rate.  Theta is not offered: with the time slices tied to T its convention is ambiguous.
 *   Statistics record (32 doubles): [0..12) the (sum, sumsq) pairs of price, delta, gamma, vega, rho, rho_q;
 *   [12..28) the pairs of the eight buckets, unused ones exact zeros; [28] = n; [29..32) = 0.  Shards add element by
 *   element; mcamd_finalize_localvol_greeks_stats serves the total (gamma_defined = 0 reports gamma as NaN with zero
 *   sums; buckets from n_vega_buckets on stay 0).  The enqueue form leaves the record in d_stats (device, >= 32 doubles;
 *   it reads NaN until the kernel has written it); mcamd_enqueued_kernel_ms covers it.  One launch, one fixed order of
 *   summation: two runs of one job give the same bits.
 *   d_samples (nullable, device): ALWAYS double, estimator-major, (6 + n_vega_buckets) x n_paths_local values:
 *   [e * n_paths_local + local path] receives sample e (MCAMD_LOCALVOL_GREEK_* order, then the buckets; the gamma row
 *   is 0 when eta = 0).
 * Requirements (MCAMD_ERR_INVALID before any device work; first everything that needs neither the surface nor the
 * context, then the surface, then the context): everything mcamd_price_localvol refuses for a barrier-less job; payoff in
 * range; n_vega_buckets <= MCAMD_LOCALVOL_GREEKS_MAX_BUCKETS; gamma_bump finite and in [0, 0.1]; the fp64 exponent-
 * range bound taken with |eta| added to the path's log-return range.  An empty shard returns zeros and launches nothing.
 * There is no mcamd_group_* form, no shim name and no barrier; per-node vega and Greeks of the smile and of the
 * autocallable are not offered.  New. */
#define MCAMD_LOCALVOL_GREEKS_MAX_BUCKETS 8

#define MCAMD_LOCALVOL_GREEK_PRICE 0
#define MCAMD_LOCALVOL_GREEK_DELTA 1
#define MCAMD_LOCALVOL_GREEK_GAMMA 2
#define MCAMD_LOCALVOL_GREEK_VEGA  3
#define MCAMD_LOCALVOL_GREEK_RHO   4
#define MCAMD_LOCALVOL_GREEK_RHO_Q 5

typedef struct mcamd_localvol_greeks_job {   /* 24 bytes */
    int32_t  payoff;           /* MCAMD_PAYOFF_* */
    uint32_t n_vega_buckets;   /* 0 .. MCAMD_LOCALVOL_GREEKS_MAX_BUCKETS */
    double   q;                /* continuous dividend yield */
    double   gamma_bump;       /* eta in ln(S) units, 0 .. 0.1; 0: no gamma */
} mcamd_localvol_greeks_job;

typedef struct mcamd_localvol_greeks {       /* 472 bytes */
    double value[6];           /* D * mean, indexed MCAMD_LOCALVOL_GREEK_*; gamma NaN when gamma_bump = 0 */
    double std_err[6];         /* D * sqrt(s^2 / n) */
    double bucket_value[8];    /* bucketed vega; buckets from n_vega_buckets on are 0 */
    double bucket_std_err[8];
    double sum[6];             /* the shard's raw fp64 sums of the undiscounted samples */
    double sumsq[6];
    double bucket_sum[8];
    double bucket_sumsq[8];
    uint64_t n;                /* paths */
    float kernel_ms;           /* HIP-event time of the kernel (it finishes its own sum: the whole call's device work) */
    float total_ms;
    uint32_t grid;             /* launch shape the engine chose */
    uint32_t block;
} mcamd_localvol_greeks;

int mcamd_price_localvol_greeks(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                const mcamd_localvol_greeks_job *job, const mcamd_localvol_surface *surface,
                                double *d_samples, mcamd_localvol_greeks *out);
int mcamd_price_localvol_greeks_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                        const mcamd_localvol_greeks_job *job, const mcamd_localvol_surface *surface,
                                        double *d_samples, double *d_stats);
int mcamd_finalize_localvol_greeks_stats(const double stats[32], double r, double T, uint32_t n_vega_buckets,
                                         int gamma_defined, mcamd_localvol_greeks *out);

/* ---- Cliquets, forward-start options and realized-variance swaps under a local-volatility surface ----
 * Additive to ABI version 5: first carried by the build that ships csrc/cliquet.hip (no struct of an earlier call
 * changed, so MCAMD_ABI_VERSION stays 5; a caller finds out with dlsym).  Payoffs built from the returns between reset
 * dates, where every other surface call reads the path at maturity or against a level fixed today: what they are worth
 * rests on the forward smile, which a local-volatility surface flattens.
 *   Paths.  Those of mcamd_price_localvol with MCAMD_LOCALVOL_NO_BARRIER, draw for draw and operation for operation:
 *       X_0 = 0, the same surface object, lookup, row rule, step and Philox subsequence (the GLOBAL path id), one normal
 *       per step and nothing else drawn.  r, T and S0 come from opt; the notional is 1, so S0 only says which spot the
 *       surface's axis x = ln(S / S0) is measured from and no arithmetic reads it.  opt->v, opt->K and opt->B are
 *       ignored.  q = cliquet->q is the dividend yield, n = n_steps, dt = T / n.
 *   Reset dates.  p = 1..M at the ends of steps s_p = p reset_every, M = n / reset_every, s_0 = 0; tau = reset_every dt.
 *       The period log-return is D_p = X_{s_p} - X_{s_{p-1}}, one subtraction in the path precision.  Periods
 *       p < first_period are walked but do not count (the forward-start forms); P = M - first_period + 1 periods count.
 *   MCAMD_CLIQUET_SUM (additive cliquet).  R_p = e^{D_p} - 1 through the exponential that ends a log-space path with
 *       multiplier 1, exp_of_logreturn(1, D_p exp_scale) with exp_scale = log2 e (fp32) or 65536 / ln 2 (fp64) narrowed
 *       to the path precision, then minus 1;  c_p = min(max(R_p, local_floor), local_cap), the bounds narrowed once;
 *       A = sum_{p >= first_period} c_p, added in date order in the path precision.
 *   MCAMD_CLIQUET_COMPOUND (compounding ratchet).  l_p = min(max(D_p, ln(1 + local_floor)), ln(1 + local_cap)), the two
 *       logarithms formed in double on the host (log(1.0 + bound): ln 0 = -inf and ln inf = +inf are legitimate
 *       operands) and narrowed once;  L = sum_{p >= first_period} l_p in date order in the path precision;
 *       A = e^L - 1: ONE exponential per path, exp_of_logreturn(1, L exp_scale) in the path precision, widened, and the
 *       subtraction in fp64.  No exponential is taken before maturity.
 *   MCAMD_CLIQUET_VARIANCE (realized variance, annualised).  V = sum_{p >= first_period} D_p^2 in date order, as
 *       V <- fma(D_p, D_p, V) in the path precision;  A = V (1 / (P tau)), the factor formed in double on the host as
 *       1.0 / (P * (reset_every * dt)) and the product taken in fp64.  No exponential at all.
 *   Sample, formed once per path in fp64:  y = min(max(A, global_floor), global_cap); an infinite bound never binds.
 *       price = exp(-rT) mean(y), std_err as in mcamd_finalize.  A forward-start call struck at k times the spot of
 *       the date t_1 the last period starts at is caller arithmetic on the SUM form with first_period = M,
 *       local_floor = k - 1 and no other bound:  (S_T / S_{t_1} - k)+ = y - (k - 1).
 *   Counters.  n_floored = paths with A <= global_floor, n_capped = paths with A >= global_cap, the comparisons in
 *       fp64 on the value that is clipped; 0 for an infinite bound.
 * A is kept in the path precision because it is path arithmetic (it is what an fp32 job is asked to do cheaply); y is
 * formed in fp64 so that the clip, the counters and the sums see one value whatever the path precision.
 * d_samples (nullable, device): n_paths_local values of the path precision; [local path] receives y.
 * res: price .. n as mcamd_result; work_steps = 64 x the steps each wavefront ran, always the full count (there is no
 * early exit).  The enqueue form leaves {sum, sumsq, n_floored, n_capped, 0, n} in d_stats: mcamd_finalize_stats serves
 * it and mcamd_enqueued_kernel_ms covers it.  A sample depends on its global path id alone, so one all-reduce of the 6
 * doubles serves multi-GPU use.  One launch, one fixed order of summation: two runs of one job give the same bits.
 * Requirements (MCAMD_ERR_INVALID before any device work).  First everything that does not need the surface: opt, sim,
 * cliquet, res non-NULL; kind in range; reserved == 0; reset_every >= 1 and n_steps % reset_every == 0;
 * 1 <= first_period <= M; no bound NaN; local_floor < local_cap and global_floor < global_cap; COMPOUND:
 * local_floor >= -1 and local_cap > -1; VARIANCE: local_floor == -inf and local_cap == +inf (they have no meaning
 * there); q finite; r finite; use_window, P1, P2, Ik, Sk, Tk and opt->dt all 0; sim->flags 0 or MCAMD_FLAG_LOG_SPACE;
 * what mcamd_price_paths refuses on sim (its fp64 exponent-range bound at the drift r - q alone).  Then the surface: NULL;
 * in fp64 the exponent-range bound of mcamd_price_localvol at |r - q| and the surface's largest entry.  Then the
 * context, and a surface created on another context.  An empty shard returns zeros and launches nothing; its enqueue
 * form writes a zero record in stream order.
 * Out of scope: an early exit once a floored sum has passed the global cap, Greeks, reverse cliquets, Napoleons and
 * memory coupons, several assets, non-uniform reset schedules, corridor, gamma and volatility (square-root) swaps, a
 * mcamd_group_* form and a shim name (the reference has no such product).  New. */
#define MCAMD_CLIQUET_SUM 0
#define MCAMD_CLIQUET_COMPOUND 1
#define MCAMD_CLIQUET_VARIANCE 2

typedef struct mcamd_cliquet {   /* 56 bytes */
    int32_t kind;            /* MCAMD_CLIQUET_* */
    uint32_t reset_every;    /* steps per period; divides n_steps */
    uint32_t first_period;   /* 1..M: the first period that counts */
    int32_t reserved;        /* must be 0 */
    double local_floor;      /* of the period return R_p (-inf: none); VARIANCE: must be -inf */
    double local_cap;        /* of the period return R_p (+inf: none); VARIANCE: must be +inf */
    double global_floor;     /* of A (-inf: none) */
    double global_cap;       /* of A (+inf: none) */
    double q;                /* continuous dividend yield */
} mcamd_cliquet;

typedef struct mcamd_cliquet_result {   /* 96 bytes */
    double price;            /* exp(-rT) * mean(y) */
    double std_err;
    double ci_lo, ci_hi;     /* 95 % confidence interval */
    double sum, sumsq;       /* the shard's raw fp64 sums of the undiscounted samples */
    uint64_t n;              /* paths */
    uint64_t n_floored;      /* paths with A <= global_floor (0 without one) */
    uint64_t n_capped;       /* paths with A >= global_cap (0 without one) */
    double work_steps;       /* 64 x the steps each wavefront ran: always the full count */
    float kernel_ms;         /* HIP-event time of the kernel (it finishes its own sum: the whole call's device work) */
    float total_ms;
    uint32_t grid;           /* launch shape the engine chose */
    uint32_t block;
} mcamd_cliquet_result;

int mcamd_price_cliquet(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_cliquet *cliquet,
                        const mcamd_localvol_surface *surface, void *d_samples, mcamd_cliquet_result *res);
int mcamd_price_cliquet_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                const mcamd_cliquet *cliquet, const mcamd_localvol_surface *surface, void *d_samples,
                                double *d_stats);
/* Host closed form, exact when the volatility varies in time only: there D_p ~ N((r - q - v_p^2 / 2) tau, v_p^2 tau),
 * independently across periods, at every step count (the log-Euler walk is exact there).  tau = T / n_periods;
 * period_vol[p - 1] = v_p, the rms volatility of period p; there is no global clip.
 *   c_p(k) = E[(e^{D_p} - k)+] = e^{(r-q) tau} N(d1) - k N(d2),  d1 = ((r - q + v_p^2 / 2) tau - ln k) / (v_p sqrt tau),
 *       d2 = d1 - v_p sqrt tau;  for k <= 0 it is e^{(r-q) tau} - k, for k = +inf it is 0.  N: the erfc form of
 *       mcamd_bs_call_f64.
 *   F = max(local_floor, -1) (a floor at or below -1 never binds);  E_p = (1 + F) + c_p(1 + F) - c_p(1 + local_cap),
 *       the mean of the clipped gross return.
 *   SUM: e^{-rT} sum_{p >= first_period} (E_p - 1).   COMPOUND: e^{-rT} (prod_{p >= first_period} E_p - 1).
 *   VARIANCE: e^{-rT} (1 / (P tau)) sum_{p >= first_period} [v_p^2 tau + ((r - q - v_p^2 / 2) tau)^2].
 * Refuses a NULL pointer, kind out of range, T <= 0, non-finite T, r or q, n_periods == 0, first_period outside
 * 1..n_periods, a volatility that is not finite and > 0, and what mcamd_price_cliquet refuses of the local bounds. */
int mcamd_cliquet_price_f64(int kind, double T, double r, double q, uint32_t n_periods, uint32_t first_period,
                            const double *period_vol, double local_floor, double local_cap, double *price);

/* ---- European options under Heston stochastic volatility ----
 * Additive to ABI version 5: first carried by the build that ships csrc/heston.hip (no struct of an earlier call
 * changed, so MCAMD_ABI_VERSION stays 5; a caller finds out with dlsym).  The one model here whose volatility has a
 * random driver of its own: it keeps the forward smile that a local-volatility surface flattens.
 *   Model.  dS / S = (r - q) dt + sqrt(v) dW1,  dv = kappa (theta - v) dt + xi sqrt(v) dW2,  d<W1, W2> = rho dt.
 *   Scheme.  MCAMD_HESTON_FULL_TRUNCATION: the full-truncation Euler scheme in the log-price (Lord, Koekkoek, van Dijk
 *       2010).  The raw variance v may go below zero; the drift, the diffusion and the mean reversion read
 *       v+ = max(v, 0).  The step map is continuous in every input (max, sqrt and fused multiply-adds: no branch on a
 *       moment ratio, no inverse distribution function), so two precisions of one path never take different formulas.
 *       The scheme is weakly first order in dt.  scheme is a field so that another one can arrive without an ABI change.
 *   Per path.  X_0 = 0 (X = ln(S / S0) in natural units), v_0 = v0, n = n_steps, dt = T / n.  r, T, S0 and K come from
 *       opt, the rest from the job; opt->v and opt->B are ignored.
 *   Draws.  z = normal i of Philox blocks 0, 1, .. of the path's subsequence (the GLOBAL path id): exactly the normal
 *       mcamd_price_barrier and mcamd_price_localvol draw for step i (4 per block in fp32, 2 per block in fp64, whole
 *       blocks, the remainder block as there).  z' = normal i of blocks 2^63, 2^63 + 1, .. of the same key and
 *       subsequence, by the same Box-Muller: where mcamd_price_lookback keeps its step uniforms.  Nothing else is drawn.
 *   Per step i = 0 .. n - 1, in one precision (the path precision) throughout:
 *       v+ = max(v_i, 0),  s = sqrt(v+)            fp32: the hardware square root (1 ulp); fp64: correctly rounded
 *       w  = fma(rho, z, sqrt(1 - rho^2) z')        sqrt(1 - rho^2) formed in double on the host and narrowed once:
 *                                                   0 at rho = +-1, where w = rho z exactly
 *       X_{i+1} = X_i + fma(s sqrt(dt), z, fma(-v+, dt / 2, (r - q) dt))
 *       v_{i+1} = v_i + fma(s (xi sqrt(dt)), w, fma(-v+, kappa dt, kappa theta dt))
 *       These are the contractions the kernels use, written as explicit fused operations (the X line is
 *       mcamd_price_localvol's move with s^2 replaced by v+).  The constants (r - q) dt, dt / 2, sqrt(dt), kappa dt,
 *       kappa theta dt, xi sqrt(dt), rho and sqrt(1 - rho^2) are formed in double on the host and narrowed once.
 *       xi = 0 (v deterministic), kappa = 0 and rho = +-1 are legal.  With xi = 0 and kappa = 0 the path is that of
 *       mcamd_price_localvol on a flat surface at sqrt(v0), normal for normal.
 *   Per path, after the loop.  S_T = S0 e^{X_n} through the exponential that ends a local-volatility path;
 *       h = max(+-(S_T - K), 0) in the path precision;  y = h widened to double.
 *       trunc = the number of steps entered with v_i < 0 (a 32-bit counter);  rv = (1 / n) sum_i v+_i, the path's
 *       average variance, summed in the path precision in step order, the factor 1 / n applied in fp64.
 *   price = exp(-rT) mean(y), std_err as in mcamd_finalize.
 * d_samples (nullable, device): n_paths_local values of the path precision; [local path] receives y.
 * d_state (nullable, device): 2 n_paths_local values of the path precision; [local path] receives S_T and
 * [n_paths_local + local path] the raw v_n, which may be negative.
 * res: price .. n as mcamd_result; truncated_steps = sum of trunc over the shard (a double: it adds over shards);
 * mean_variance = mean of rv over the shard; work_steps = 64 x the steps each wavefront ran, always the full count
 * (there is no early exit).  The enqueue form leaves {sum, sumsq, truncated_steps, sum of rv, 0, n} in d_stats:
 * mcamd_finalize_stats serves it and mcamd_enqueued_kernel_ms covers it.  A sample depends on its global path id alone,
 * so shards add element by element and one all-reduce of the 6 doubles serves multi-GPU use.  One launch, one fixed
 * order of summation: two runs of one job give the same bits.
 * Requirements (MCAMD_ERR_INVALID before any device work, in this order): opt, sim, heston, res non-NULL; payoff and
 * scheme in range; reserved == 0; q, v0, kappa, theta, xi, rho finite; v0, kappa, theta, xi >= 0; |rho| <= 1; r finite;
 * use_window, P1, P2, Ik, Sk, Tk and opt->dt all 0; sim->flags 0 or MCAMD_FLAG_LOG_SPACE; what mcamd_price_paths refuses
 * on sim (its fp64 exponent-range bound at the drift r - q alone: the variance is random, and no bound on the request
 * covers it); S0 > 0 and K > 0; then the context.  An empty shard returns zeros and launches nothing; its enqueue form
 * writes a zero record in stream order.
 * Left out on purpose: the QE scheme and exact simulation, Asians and lookbacks, Greeks, a term structure of the
 * parameters, a mcamd_group_* form and a shim name (the reference has no such model).  The smile of the model is
 * mcamd_price_heston_smile, its cliquets mcamd_price_heston_cliquet and its single barriers
 * mcamd_price_heston_barrier, below.
 * New. */
#define MCAMD_HESTON_FULL_TRUNCATION 0

typedef struct mcamd_heston {   /* 64 bytes */
    int32_t payoff;          /* MCAMD_PAYOFF_* */
    int32_t scheme;          /* MCAMD_HESTON_FULL_TRUNCATION */
    double q;                /* continuous dividend yield */
    double v0;               /* the variance at t = 0, >= 0 */
    double kappa;            /* speed of mean reversion, >= 0 */
    double theta;            /* long-run variance, >= 0 */
    double xi;               /* volatility of the variance, >= 0 */
    double rho;              /* correlation of the two drivers, in [-1, 1] */
    double reserved;         /* must be 0 */
} mcamd_heston;

typedef struct mcamd_heston_result {   /* 96 bytes */
    double price;            /* exp(-rT) * mean(y) */
    double std_err;
    double ci_lo, ci_hi;     /* 95 % confidence interval */
    double sum, sumsq;       /* the shard's raw fp64 sums of the undiscounted samples */
    uint64_t n;              /* paths */
    double truncated_steps;  /* lane-steps entered with v < 0 */
    double mean_variance;    /* mean over the shard of the paths' average variance (1 / n_steps) sum v+ */
    double work_steps;       /* 64 x the steps each wavefront ran: always the full count */
    float kernel_ms;         /* HIP-event time of the kernel (it finishes its own sum: the whole call's device work) */
    float total_ms;
    uint32_t grid;           /* launch shape the engine chose */
    uint32_t block;
} mcamd_heston_result;

int mcamd_price_heston(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *heston,
                       void *d_samples, void *d_state, mcamd_heston_result *res);
int mcamd_price_heston_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *heston,
                               void *d_samples, void *d_state, double *d_stats);
/* ---- Heston smile: n_expiries x n_strikes vanillas priced on ONE set of Heston paths ----
 * Additive to ABI version 5: first carried by the build that ships csrc/heston_smile.hip (MCAMD_ABI_VERSION stays 5; a
 * caller finds out with dlsym).  mcamd_price_localvol_smile's shape on mcamd_price_heston's paths: the paths are walked
 * once and read at every expiry step, where 252 calls of mcamd_price_heston would walk nearly the same paths 252 times.
 *   Paths.  Those of mcamd_price_heston, draw for draw and operation for operation: X_0 = 0 and v_0 = v0, the same step
 *       in the path precision with dt = T / n_steps over the WHOLE n_steps, z from Philox blocks 0, 1, .. and z' from
 *       blocks 2^63, 2^63 + 1, .. of the path's subsequence (the GLOBAL path id).  Nothing else is drawn.  The walk ends
 *       after the last expiry step.  r, T and S0 come from opt, the model and q from heston; heston->payoff holds for
 *       every node; opt->K, opt->v and opt->B are ignored (and may hold anything).
 *   Expiries.  h_expiry_steps[m], m = 0 .. n_expiries - 1, strictly ascending with 1 <= s_m <= n_steps.  Expiry m is the
 *       time t_m = s_m (T / n_steps); its spot is S_m = S0 e^{X_{s_m}}, evaluated exactly as mcamd_price_heston evaluates
 *       S_T, in the path precision.  With s_m = n_steps, S_m and v_{s_m} are mcamd_price_heston's S_T and v_n, bit for
 *       bit.
 *   Nodes, h_stats, price and std_err: as mcamd_price_localvol_smile defines them.  Node (m, k) has the undiscounted
 *       sample h = max(+-(S_m - K_k), 0), formed in the path precision from K_k narrowed to it, then widened to double;
 *       h_stats is 2 n_expiries n_strikes doubles, the sums [m n_strikes + k] first, then the sums of squares, both
 *       accumulated in fp64; every node is discounted to its OWN expiry t_m.  mcamd_finalize_smile serves the sums: it
 *       reads only n_expiries and n_strikes of its mcamd_smile.
 *   res: as mcamd_price_localvol_smile fills it.  n, kernel_ms (the path kernel), total_ms (with the sum of the
 *       per-wavefront records), grid, block; work_steps = 64 x the steps each wavefront ran (s_last per wavefront that
 *       holds a path), live_steps = work_steps; sum, sumsq, price, std_err, ci_lo, ci_hi are those of the LAST node,
 *       finalized with t of the last expiry.  Everything else in res is zero.
 *   Diagnostics.  truncated_steps and mean_variance are NOT reported: a wavefront's record holds node sums only, and
 *       mcamd_price_heston on the same sim gives both for the same paths.
 *   d_state (nullable, device): 2 n_expiries x n_paths_local values of the path precision:
 *       [m n_paths_local + local path] receives S_m and [(n_expiries + m) n_paths_local + local path] the raw variance
 *       v_{s_m}, which may be negative.
 *   The enqueue form leaves the same 2 n_expiries n_strikes doubles in d_stats, followed by one more double that holds
 *   n (the shard's paths): d_stats has room for 2 n_expiries n_strikes + 1 doubles.  Shards add element by element.
 *   mcamd_enqueued_kernel_ms covers the path kernel.  h_expiry_steps and h_strikes are read before the call returns.
 *   Results do not depend on earlier calls, and two runs of one job give the same bits.
 * Requirements (MCAMD_ERR_INVALID before any device work, in this order): no NULL pointer (d_state apart); what
 * mcamd_price_heston refuses of payoff, scheme, reserved, the model's parameters and r; n_expiries in
 * 1 .. MCAMD_SMILE_MAX_EXPIRIES, n_strikes in 1 .. MCAMD_SMILE_MAX_STRIKES; expiry steps strictly ascending in
 * 1 .. n_steps; every strike finite and > 0; what mcamd_price_heston refuses of opt's other fields, sim->flags and sim;
 * S0 > 0; then the context.  An empty shard returns zeros and launches nothing; its enqueue form writes a zero record in
 * stream order.  There is no mcamd_group_* form and no shim name.  Barriers, mixed call / put nodes and Greeks are not
 * offered.  New. */
int mcamd_price_heston_smile(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *heston,
                             uint32_t n_expiries, uint32_t n_strikes, const uint32_t *h_expiry_steps,
                             const double *h_strikes, void *d_state, double *h_stats, mcamd_result *res);
int mcamd_price_heston_smile_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                     const mcamd_heston *heston, uint32_t n_expiries, uint32_t n_strikes,
                                     const uint32_t *h_expiry_steps, const double *h_strikes, void *d_state,
                                     double *d_stats);

/* ---- Cliquets, forward-start options and realized-variance swaps under Heston ----
 * Additive to ABI version 5: first carried by the build that ships csrc/heston_cliquet.hip (no struct of an earlier call
 * changed, so MCAMD_ABI_VERSION stays 5; a caller finds out with dlsym).  mcamd_price_cliquet's payoffs on the one model
 * here that keeps the forward smile they are worth.  Both job structs are the earlier calls', unchanged.
 *   Paths.  Those of mcamd_price_heston, draw for draw and operation for operation: X_0 = 0 and v_0 = v0, the same
 *       full-truncation step in the path precision with dt = T / n_steps, z from Philox blocks 0, 1, .. and z' from
 *       blocks 2^63, 2^63 + 1, .. of the path's subsequence (the GLOBAL path id).  Nothing else is drawn.  r, T and S0
 *       come from opt, the model, the scheme and q from heston; the notional is 1 and no arithmetic reads S0.  opt->v,
 *       opt->K and opt->B are ignored.  heston->payoff must be in range but is not read.  cliquet->q states the same
 *       dividend yield a second time and must equal heston->q bit for bit.
 *   Reset dates, kinds, sample, counters.  Those of mcamd_price_cliquet, operation for operation, with X the Heston
 *       log-price: dates p = 1..M at the ends of steps p reset_every, D_p = X_{s_p} - X_{s_{p-1}}, periods
 *       p >= first_period count; MCAMD_CLIQUET_SUM, _COMPOUND and _VARIANCE accumulate A as defined there, in the path
 *       precision; y = min(max(A, global_floor), global_cap) in fp64; n_floored and n_capped count A <= global_floor
 *       and A >= global_cap.  price = exp(-rT) mean(y), std_err as in mcamd_finalize.
 *   Caller arithmetic.  A forward-start call struck at k times the spot of the date the last period starts at is the SUM
 *       form with first_period = M, local_floor = k - 1 and no other bound: (S_T / S_{t_1} - k)+ = y - (k - 1).  A call
 *       on realized variance struck at K is the VARIANCE form with global_floor = K: max(A, K) = K + (A - K)+.
 *   Diagnostics.  trunc and rv per path as mcamd_price_heston defines them, over all n steps.
 * d_samples (nullable, device): n_paths_local values of the path precision; [local path] receives y.
 * res: price .. block as mcamd_cliquet_result, work_steps = 64 x the steps each wavefront ran (always the full count,
 * computed on the host); truncated_steps and mean_variance as mcamd_heston_result: on one job they are
 * mcamd_price_heston's.  The enqueue form leaves {sum, sumsq, n_floored, n_capped, sum of rv, n} in d_stats:
 * mcamd_finalize_stats serves it with control_variate = 0 and mcamd_enqueued_kernel_ms covers it; truncated_steps is
 * reported by the synchronous call only (the statistics layout keeps n where the kernel's record keeps it).  A sample
 * depends on its global path id alone, so shards add element by element.  One launch, one fixed order of summation:
 * two runs of one job give the same bits.
 * Requirements (MCAMD_ERR_INVALID before any device work, in this order).  opt, sim, heston, cliquet, res non-NULL.
 * Then everything mcamd_price_cliquet refuses before its surface: kind in range; cliquet->reserved == 0;
 * reset_every >= 1 and n_steps % reset_every == 0; 1 <= first_period <= M; no bound NaN; local_floor < local_cap and
 * global_floor < global_cap; COMPOUND: local_floor >= -1 and local_cap > -1; VARIANCE: local_floor == -inf and
 * local_cap == +inf; cliquet->q finite; r finite; use_window, P1, P2, Ik, Sk, Tk and opt->dt all 0; sim->flags 0 or
 * MCAMD_FLAG_LOG_SPACE; what mcamd_price_paths refuses on sim (its fp64 exponent-range bound at the drift r - q alone).
 * Then what mcamd_price_heston refuses of the model: payoff and scheme in range; heston->reserved == 0; q, v0, kappa,
 * theta, xi, rho finite; v0, kappa, theta, xi >= 0; |rho| <= 1; then cliquet->q != heston->q; with equal yields
 * mcamd_price_heston's refusals of sim are those already made, and S0 and K are not looked at.  Then the context.  An
 * empty shard returns zeros and launches nothing; its enqueue form writes a zero record in stream order.
 * Out of scope: the QE scheme, Asians under Heston (single barriers are mcamd_price_heston_barrier, below), Greeks,
 * volatility (square-root) swaps, non-uniform reset schedules, a mcamd_group_* form and a shim name (the reference has no
 * such product).  New. */
typedef struct mcamd_heston_cliquet_result {   /* 112 bytes */
    double price;            /* exp(-rT) * mean(y) */
    double std_err;
    double ci_lo, ci_hi;     /* 95 % confidence interval */
    double sum, sumsq;       /* the shard's raw fp64 sums of the undiscounted samples */
    uint64_t n;              /* paths */
    uint64_t n_floored;      /* paths with A <= global_floor (0 without one) */
    uint64_t n_capped;       /* paths with A >= global_cap (0 without one) */
    double work_steps;       /* 64 x the steps each wavefront ran: always the full count */
    float kernel_ms;         /* HIP-event time of the kernel (it finishes its own sum: the whole call's device work) */
    float total_ms;
    uint32_t grid;           /* launch shape the engine chose */
    uint32_t block;
    double truncated_steps;  /* lane-steps entered with v < 0 */
    double mean_variance;    /* mean over the shard of the paths' average variance (1 / n_steps) sum v+ */
} mcamd_heston_cliquet_result;

int mcamd_price_heston_cliquet(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *heston,
                               const mcamd_cliquet *cliquet, void *d_samples, mcamd_heston_cliquet_result *res);
int mcamd_price_heston_cliquet_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                       const mcamd_heston *heston, const mcamd_cliquet *cliquet, void *d_samples,
                                       double *d_stats);

/* ---- Single-barrier options under Heston: down / up, knock-out / knock-in, call / put, discrete or continuous ----
 * Additive to ABI version 5: first carried by the build that ships csrc/heston_barrier.hip (no struct of an earlier call
 * changed, so MCAMD_ABI_VERSION stays 5; a caller finds out with dlsym).  mcamd_price_barrier's product on
 * mcamd_price_heston's paths: the volatility moves with and after the spot's approach to the level, which a calibrated
 * local-volatility surface cannot say.  Both job structs are the earlier calls', unchanged.
 *   Inputs.  r, T, S0, K and the level B come from opt; opt->v is ignored.  The model, the scheme and q come from
 *       heston, the kind and the monitoring from barrier.  barrier->payoff is the payoff; heston->payoff states it a
 *       second time and must be equal.
 *   Paths.  Those of mcamd_price_heston, draw for draw and operation for operation: X_0 = 0 and v_0 = v0, the same
 *       full-truncation step in the path precision with dt = T / n_steps, z from Philox blocks 0, 1, .. and z' from
 *       blocks 2^63, 2^63 + 1, .. of the path's subsequence (the GLOBAL path id).  Nothing else is drawn.  v+_i is the
 *       variance step i was taken at, max(v_{i-1}, 0), i = 1..n.
 *   Barrier.  b = ln(B / S0), formed in double on the host and narrowed once.  The tests and distances are those of
 *       mcamd_price_barrier in the path precision: hit at step end i iff b > X_i (down) or X_i > b (up), strictly;
 *       d_i = X_i - b (down) or b - X_i (up), d_0 = |b|; a path is alive while no step end has hit.
 *   Survival weight w.
 *       MCAMD_MONITOR_DISCRETE    w = 1 on a path that is alive at the end, 0 once hit.
 *       MCAMD_MONITOR_CONTINUOUS  w = prod_i f_i on such a path, 0 once hit;  q_i = 2 d_{i-1} d_i / (v+_i dt);
 *           f_i = 1 - exp(-q_i) where the path is alive after step i and q_i < Q, Q = 38 (fp64) / 18 (fp32) in
 *           natural-log units, and f_i is DEFINED as exactly 1 elsewhere.  The test is made without a division, in the
 *           path precision: the factor is taken iff kq d_{i-1} d_i < q_cut v+_i, with kq = 2 / dt and q_cut = Q (fp32:
 *           both divided by ln 2 on the host, the factor being 1 - 2^{-q}); then q_i = (kq d_{i-1} d_i) / v+_i.  So a
 *           step taken at v+_i = 0 has f_i = 1 by definition, and rightly: it moves along a straight line, and the test
 *           at its end decides.  The rule is part of the definition: a restatement skips the factors the kernel skips.
 *       Why this weight.  The scheme freezes v+ over a step, so the bridge between two step ends is a Brownian bridge of
 *       variance rate v+_i and f_i is its exact probability of staying on the live side.  The continuous sample is
 *       therefore unbiased for the continuously monitored barrier OF THE SCHEME'S frozen-variance interpolation at
 *       every n_steps (n_steps = 1 included); against the model it carries the scheme's O(dt) weak error, like every
 *       price under MCAMD_HESTON_FULL_TRUNCATION.  The discrete sample prices the barrier monitored at the n step ends.
 *   Sample, in fp64 from the path-precision w and h, as mcamd_price_localvol forms it:  S_T = S0 e^{X_n} through the
 *       exponential that ends a mcamd_price_heston path, h = max(+-(S_T - K), 0);  knock-out  y = w h(S_T), and 0 for a
 *       path that was hit, whatever its unfinished price is;  knock-in  y = (1 - w) h(S_T).  No rebate.
 *   price = exp(-rT) mean(y), std_err as in mcamd_finalize.
 *   Early exit.  A knock-out wavefront leaves the walk at the first Philox-block end at which every one of its lanes is
 *       knocked; a knock-in runs to maturity (it needs S_T).
 *   Diagnostics.  The steps of a path that COUNT are all n for a knock-in and, for a knock-out, the steps it entered not
 *       yet hit.  live = the steps entered not yet hit (both kinds); trunc = the counted steps entered with v < 0;
 *       vs = sum of v+ over the counted steps, in the path precision in step order.  All depend on the path's global id
 *       alone (not on where its wavefront stopped), so shards add.
 * d_samples (nullable, device): n_paths_local values of the path precision; [local path] receives y.
 * d_state (nullable, device): 3 n_paths_local values of the path precision; [local path] receives S_T,
 * [n_paths_local + local path] the raw v_n and [2 n_paths_local + local path] w.  A knock-out path that was hit gets a
 * quiet NaN for S_T and v_n and w = 0: its walk may stop early, and where depends on its wavefront's other lanes, so no
 * value is defined there.
 * res: price .. n as mcamd_result; live_steps = sum of live; work_steps = 64 x the steps each wavefront ran;
 * truncated_steps = sum of trunc; mean_variance = sum of vs / the counted lane-steps (n_paths_local n_steps for a
 * knock-in, live_steps for a knock-out), formed on the host.  For a knock-in truncated_steps is mcamd_price_heston's
 * exactly and mean_variance its value up to rounding.  The block record is {sum, sumsq, live, trunc, vs, wave-steps};
 * the enqueue form leaves {sum, sumsq, live_steps, truncated_steps, sum of vs, n} in d_stats (device, >= 6 doubles):
 * mcamd_finalize_stats serves it and mcamd_enqueued_kernel_ms covers it; work_steps is reported by the synchronous call
 * only.  One launch, one fixed order of summation: two runs of one job give the same bits.
 * Requirements (MCAMD_ERR_INVALID before any device work, in this order).  opt, sim, heston, barrier, res non-NULL.
 * Then what mcamd_price_barrier refuses of the barrier: monitoring in range; barrier->reserved == 0; kind and
 * barrier->payoff in range; B > 0 and finite; S0 strictly on the live side (down: S0 > B, up: 0 < S0 < B).  Then what
 * mcamd_price_heston refuses: heston->payoff and scheme in range; heston->reserved == 0; q, v0, kappa, theta, xi, rho
 * finite; v0, kappa, theta, xi >= 0; |rho| <= 1; r finite; use_window, P1, P2, Ik, Sk, Tk and opt->dt all 0; sim->flags
 * 0 or MCAMD_FLAG_LOG_SPACE; what mcamd_price_paths refuses on sim (its fp64 exponent-range bound at the drift r - q
 * alone); S0 > 0 and K > 0.  Then heston->payoff != barrier->payoff.  Then the context.  An empty shard returns zeros
 * and launches nothing; its enqueue form writes a zero record in stream order.
 * Left out on purpose: rebates; double barriers; lane compaction of knocked paths (live_steps / work_steps is what it
 * would start from); the QE scheme; Asians and lookbacks under Heston; Greeks; a mcamd_group_* form and a shim name
 * (the reference has no such product); a closed form of the model's barrier price (none exists in general: with
 * rho = 0 and r = q the continuous sample's expectation given the variance path is mcamd_barrier_price_f64 at r = 0 and
 * v = sqrt(sum_i v+_i dt / T), at every n_steps, which tests/test_heston_barrier_cpu.py checks).  New. */
typedef struct mcamd_heston_barrier_result {   /* 104 bytes */
    double price;            /* exp(-rT) * mean(y) */
    double std_err;
    double ci_lo, ci_hi;     /* 95 % confidence interval */
    double sum, sumsq;       /* the shard's raw fp64 sums of the undiscounted samples */
    uint64_t n;              /* paths */
    double live_steps;       /* lane-steps entered not yet hit */
    double work_steps;       /* 64 x the steps each wavefront ran */
    double truncated_steps;  /* counted lane-steps entered with v < 0 */
    double mean_variance;    /* sum of v+ over the counted lane-steps / their number */
    float kernel_ms;         /* HIP-event time of the kernel (it finishes its own sum: the whole call's device work) */
    float total_ms;
    uint32_t grid;           /* launch shape the engine chose */
    uint32_t block;
} mcamd_heston_barrier_result;

int mcamd_price_heston_barrier(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *heston,
                               const mcamd_barrier *barrier, void *d_samples, void *d_state,
                               mcamd_heston_barrier_result *res);
int mcamd_price_heston_barrier_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                       const mcamd_heston *heston, const mcamd_barrier *barrier, void *d_samples,
                                       void *d_state, double *d_stats);

/* Host closed form of the model itself (not of the scheme, whose bias is first order in dt).  With F = S0 e^{(r-q)T},
 * D = e^{-rT}, k = ln(F / K) and phi the characteristic function of ln(S_T / F) in the branch-cut-safe form (Albrecher,
 * Mayer, Schoutens, Tistaert 2007, "the little Heston trap"), rearranged so that nothing is divided by xi^2:
 *   call = D (F - sqrt(F K) / pi  int_0^U Re[e^{iuk} phi(u - i/2)] / (u^2 + 1/4) du)   (Lewis 2000);  put by parity.
 * The rule: composite Gauss-Legendre, 16 nodes on each panel of width 1/2, over [0, U] with U the first of 32, 64, ..,
 * 4096 at which the envelope |phi(U - i/2)| / (U^2 + 1/4) is below 1e-15: 1024 nodes at U = 32, 131072 at most.
 * |phi(u - i/2)| <= E[e^{x/2}] <= 1, so whatever the parameters the dropped tail is at most D sqrt(F K) / (pi U); it
 * is that large only where the envelope has not fallen by U = 4096: a total variance near 0, or rho = +-1 (at
 * xi = 2 kappa rho the characteristic function does not decay at all).  Halving the panel or doubling U moves the
 * inputs of tests/test_heston_cpu.py by less than 1e-9 of S0, and an adaptive quadrature of the textbook form agrees
 * with them to 3e-13.
 * Below xi = MCAMD_HESTON_XI_MIN the variance is taken as deterministic: Black-Scholes (mcamd_bs_price_f64) at the
 * average variance theta + (v0 - theta)(1 - e^{-kappa T}) / (kappa T) (v0 at kappa = 0; the discounted intrinsic value
 * of the forward where that is 0).  The model's price has a slope in xi at 0 (the skew rho buys: up to 5 per unit
 * of xi at a spot of 100 on the tests' inputs), so the step across the threshold is that slope times 1e-8: below
 * 1e-9 S0.
 * Refuses a NULL price, payoff out of range, what mcamd_price_heston refuses of q, v0, kappa, theta, xi and rho,
 * S0 <= 0, K <= 0, T <= 0 and a non-finite S0, K, T or r. */
#define MCAMD_HESTON_XI_MIN 1e-8
int mcamd_heston_price_f64(double S0, double K, double T, double r, double q, double v0, double kappa, double theta,
                           double xi, double rho, int payoff, double *price);

/* Host closed form of mcamd_price_heston_cliquet's payoffs under the model itself (not the scheme), without a global
 * clip.  tau = T / n_periods; period p = 1..n_periods starts at t = (p - 1) tau; P = n_periods - first_period + 1.
 * The period's log-return D_p has the forward characteristic function
 *   E[e^{iu D_p}] = exp(iu (r - q) tau + C(tau, u)) M_t(D(tau, u)),
 * with C and D the coefficients of mcamd_heston_price_f64's branch-cut-safe form (ln phi = C + D v0) and
 *   M_t(w) = E[e^{w v_t}] = (1 - 2cw)^{-2 kappa theta / xi^2} exp(w v0 e^{-kappa t} / (1 - 2cw)),
 *   c = xi^2 (1 - e^{-kappa t}) / (4 kappa),
 * (1 - e^{-kappa t}) / kappa through expm1 (t at kappa = 0, where the power is 1), the power through a complex logarithm
 * arranged so that nothing is divided by xi^2; M_0(w) = e^{w v0}.
 *   SUM: c_p(k) = E[(e^{D_p} - k)+] by the Lewis integral and the quadrature rule of mcamd_heston_price_f64 with
 *       F = e^{(r-q) tau}; F - k for k <= 0, 0 for k = +inf.  Where kappa theta = 0 zero absorbs the variance: a path
 *       enters the period at v_t = 0 with probability P0 = lim_{w -> -inf} M_t(w) = exp(-v0 e^{-kappa t} / (2c)) and then
 *       earns the forward exactly, a mass that keeps the characteristic function from decaying; its call P0 (F - k)+ is
 *       added in closed form and the integral takes phi - P0.  F_lo = max(local_floor, -1),
 *       E_p = (1 + F_lo) + c_p(1 + F_lo) - c_p(1 + local_cap), price = e^{-rT} sum_{p >= first_period} (E_p - 1): exact
 *       whatever the number of periods, because expectations add although the periods depend on each other.
 *   VARIANCE: price = e^{-rT} (1 / (P tau)) sum_{p >= first_period} E[D_p^2], the exact mean of the DISCRETELY sampled
 *       realized variance (its continuous-sampling limit theta + (v0 - theta)(e^{-kappa t_1} - e^{-kappa T}) /
 *       (kappa (T - t_1)) is not what is returned).  E[D_p^2] = k2 + k1^2 from the first two cumulants of D_p, each a
 *       central difference of ln phi_p at h = 1/32 and 2h combined as (4 g(h) - g(2h)) / 3 (error of order h^4 times
 *       the fifth and sixth cumulants): within 1e-8 relative of -phi_p''(0) evaluated at 30 digits on the inputs of
 *       tests/test_heston_cliquet_cpu.py.
 *   COMPOUND: the periods depend on each other through v, so there is no product form.  Served where one period counts
 *       (first_period == n_periods: it is the SUM form) and below MCAMD_HESTON_XI_MIN; refused otherwise.
 * Below xi = MCAMD_HESTON_XI_MIN the variance is taken as deterministic: mcamd_cliquet_price_f64 at the period
 * volatilities v_p^2 = the average of theta + (v0 - theta) e^{-kappa s} over period p (and its refusal of a volatility
 * that is 0).
 * Refuses a NULL price, kind out of range, what mcamd_price_cliquet refuses of the local bounds, what mcamd_price_heston
 * refuses of q, v0, kappa, theta, xi and rho, T <= 0, a non-finite T or r, n_periods == 0, first_period outside
 * 1..n_periods, and the COMPOUND form described above. */
int mcamd_heston_cliquet_price_f64(int kind, double T, double r, double q, double v0, double kappa, double theta,
                                   double xi, double rho, uint32_t n_periods, uint32_t first_period,
                                   double local_floor, double local_cap, double *price);

/* Host: discount + mean + standard error + 95% CI from (sum, sumsq, n) — after an all-reduce
 * over shards, or directly.  Fills price/std_err/ci_* (and copies sum/sumsq/n) in *res. */
int mcamd_finalize(double sum, double sumsq, uint64_t n, double r, double T, mcamd_result *res);

/* Host: as mcamd_finalize for a control-variate run.  sums = {sum y, sum y^2, sum c, sum c^2, sum y c} with c already
 * centred on its known mean (what mcamd_price_paths returns in sum, sumsq, sum_c, sum_cc, sum_yc — after an
 * all-reduce over shards, or directly): price = exp(-rT) (ybar - beta cbar), beta = cov(y,c)/var(c),
 * std_err from the residual variance var(y)(1 - rho^2). */
int mcamd_finalize_cv(const double sums[5], uint64_t n, double r, double T, mcamd_result *res);

/* Host: the reference's serial CPU Monte Carlo (the baseline of BASELINE configs[0]), restated: fp32 paths and an fp32
 * running sum, std::mt19937 + std::normal_distribution<float>, one draw per step in path order,
 *   St *= expf((r - v^2/2) dt + v sqrtf(dt) G),   count += (St < B)  [use_window],   payoff max(St - K, 0) if the
 *   window admits the count,   price = expf(-r T) * sum / n_paths.
 * n_steps = 1 with use_window = 0 is simulateOptionPriceCPU (inc/tool.cuh:104-130); n_steps = N_STEPS with the window is
 * simulateBulletOptionPriceCPU (inc/tool.cuh:133-173).  dt = opt->dt, or T / n_steps when that is 0.  The reference seeds
 * from std::random_device and is not reproducible (inc/tool.cuh:116,151): from_random_device != 0 does the same; otherwise
 * the generator is std::mt19937(seed), which makes the path testable.  payoff_sum (nullable) receives the undiscounted fp32
 * sum.  This is the reference's CPU baseline, not a fallback: no GPU entry point ever routes here.  Single thread. */
int mcamd_cpu_mc_f32(const mcamd_option *opt, uint64_t n_paths, uint32_t n_steps, uint64_t seed, int from_random_device,
                     float *price, float *payoff_sum);

/* Host closed form.  _f32 restates the reference's fp32 code path operation for operation
 * (CND: inc/BlackandScholes.hpp:8-30; black_scholes_CPU: :34-43); _f64 is the exact erfc form. */
float mcamd_cnd_f32(float x);
float mcamd_bs_call_f32(float x0, float strike, float T, float r, float sigma);
double mcamd_bs_call_f64(double x0, double strike, double T, double r, double sigma);

#ifdef __cplusplus
}
#endif
#endif /* MCAMD_H */
