// lookback.hip — lookback options for gfx950 (both path precisions): floating or fixed strike, call or put, monitored
// at the step ends (discrete) or all the time (continuous, by sampling the Brownian-bridge extremum of every step).
//
// Definitions (include/mcamd.h, mcamd_price_lookback): X_i = ln(S_i / S0) after step i, E_0 = 0, and E_i is the
// running maximum (floating put, fixed call) or minimum (floating call, fixed put) of X.  Discrete: E_i =
// max(E_{i-1}, X_i).  Continuous, for the maximum: E^ = max(E_{i-1}, X_i), q_i = 2 (E^ - X_{i-1})(E^ - X_i) / (v^2 dt),
// and where q_i < Q (22.25 in fp32, 36.75 in fp64) the bridge maximum m_i = (X_{i-1} + X_i + sqrt(x_i^2 - 2 v^2 dt
// ln U_i)) / 2 enters: E_i = max(E^, m_i); elsewhere E_i = E^ (no uniform the generator can produce would move it).
// The minimum is the mirror image.  The sample is formed once per path in fp64 from S_T = S0 e^{X_n} and
// S_E = S0 e^{E_n}, both through exp_of_logreturn, so a path whose extremum is its last point has S_E == S_T.
//
// The loop is walk_steps (mc_device.hpp) in log space: per Philox block one Exponents<T>::fill and — continuous —
// one more Philox block at 2^63 + k for the step uniforms; per step acc += x, one max / min, and for the bridge two
// subtracts, two multiplies and a compare for q, a logarithm, a fused multiply-add, a root, two adds, a multiply, one
// max / min and a select.  The bridge is predicated per lane, not skipped per wavefront: at 50 steps a half to three
// quarters of the lanes have q < Q at any step and at 252 steps still more than a third, so a wavefront with no such
// lane does not occur, and without the branch the compiler is free to interleave the transcendentals of a block's steps.
#include "lookback.hpp"
#include "path_consts.hpp"
#include "path_frame.hpp"

namespace mcamd {

template <typename T>
struct LookbackArgs {
    StepConsts<T> c;   // drift, vol, S_start, n_sim in exponent units (K, B, logB unused)
    T kq;              // 2 u^2 / (v^2 dt), u = natural log per exponent unit: q = kq d d' in natural-log units
    T kb;              // fp64: v^2 dt / u^2, times f64::neg2log(U) = -2 ln U; fp32: 2 ln 2 v^2 dt / u^2, times -log2 U
    T q_cut;           // Q, natural-log units
    double K;          // fixed strike
    int fixed, put;
    PathShard shard;
    T *samples;        // nullable
    GridFinish fin;
};

// The uniforms' block of a step block: same key and subsequence, 2^63 beyond (n_steps is 32-bit: the normals never
// get there).
constexpr uint64_t kUniformBlocks = 1ull << 63;

// What the bridge root needs of the step uniforms of one Philox block, one per step of Exponents<T>.
// fp32: word j serves step 4k + j, U = fma(word, 2^-32, 2^-32) (rocRAND's float uniform; may round to 1); l = -log2 U.
// fp64: (x, y) serve step 2k and (z, w) step 2k + 1, U = ((x ^ (y << 21)) + 1) 2^-53 (f64::u53); l = -2 ln U.
template <typename T>
struct BridgeLogs;

template <>
struct BridgeLogs<float> {
    float l[4];
    __device__ __forceinline__ void fill(const MathCtx<float> &, const PhiloxKeys &key, uint64_t subsequence,
                                         uint64_t block)
    {
        constexpr float k2pow32inv = 2.3283064365386963e-10f;
        const U4 w = philox_block(key, subsequence, kUniformBlocks + block);
        const uint32_t word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            l[j] = -__builtin_amdgcn_logf(__builtin_fmaf(static_cast<float>(word[j]), k2pow32inv, k2pow32inv));
    }
};

template <>
struct BridgeLogs<double> {
    double l[2];
    __device__ __forceinline__ void fill(const MathCtx<double> &m, const PhiloxKeys &key, uint64_t subsequence,
                                         uint64_t block)
    {
        const U4 w = philox_block(key, subsequence, kUniformBlocks + block);
        l[0] = f64::neg2log(f64::u53(w.x, w.y, 0x1p-53), m.t.log_tab);
        l[1] = f64::neg2log(f64::u53(w.z, w.w, 0x1p-53), m.t.log_tab);
    }
};

__device__ __forceinline__ float max_t(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double max_t(double a, double b) { return __builtin_fmax(a, b); }
__device__ __forceinline__ float min_t(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double min_t(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ float root_t(float a) { return __builtin_amdgcn_sqrtf(a); }   // a >= 0
// a > 0: x^2 + kb l with l = f64::neg2log(U) strictly positive for every U in (0, 1] (fast64.hpp)
__device__ __forceinline__ double root_t(double a) { return f64::sqrt_unclamped(a); }

template <typename T, bool MAXIMUM, bool CONT>
__global__ __launch_bounds__(kBlock) void lookback_kernel(LookbackArgs<T> a, double *__restrict__ partials)
{
    constexpr int NB = Exponents<T>::kPerBlock;
    const MathCtx<T> m = MathCtx<T>::init();
    const PhiloxKeys key = PhiloxKeys::make(a.shard.seed);
    const StepConsts<T> c = resident(a.c);
    // the bridge constants of the full-rate fp32 instructions belong in vector registers
    const T kq = resident_t(a.kq), kb = resident_t(a.kb), q_cut = resident_t(a.q_cut);
    const StepBlocks blocks = step_blocks<NB>(c.n_sim);
    double acc4[kLookbackRecord] = {0.0, 0.0, 0.0, 0.0};
    for (const uint64_t i : ThreadPaths{a.shard.n_local}) {
        const uint64_t subsequence = a.shard.path_offset + i;
        T acc = T(0);        // X so far, in exponent units
        T E = T(0);          // its running extremum: the option is newly issued, so S0 counts
        uint32_t live = 0;   // steps whose bridge extremum was formed (q < Q)
        Exponents<T> ex;
        BridgeLogs<T> bl;
        auto step = [&](T x, T l) {
            const T x_prev = acc;
            acc += x;
            E = MAXIMUM ? max_t(E, acc) : min_t(E, acc);
            if (CONT) {
                const T d_prev = MAXIMUM ? E - x_prev : x_prev - E;
                const T d = MAXIMUM ? E - acc : acc - E;
                const T q = kq * d_prev * d;
                const bool close_by = q < q_cut;
                const T root = root_t(fma_t(kb, l, x * x));
                const T ends = x_prev + acc;
                const T mid = T(0.5) * (MAXIMUM ? ends + root : ends - root);
                const T with_bridge = MAXIMUM ? max_t(E, mid) : min_t(E, mid);
                E = close_by ? with_bridge : E;
                live += close_by ? 1u : 0u;
            }
        };
        walk_steps<NB>(
            blocks,
            [&](uint32_t k) {
                ex.fill(m, c, key, subsequence, k);
                if (CONT) bl.fill(m, key, subsequence, k);
            },
            [&](uint32_t, int j) { step(ex.x[j], CONT ? bl.l[j] : T(0)); });
        // the same routine for both prices: E == acc bit for bit gives S_E == S_T, and a floating sample of exactly 0
        const double St = static_cast<double>(exp_of_logreturn(c.S_start, acc, m));
        const double Se = static_cast<double>(exp_of_logreturn(c.S_start, E, m));
        double y;
        if (a.fixed) {
            y = a.put ? a.K - Se : Se - a.K;
            y = y > 0.0 ? y : 0.0;
        } else {
            y = a.put ? Se - St : St - Se;
        }
        if (a.samples) a.samples[i] = static_cast<T>(y);
        add_sample(acc4, y);
        add_counters(acc4, c.n_sim, live);
    }
    if (a.fin.n_value >= 0.0) acc4[2] = acc4[3] = 0.0;   // the 6-double statistics layout has no slot for the counters
    finish_paths(acc4, partials, a.fin);
}

template <typename T, bool MAXIMUM>
static void launch_lookback_k(const LookbackJob &j, const LookbackArgs<T> &a, double *d_partials, uint32_t grid,
                              hipStream_t stream)
{
    const dim3 g(grid), b(kBlock);
    if (j.continuous) hipLaunchKernelGGL((lookback_kernel<T, MAXIMUM, true>), g, b, 0, stream, a, d_partials);
    else hipLaunchKernelGGL((lookback_kernel<T, MAXIMUM, false>), g, b, 0, stream, a, d_partials);
}

template <typename T>
static hipError_t launch_lookback_t(const LookbackJob &j, double *d_partials, uint32_t grid, const FinishSpec &fs,
                                    hipStream_t stream)
{
    // log_unit: what the precision's logarithm of U has to be multiplied by to give -2 ln U (v_log_f32 is a log2;
    // f64::neg2log is -2 ln already)
    const double u = exponent_unit<T>();
    const double log_unit = sizeof(T) == 4 ? 2.0 * kLn2 : 1.0;
    const double q_cut = sizeof(T) == 4 ? 22.25 : 36.75;
    const LookbackArgs<T> a{make_consts<T>(j.path), static_cast<T>(2.0 * u * u / j.v2dt),
                            static_cast<T>(j.v2dt * log_unit / (u * u)), static_cast<T>(q_cut), j.K, j.fixed ? 1 : 0,
                            j.put ? 1 : 0, shard_of(j.path), static_cast<T *>(j.d_samples), grid_finish_of(fs)};
    if (j.maximum) launch_lookback_k<T, true>(j, a, d_partials, grid, stream);
    else launch_lookback_k<T, false>(j, a, d_partials, grid, stream);
    return hipGetLastError();
}

hipError_t launch_lookback(const LookbackJob &job, double *d_partials, uint32_t grid, const FinishSpec &finish,
                           hipStream_t stream)
{
    if (!finish_ok(finish, grid)) return hipErrorInvalidValue;
    return dispatch_precision(job.path.precision, [&](auto p) {
        return launch_lookback_t<typename decltype(p)::type>(job, d_partials, grid, finish, stream);
    });
}

}  // namespace mcamd
