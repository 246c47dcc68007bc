// device_math_check.hip — test helper (built by tests/device_math_harness.py with the library's own compile flags):
// runs the SHIPPED fp64 / fp32 building blocks of csrc/fast64.hpp and csrc/mc_device.hpp on crafted Philox words, so
// tests/test_gpu_device_math.py can compare each call, element by element, with an extended-precision reference —
// the arithmetic the GPU runs (v_rsq_f64 seed, inline assembly, hipcc's contraction default, the LDS table copies),
// not the host build of the same header.  Philox is bypassed: the tests supply the words.  Not part of the product.
//
// Every kernel builds its tables with MathCtx<T>::init<ROTATED>() exactly as the pricing kernels do: every thread of
// the workgroup calls it (it holds a barrier) before the bounds check, and workgroups are whole 64-lane wavefronts.
// Launchers return the hipDeviceSynchronize status.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "mc_device.hpp"
#include "path_consts.hpp"

using namespace mcamd;

namespace {

constexpr int kThreads = 256;

inline dim3 grid_for(uint64_t n) { return dim3(static_cast<uint32_t>((n + kThreads - 1) / kThreads)); }

// (a) the radius: u53, neg2log, sqrt_unclamped and sqrt_scaled(., k[i]) from the words (x, y)
__global__ void k_radius(uint64_t n, const uint32_t *x, const uint32_t *y, const double *k, double *u, double *a,
                         double *su, double *ss)
{
    const MathCtx<double> m = MathCtx<double>::init<false>();
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const double uu = f64::u53(x[i], y[i], 0x1p-53);
    const double aa = f64::neg2log(uu, m.t.log_tab);
    u[i] = uu;
    a[i] = aa;
    su[i] = f64::sqrt_unclamped(aa);
    ss[i] = f64::sqrt_scaled(aa, k[i]);
}

// (b) the angle on the plain table: sincos_bits(z, w)
__global__ void k_sincos(uint64_t n, const uint32_t *z, const uint32_t *w, double *s, double *c)
{
    const MathCtx<double> m = MathCtx<double>::init<false>();
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    double sn, cs;
    f64::sincos_bits(z[i], w[i], m.t.sincos_tab, sn, cs);
    s[i] = sn;
    c[i] = cs;
}

// (b) the angle on the table rotated by N/8 (the pair-sum loop's): sin_bits_rotated<true> (sine and cosine), and
// the sine of the <false> form, which must be the same bits
__global__ void k_rotated(uint64_t n, const uint32_t *z, const uint32_t *w, double *s, double *c, double *s_only)
{
    const MathCtx<double> m = MathCtx<double>::init<true>();
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    double cs;
    s[i] = f64::sin_bits_rotated<true>(z[i], w[i], m.t.sincos_tab, &cs);
    c[i] = cs;
    s_only[i] = f64::sin_bits_rotated<false>(z[i], w[i], m.t.sincos_tab, nullptr);
}

// (c) fp64 Box-Muller of one block's words (plain table): z0, z1
__global__ void k_box_muller64(uint64_t n, const U4 *words, double *z0, double *z1)
{
    const MathCtx<double> m = MathCtx<double>::init<false>();
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    double a, b;
    box_muller(words[i], m, a, b);
    z0[i] = a;
    z1[i] = b;
}

// (c) the fp64 pair sum (rotated table): add_words(0, w) and head_words(w), both in units of PairSum<double>::kUnit
__global__ void k_pairsum64(uint64_t n, const U4 *words, double *sum, double *head)
{
    const MathCtx<double> m = MathCtx<double>::init<true>();
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    sum[i] = PairSum<double>::add_words(0.0, words[i], m);
    head[i] = PairSum<double>::head_words(words[i], m);
}

// (c) fp32: box_muller(x, y), PairSum<float>::pair(x, y), polar(x, y) with shifts 0 and 1/8, head_words(w, 1 | 3).
// out32 holds 9 floats per element: z0, z1, pair, t, rev (shift 0), t, rev (shift 1/8), head(1), head(3).
__global__ void k_f32(uint64_t n, const U4 *words, float *out32)
{
    const MathCtx<float> m = MathCtx<float>::init<false>();
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const U4 w = words[i];
    float *o = out32 + 9 * i;
    float a, b, t, rev;
    box_muller(w.x, w.y, a, b);
    o[0] = a;
    o[1] = b;
    o[2] = PairSum<float>::pair(w.x, w.y);
    PairSum<float>::polar(w.x, w.y, 0.0f, t, rev);
    o[3] = t;
    o[4] = rev;
    PairSum<float>::polar(w.x, w.y, 0.125f, t, rev);
    o[5] = t;
    o[6] = rev;
    o[7] = PairSum<float>::head_words(w, m, 1);
    o[8] = PairSum<float>::head_words(w, m, 3);
}

// (d) one exponential: f64::mul_exp(S, x) (x in natural units) and exp_of_logreturn(S, y) (y in exponent units)
__global__ void k_exp(uint64_t n, const double *S, const double *x, const double *y, double *me, double *el)
{
    const MathCtx<double> m = MathCtx<double>::init<false>();
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    me[i] = f64::mul_exp(S[i], x[i], m.t.exp_hi_tab, m.t.exp_lo_tab);
    el[i] = exp_of_logreturn(S[i], y[i], m);
}

// (d) PathState<double>: start(S[lane]), then step(y) n_steps times with lane `lane` reading the sequence
// y_tab[lane_pat[lane] * n_steps + ...]; value(), a.k and a.P after every step (lane-major: [lane * n_steps + step])
__global__ void k_path(uint32_t lanes, uint32_t n_steps, const double *y_tab, const uint32_t *lane_pat, const double *S,
                       double *value, int32_t *k, double *P)
{
    const MathCtx<double> m = MathCtx<double>::init<false>();
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= lanes) return;
    const double *y = y_tab + static_cast<uint64_t>(lane_pat[lane]) * n_steps;
    PathState<double> ps = PathState<double>::start(S[lane]);
    for (uint32_t s = 0; s < n_steps; ++s) {
        ps.step(y[s], m);
        const uint64_t o = static_cast<uint64_t>(lane) * n_steps + s;
        value[o] = ps.value(m);
        k[o] = ps.a.k;
        P[o] = ps.a.P;
    }
}

// (e) the barrier test of PathState<double>: arm_barrier(theta), then at every step step(y) and below_barrier(c, m).
// flags[lane * n_steps + step]: bit 0 what below_barrier returned, bit 1 c.B > value(m), bit 2 the lane's wavefront was
// all-sure (no lane had |q| <= win_delta: below_barrier took the cheap branch); q_out the q it decided from.
// restart == 0: the path starts at c.S_start and theta = c.logB (the pricing kernels);
// restart != 0: it starts at St0[lane] and theta = c.logB - log_ratio(St0, c.S_start), computed here (nmc.hip,
// nmc_compact.hpp, simulate_sample's log_start).
__global__ void k_barrier(uint32_t lanes, uint32_t n_steps, const StepConsts<double> *consts, const double *y_tab,
                          const uint32_t *lane_pat, const double *St0, int restart, uint8_t *flags, float *q_out)
{
    const MathCtx<double> m = MathCtx<double>::init<false>();
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= lanes) return;
    const StepConsts<double> c = consts[lane];
    const double *y = y_tab + static_cast<uint64_t>(lane_pat[lane]) * n_steps;
    const double S = restart ? St0[lane] : c.S_start;
    PathState<double> ps = PathState<double>::start(S);
    ps.arm_barrier(restart ? c.logB - log_ratio(S, c.S_start) : c.logB);
    for (uint32_t s = 0; s < n_steps; ++s) {
        ps.step(y[s], m);
        const int32_t below = ps.below_barrier(c, m);
        // the same expression as below_barrier's, and the same ballot
        const double q = __builtin_fma(ps.a.P, f64::kExpScale, ps.kq);
        const bool unsure = !(__builtin_fabs(q) > c.win_delta);
        const bool all_sure = __builtin_amdgcn_ballot_w64(unsure) == 0;
        const bool exact = c.B > ps.value(m);
        const uint64_t o = static_cast<uint64_t>(lane) * n_steps + s;
        flags[o] = static_cast<uint8_t>((below & 1) | (exact ? 2 : 0) | (all_sure ? 4 : 0));
        q_out[o] = static_cast<float>(q);
    }
}

PathJob job_for(uint32_t n_steps, double B, double S_start)
{
    PathJob j{};
    j.B = B;
    j.S_start = S_start;
    j.n_steps = n_steps;
    j.n_sim = n_steps;
    j.window = true;
    j.precision = 64;
    return j;
}

}  // namespace

extern "C" {

int dm_radius(uint64_t n, const uint32_t *x, const uint32_t *y, const double *k, double *u, double *a, double *su,
              double *ss)
{
    hipLaunchKernelGGL(k_radius, grid_for(n), dim3(kThreads), 0, 0, n, x, y, k, u, a, su, ss);
    return static_cast<int>(hipDeviceSynchronize());
}

int dm_sincos(uint64_t n, const uint32_t *z, const uint32_t *w, double *s, double *c)
{
    hipLaunchKernelGGL(k_sincos, grid_for(n), dim3(kThreads), 0, 0, n, z, w, s, c);
    return static_cast<int>(hipDeviceSynchronize());
}

int dm_rotated(uint64_t n, const uint32_t *z, const uint32_t *w, double *s, double *c, double *s_only)
{
    hipLaunchKernelGGL(k_rotated, grid_for(n), dim3(kThreads), 0, 0, n, z, w, s, c, s_only);
    return static_cast<int>(hipDeviceSynchronize());
}

int dm_box_muller64(uint64_t n, const uint32_t *words, double *z0, double *z1)
{
    hipLaunchKernelGGL(k_box_muller64, grid_for(n), dim3(kThreads), 0, 0, n, reinterpret_cast<const U4 *>(words), z0, z1);
    return static_cast<int>(hipDeviceSynchronize());
}

int dm_pairsum64(uint64_t n, const uint32_t *words, double *sum, double *head)
{
    hipLaunchKernelGGL(k_pairsum64, grid_for(n), dim3(kThreads), 0, 0, n, reinterpret_cast<const U4 *>(words), sum, head);
    return static_cast<int>(hipDeviceSynchronize());
}

int dm_f32(uint64_t n, const uint32_t *words, float *out32)
{
    hipLaunchKernelGGL(k_f32, grid_for(n), dim3(kThreads), 0, 0, n, reinterpret_cast<const U4 *>(words), out32);
    return static_cast<int>(hipDeviceSynchronize());
}

int dm_exp(uint64_t n, const double *S, const double *x, const double *y, double *me, double *el)
{
    hipLaunchKernelGGL(k_exp, grid_for(n), dim3(kThreads), 0, 0, n, S, x, y, me, el);
    return static_cast<int>(hipDeviceSynchronize());
}

// lanes: a multiple of 64 (whole wavefronts)
int dm_path(uint32_t lanes, uint32_t n_steps, const double *y_tab, const uint32_t *lane_pat, const double *S,
            double *value, int32_t *k, double *P)
{
    if (lanes % kWave != 0) return -1;
    hipLaunchKernelGGL(k_path, grid_for(lanes), dim3(kThreads), 0, 0, lanes, n_steps, y_tab, lane_pat, S, value, k, P);
    return static_cast<int>(hipDeviceSynchronize());
}

// Host only: the constants make_consts<double> derives for a job of n_steps steps with barrier B from S_start.
void dm_consts(uint32_t n_steps, double B, double S_start, double *logB, double *win_delta)
{
    const StepConsts<double> c = make_consts<double>(job_for(n_steps, B, S_start));
    *logB = c.logB;
    *win_delta = c.win_delta;
}

// B, S_start: host arrays of one value per lane (the StepConsts of each lane are built here, with make_consts);
// lanes: a multiple of 64.  The other pointers are device memory.
int dm_barrier(uint32_t lanes, uint32_t n_steps, const double *B, const double *S_start, const double *y_tab,
               const uint32_t *lane_pat, const double *St0, int restart, uint8_t *flags, float *q_out)
{
    if (lanes % kWave != 0) return -1;
    std::vector<StepConsts<double>> h(lanes);
    for (uint32_t l = 0; l < lanes; ++l) h[l] = make_consts<double>(job_for(n_steps, B[l], S_start[l]));
    StepConsts<double> *d = nullptr;
    hipError_t e = hipMalloc(&d, sizeof(StepConsts<double>) * lanes);
    if (e != hipSuccess) return static_cast<int>(e);
    e = hipMemcpy(d, h.data(), sizeof(StepConsts<double>) * lanes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_barrier, grid_for(lanes), dim3(kThreads), 0, 0, lanes, n_steps, d, y_tab, lane_pat, St0,
                           restart, flags, q_out);
        e = hipDeviceSynchronize();
    }
    const hipError_t f = hipFree(d);
    return static_cast<int>(e != hipSuccess ? e : f);
}

}  // extern "C"
