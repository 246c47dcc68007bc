// american_device.hpp — the device functions both passes of american.hip decide and fit with: the payoff, the fitted
// continuation value, the exercise decision and the normal-equation solver of one date.  A header of their own so
// that tests/american_solve_check.hip runs them call by call, compiled as the kernels compile them.
#pragma once

#include <hip/hip_runtime.h>

namespace mcamd {

__device__ __forceinline__ double am_payoff(bool put, double K, double S)
{
    const double x = put ? K - S : S - K;
    return x > 0.0 ? x : 0.0;
}

// phi(S) . beta by Horner, with explicit fused multiply-adds (no contraction choice left to the compiler)
template <int MB>
__device__ __forceinline__ double am_continuation(const double (&beta)[MB], double u)
{
    double c = beta[MB - 1];
#pragma unroll
    for (int q = MB - 2; q >= 0; --q) c = __builtin_fma(c, u, beta[q]);
    return c;
}

// The exercise decision of both passes at a regressed date: true (y = d h(S)) when h(S) > 0 and d h(S) beats the
// fitted continuation value phi(S) . beta.
template <int MB>
__device__ __forceinline__ bool am_exercise(const double (&beta)[MB], double disc, double K, bool put, double S,
                                            double &y)
{
    const double h = am_payoff(put, K, S);
    if (!(h > 0.0)) return false;
    y = disc * h;
    return y > am_continuation<MB>(beta, S / K - 1.0);
}

// Normal equations of one date from its record: A = Hankel(P_0..P_{2m-2}), b = (sum V u^q).  Jacobi scaling
// D = diag(A)^(-1/2), Cholesky of D A D, two triangular solves, beta = D z.  Returns false — date not regressed — when
// |I_j| < 4 m or not finite, a diagonal entry is not positive, a scaled pivot is <= kAmPivotMin or a coefficient is not
// finite (NaN records included: the comparisons are written so that NaN fails them; a NaN or inf cross sum reaches no
// pivot, only beta).  Fields the basis does not use (P_{2m-1}.., sum V u^q for q >= m) are not read.
// pivot_min is kAmPivotMin in every kernel; the tests' harness also measures the fit under other thresholds.
constexpr double kAmPivotMin = 1e-10;   // fitted values are good to about 5 * 2^-53 / pivot of their scale

template <int MB>
__device__ __forceinline__ bool am_solve(const double *__restrict__ rec, double (&beta)[MB],
                                         double pivot_min = kAmPivotMin)
{
    bool ok = rec[11] >= 4.0 * MB && rec[11] < __builtin_inf();
    double D[MB];
#pragma unroll
    for (int a = 0; a < MB; ++a) {
        const double d = rec[2 * a];
        ok = ok && d > 0.0;
        D[a] = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
    }
    double L[MB][MB];
#pragma unroll
    for (int c = 0; c < MB; ++c) {
        double s = rec[2 * c] * D[c] * D[c];
#pragma unroll
        for (int q = 0; q < c; ++q) s -= L[c][q] * L[c][q];
        ok = ok && s > pivot_min;
        const double l = sqrt(s > pivot_min ? s : 1.0);
        L[c][c] = l;
#pragma unroll
        for (int r = c + 1; r < MB; ++r) {
            double t = rec[r + c] * D[r] * D[c];
#pragma unroll
            for (int q = 0; q < c; ++q) t -= L[r][q] * L[c][q];
            L[r][c] = t / l;
        }
    }
    double y[MB];
#pragma unroll
    for (int a = 0; a < MB; ++a) {
        double t = rec[7 + a] * D[a];
#pragma unroll
        for (int q = 0; q < a; ++q) t -= L[a][q] * y[q];
        y[a] = t / L[a][a];
    }
#pragma unroll
    for (int a = MB - 1; a >= 0; --a) {
        double t = y[a];
#pragma unroll
        for (int q = a + 1; q < MB; ++q) t -= L[q][a] * beta[q];
        beta[a] = t / L[a][a];
    }
#pragma unroll
    for (int a = 0; a < MB; ++a) {
        beta[a] *= D[a];
        ok = ok && __builtin_fabs(beta[a]) < __builtin_inf();
    }
    return ok;
}

}  // namespace mcamd
