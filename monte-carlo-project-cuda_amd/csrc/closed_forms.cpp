// closed_forms.cpp — every host formula of the C ABI that touches no device: the Black-Scholes family, the closed
// forms the product tests price against, and the host lookup of a local-volatility table.  Compiled with the flags of
// the other C ABI files (no contraction), so a formula a prepare_* step shares gives the bits it gives here.
#define MCAMD_CAPI_HOST_ONLY
#include "capi_internal.hpp"
#include "mcamd_heston_greeks.h"

#include <algorithm>
#include <complex>
#include <vector>

using namespace mcamd::capi;

namespace mcamd::capi {

// Black-Scholes with a dividend yield at volatility v > 0 and its vega; every argument checked by the caller
double bs_value(double S0, double K, double T, double r, double q, double v, bool call, double *vega)
{
    const double sqrtT = std::sqrt(T);
    const double d1 = (std::log(S0 / K) + (r - q + 0.5 * v * v) * T) / (v * sqrtT), d2 = d1 - v * sqrtT;
    const double Sd = S0 * std::exp(-q * T), Kd = K * std::exp(-r * T);
    if (vega) *vega = Sd * sqrtT * std::exp(-0.5 * d1 * d1) * 0.3989422804014327;
    return call ? Sd * norm_cdf(d1) - Kd * norm_cdf(d2) : Kd * norm_cdf(-d2) - Sd * norm_cdf(-d1);
}

// The discrete geometric average of geometric Brownian motion over the step ends i = 1..n (and t = 0 with
// include_spot; m dates in all) is lognormal: ln G ~ N(M, s^2) with M = ln S0 + mu dt n(n+1) / (2m) and
// s^2 = v^2 dt n(n+1)(2n+1) / (6 m^2), mu = r - v^2/2.  The floating strike exchanges G for S_T, two lognormals with
// covariance v^2 dt n(n+1) / (2m) of their logarithms (Margrabe's form on the forwards).
int asian_geometric_price(double S0, double K, double T, double r, double v, uint32_t n_steps, int include_spot,
                          int strike, int payoff, double *price)
{
    *price = 0.0;
    if (!(S0 > 0.0) || !(T > 0.0) || !(v > 0.0) || !std::isfinite(S0) || !std::isfinite(T) || !std::isfinite(r) ||
        !std::isfinite(v))
        return fail(MCAMD_ERR_INVALID, "the geometric Asian closed form needs finite S0, T, v > 0 and a finite r");
    if (n_steps == 0) return fail(MCAMD_ERR_INVALID, "n_steps must be >= 1");
    if (int rc = check_asian_kind(K, strike, payoff, include_spot)) return rc;
    const double n = static_cast<double>(n_steps), m = n + include_spot, dt = T / n;
    const double mu = r - 0.5 * v * v, D = std::exp(-r * T);
    const double M = std::log(S0) + mu * dt * n * (n + 1.0) / (2.0 * m);
    const double s2 = v * v * dt * n * (n + 1.0) * (2.0 * n + 1.0) / (6.0 * m * m);
    const double F = std::exp(M + 0.5 * s2);   // E[G]
    const bool put = payoff == MCAMD_PAYOFF_PUT;
    if (strike == MCAMD_ASIAN_FIXED) {
        const double s = std::sqrt(s2);
        const double d1 = (M - std::log(K)) / s + s;
        const double call = D * (F * norm_cdf(d1) - K * norm_cdf(d1 - s));
        *price = put ? call - D * (F - K) : call;
        return MCAMD_OK;
    }
    const double sf2 = v * v * T + s2 - v * v * dt * n * (n + 1.0) / m;
    // one step without the spot: the average IS S_T, and the option pays nothing
    if ((n_steps == 1 && !include_spot) || !(sf2 > 0.0)) return MCAMD_OK;
    const double F1 = S0 * std::exp(r * T), sf = std::sqrt(sf2);
    const double d1 = (std::log(F1 / F) + 0.5 * sf2) / sf;
    const double call = D * (F1 * norm_cdf(d1) - F * norm_cdf(d1 - sf));
    *price = put ? call - D * (F1 - F) : call;
    return MCAMD_OK;
}

}  // namespace mcamd::capi

namespace {

using cplx = std::complex<double>;

// e^x - 1 for a complex x without the cancellation at small |x|
cplx c_expm1(cplx x)
{
    const double a = x.real(), b = x.imag(), sh = std::sin(0.5 * b);
    return {std::expm1(a) * std::cos(b) - 2.0 * sh * sh, std::exp(a) * std::sin(b)};
}

// ln(1 + z) / z for a complex z, 1 at z = 0 (Kahan's quotient: the rounding of 1 + z cancels)
cplx c_log1p_over(cplx z)
{
    const cplx w = 1.0 + z;
    if (w == cplx(1.0, 0.0)) return 1.0 - 0.5 * z;
    return std::log(w) / (w - 1.0);
}

// ln E[e^{iu x}] of x = ln(S_T / F) under Heston in the branch-cut-safe form (Albrecher, Mayer, Schoutens, Tistaert
// 2007), rearranged so that nothing is divided by xi^2.  With A = u^2 + iu, b = kappa - rho xi iu, d = sqrt(b^2 + xi^2 A)
// (principal root, Re d >= 0), the textbook (b - d) / xi^2 is -A / (b + d) (b^2 - d^2 = -xi^2 A: no cancellation),
// g = (b - d) / (b + d) = -xi^2 A / (b + d)^2, E = e^{-dT}, and
//     ln phi = kappa theta [ -A T / (b + d) - 2 ln(1 + z) / xi^2 ] - v0 A (1 - E) / ((b + d)(1 - g E)),
//     z = g (1 - E) / (1 - g),   ln(1 + z) / xi^2 = [ln(1 + z) / z] [-A (1 - E) / ((b + d)^2 (1 - g))].
// It stays finite down to xi = 0 unless kappa is 0 as well (b + d = 0), which the caller's limit serves.
cplx heston_log_cf(cplx u, double T, double v0, double kappa, double theta, double xi, double rho)
{
    const cplx iu = cplx(0.0, 1.0) * u, A = u * u + iu;
    const cplx b = kappa - rho * xi * iu, d = std::sqrt(b * b + xi * xi * A), bd = b + d;
    const cplx q = -A / bd, g = xi * xi * q / bd;
    const cplx one_minus_E = -c_expm1(-d * T), E = 1.0 - one_minus_E;
    const cplx z = g * one_minus_E / (1.0 - g);
    const cplx log_over_xi2 = c_log1p_over(z) * (q * one_minus_E / (bd * (1.0 - g)));
    return kappa * theta * (q * T - 2.0 * log_over_xi2) + v0 * q * one_minus_E / (1.0 - g * E);
}

constexpr int kGlNodes = 16;          // Gauss-Legendre nodes per panel
constexpr double kHestonPanel = 0.5;  // panel width in u
constexpr double kHestonRangeMin = 32.0, kHestonRangeMax = 4096.0;
constexpr double kHestonEnvelope = 1e-15;

// nodes and weights of the 16-point Gauss-Legendre rule on [-1, 1]: Newton steps on P_16 from the Chebyshev guess
void gauss_legendre(double x[kGlNodes], double w[kGlNodes])
{
    for (int i = 0; i < kGlNodes; ++i) {
        double t = std::cos(M_PI * (i + 0.75) / (kGlNodes + 0.5)), dp = 1.0;
        for (int it = 0; it < 100; ++it) {
            double p0 = 1.0, p1 = t;
            for (int k = 2; k <= kGlNodes; ++k) {
                const double p2 = ((2.0 * k - 1.0) * t * p1 - (k - 1.0) * p0) / k;
                p0 = p1;
                p1 = p2;
            }
            dp = kGlNodes * (t * p1 - p0) / (t * t - 1.0);
            const double step = p1 / dp;
            t -= step;
            if (std::fabs(step) < 1e-16) break;
        }
        x[i] = t;
        w[i] = 2.0 / ((1.0 - t * t) * dp * dp);
    }
}

// Lewis's integral int_0^U Re[e^{iuk} (phi(u - i/2) - atom)] / (u^2 + 1/4) du of a characteristic function given by its
// logarithm lnphi(u), by the rule of mcamd_heston_price_f64 (include/mcamd.h): 16 Gauss-Legendre nodes on each panel of
// width 1/2, U the first of 32, 64, .. 4096 at which the integrand's envelope |phi(U - i/2) - atom| / (U^2 + 1/4) is
// below 1e-15.  atom: the mass the distribution has at x = 0, which does not decay and which the caller integrates in
// closed form; 0 for a distribution without one.
template <typename LogCf>
double lewis_integral(double k, LogCf lnphi, double atom = 0.0)
{
    const auto integrand = [&](double u) {
        if (atom == 0.0) return (std::exp(lnphi(cplx(u, -0.5)) + cplx(0.0, u * k))).real() / (u * u + 0.25);
        return ((std::exp(lnphi(cplx(u, -0.5))) - atom) * std::exp(cplx(0.0, u * k))).real() / (u * u + 0.25);
    };
    const auto envelope = [&](double u) {
        if (atom == 0.0) return std::exp(lnphi(cplx(u, -0.5)).real()) / (u * u + 0.25);
        return std::abs(std::exp(lnphi(cplx(u, -0.5))) - atom) / (u * u + 0.25);
    };
    double U = kHestonRangeMin;
    while (U < kHestonRangeMax && envelope(U) >= kHestonEnvelope) U *= 2.0;
    double x[kGlNodes], w[kGlNodes];
    gauss_legendre(x, w);
    const int panels = static_cast<int>(U / kHestonPanel);
    double integral = 0.0;
    for (int p = 0; p < panels; ++p) {
        const double mid = (p + 0.5) * kHestonPanel;
        double s = 0.0;
        for (int i = 0; i < kGlNodes; ++i) s += w[i] * integrand(mid + 0.5 * kHestonPanel * x[i]);
        integral += 0.5 * kHestonPanel * s;
    }
    return integral;
}

// The integral of the spot derivative of Lewis's formula, int_0^U Re[(1/2 + iu) e^{iuk} phi(u - i/2)] / (u^2 + 1/4) du,
// by lewis_integral's rule (the same panels and nodes) with the envelope multiplied by U: the integrand gains the
// factor |1/2 + iu| and decays one power of u more slowly.  For a distribution without an atom.
template <typename LogCf>
double lewis_delta_integral(double k, LogCf lnphi)
{
    const auto integrand = [&](double u) {
        return (cplx(0.5, u) * std::exp(lnphi(cplx(u, -0.5)) + cplx(0.0, u * k))).real() / (u * u + 0.25);
    };
    const auto envelope = [&](double u) { return u * std::exp(lnphi(cplx(u, -0.5)).real()) / (u * u + 0.25); };
    double U = kHestonRangeMin;
    while (U < kHestonRangeMax && envelope(U) >= kHestonEnvelope) U *= 2.0;
    double x[kGlNodes], w[kGlNodes];
    gauss_legendre(x, w);
    const int panels = static_cast<int>(U / kHestonPanel);
    double integral = 0.0;
    for (int p = 0; p < panels; ++p) {
        const double mid = (p + 0.5) * kHestonPanel;
        double s = 0.0;
        for (int i = 0; i < kGlNodes; ++i) s += w[i] * integrand(mid + 0.5 * kHestonPanel * x[i]);
        integral += 0.5 * kHestonPanel * s;
    }
    return integral;
}

// d(price) / dS0 of mcamd_heston_price_f64 on arguments it accepts (include/mcamd_heston_greeks.h):
//     delta_call = (D / S0) (F - sqrt(F K) / pi  int Re[(1/2 + iu) e^{iuk} phi(u - i/2)] / (u^2 + 1/4) du),
// the put by parity; below MCAMD_HESTON_XI_MIN the Black-Scholes delta at the average variance.
double heston_delta(double S0, double K, double T, double r, double q, double v0, double kappa, double theta, double xi,
                    double rho, bool call)
{
    const double D = std::exp(-r * T), F = S0 * std::exp((r - q) * T), Dq = std::exp(-q * T);
    if (xi < MCAMD_HESTON_XI_MIN) {
        const double kT = kappa * T;
        const double mean_v = theta + (v0 - theta) * (kT > 0.0 ? -std::expm1(-kT) / kT : 1.0);
        if (!(mean_v > 0.0)) return call ? (F > K ? Dq : 0.0) : (F < K ? -Dq : 0.0);
        const double v = std::sqrt(mean_v), sqrtT = std::sqrt(T);
        const double d1 = (std::log(S0 / K) + (r - q + 0.5 * v * v) * T) / (v * sqrtT);
        return call ? Dq * norm_cdf(d1) : -Dq * norm_cdf(-d1);
    }
    const double k = std::log(F / K);
    const double integral =
        lewis_delta_integral(k, [&](cplx u) { return heston_log_cf(u, T, v0, kappa, theta, xi, rho); });
    const double dc = D / S0 * (F - std::sqrt(F * K) / M_PI * integral);
    return call ? dc : dc - D * F / S0;
}

// (1 - e^{-kappa t}) / kappa, t at kappa = 0
double decay_gain(double kappa, double t)
{
    const double kt = kappa * t;
    return kt > 0.0 ? -std::expm1(-kt) / kappa : t;
}

// ln E[e^{iu x}] of the forward log-return x = ln(S_{t + tau} / S_t) - (r - q) tau under Heston.  Given v_t the return
// over [t, t + tau] has the spot characteristic function exp(C(tau, u) + D(tau, u) v_t), heston_log_cf being affine in
// its v0: C is its value at v0 = 0 and D its value at v0 = 1 with theta = 0.  v_t is a scaled noncentral chi-square:
//     E[e^{w v_t}] = (1 - 2cw)^{-2 kappa theta / xi^2} exp(w v0 e^{-kappa t} / (1 - 2cw)),  c = xi^2 (1 - e^{-kappa t}) / (4 kappa),
// and with z = -2cw the power is exp(-(2 kappa theta / xi^2) ln(1 + z)) = exp(kappa theta [(1 - e^{-kappa t}) / kappa] w
// [ln(1 + z) / z]): the complex logarithm is taken in Kahan's quotient and nothing is divided by xi^2.  Re w <= 0 on
// the lines the callers use, so 1 + z stays in the right half plane and the principal logarithm is the continuous one.
// kappa = 0: c = xi^2 t / 4 and the power is 1.  t = 0: e^{w v0}.
cplx heston_forward_log_cf(cplx u, double t, double tau, double v0, double kappa, double theta, double xi, double rho)
{
    const cplx C = heston_log_cf(u, tau, 0.0, kappa, theta, xi, rho);
    const cplx w = heston_log_cf(u, tau, 1.0, kappa, 0.0, xi, rho);
    if (!(t > 0.0)) return C + w * v0;
    const double gain = decay_gain(kappa, t), c = 0.25 * xi * xi * gain;
    const cplx z = -2.0 * c * w;
    return C + (kappa * theta * gain) * w * c_log1p_over(z) + w * (v0 * std::exp(-kappa * t)) / (1.0 + z);
}

// The step of the two central differences that give the first two cumulants of a period's log-return from
// f = ln phi: with g1(h) = Im f(h) / h = k1 - k3 h^2 / 6 + .. and g2(h) = -2 Re f(h) / h^2 = k2 - k4 h^2 / 12 + ..,
// (4 g(h) - g(2h)) / 3 leaves an error of order h^4 (k5 h^4 / 30, k6 h^4 / 90).  f is evaluated where it is small with
// the relative accuracy of its parts (nothing in heston_log_cf cancels at u -> 0), so rounding costs about eps / h.
constexpr double kCumulantStep = 1.0 / 32.0;

}  // namespace

extern "C" {

int mcamd_bs_greeks_f64(double S0, double K, double T, double r, double v, double out[6])
{
    if (!out) return fail(MCAMD_ERR_INVALID, "out is NULL");
    if (!(S0 > 0.0) || !(K > 0.0) || !(T > 0.0) || !(v > 0.0) || !std::isfinite(S0) || !std::isfinite(K) ||
        !std::isfinite(T) || !std::isfinite(r) || !std::isfinite(v))
        return fail(MCAMD_ERR_INVALID, "closed-form Greeks need finite S0, K, T, v > 0 and a finite r");
    const double sqrtT = std::sqrt(T);
    const double d1 = (std::log(S0 / K) + (r + 0.5 * v * v) * T) / (v * sqrtT);
    const double d2 = d1 - v * sqrtT;
    const double Nd1 = norm_cdf(d1), Nd2 = norm_cdf(d2);
    const double phi = std::exp(-0.5 * d1 * d1) / std::sqrt(2.0 * M_PI);
    const double Kdisc = K * std::exp(-r * T);
    out[MCAMD_GREEK_PRICE] = mcamd_bs_call_f64(S0, K, T, r, v);
    out[MCAMD_GREEK_DELTA] = Nd1;
    out[MCAMD_GREEK_GAMMA] = phi / (S0 * v * sqrtT);
    out[MCAMD_GREEK_VEGA] = S0 * phi * sqrtT;
    out[MCAMD_GREEK_RHO] = Kdisc * T * Nd2;
    out[MCAMD_GREEK_THETA] = -S0 * phi * v / (2.0 * sqrtT) - r * Kdisc * Nd2;
    return MCAMD_OK;
}

// Reiner and Rubinstein (1991) / Merton (1973): the continuously monitored single barrier without rebate or dividends,
// from the four terms A..D of the standard presentation (phi = 1 call / -1 put, eta = 1 down / -1 up).
int mcamd_barrier_price_f64(double S0, double K, double B, double T, double r, double v, int kind, int payoff,
                            double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (!(K > 0.0) || !(T > 0.0) || !(v > 0.0) || !std::isfinite(K) || !std::isfinite(T) || !std::isfinite(r) ||
        !std::isfinite(v))
        return fail(MCAMD_ERR_INVALID, "the barrier closed form needs finite K, T, v > 0 and a finite r");
    if (int rc = check_barrier_kind(S0, B, kind, payoff)) return rc;
    const auto [up, out] = barrier_sides(kind);
    const double phi = payoff == MCAMD_PAYOFF_PUT ? -1.0 : 1.0, eta = up ? -1.0 : 1.0;
    const double s = v * std::sqrt(T), mu = (r - 0.5 * v * v) / (v * v), Kd = K * std::exp(-r * T);
    const auto N = norm_cdf;
    const double x1 = std::log(S0 / K) / s + (1.0 + mu) * s, x2 = std::log(S0 / B) / s + (1.0 + mu) * s;
    const double y1 = std::log(B * B / (S0 * K)) / s + (1.0 + mu) * s, y2 = std::log(B / S0) / s + (1.0 + mu) * s;
    const double p0 = std::pow(B / S0, 2.0 * mu), p1 = p0 * (B / S0) * (B / S0);
    const double tA = phi * S0 * N(phi * x1) - phi * Kd * N(phi * x1 - phi * s);
    const double tB = phi * S0 * N(phi * x2) - phi * Kd * N(phi * x2 - phi * s);
    const double tC = phi * S0 * p1 * N(eta * y1) - phi * Kd * p0 * N(eta * y1 - eta * s);
    const double tD = phi * S0 * p1 * N(eta * y2) - phi * Kd * p0 * N(eta * y2 - eta * s);
    // the knock-in; the knock-out is the vanilla price (term A) less it.  Which combination depends on whether the
    // strike lies on the live side of the barrier for this payoff.
    const bool call = phi > 0.0;
    double in;
    if (call != up) in = (call ? K >= B : K <= B) ? tC : tA - tB + tD;          // down call, up put
    else in = (call ? K >= B : K <= B) ? tA : tB - tC + tD;                     // up call, down put
    *price = out ? tA - in : in;
    return MCAMD_OK;
}

// Goldman, Sosin and Gatto (1979) for the floating strike, Conze and Viswanathan (1991) for the fixed one: the
// continuously monitored, newly issued lookback without dividends.  A fixed strike on the side of the spot the extremum
// has already passed (call: K <= S0, put: K >= S0) is the opposite floating lookback plus a forward.
int mcamd_lookback_price_f64(double S0, double K, double T, double r, double v, int strike, int payoff, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (!(S0 > 0.0) || !(T > 0.0) || !(v > 0.0) || !std::isfinite(S0) || !std::isfinite(T) || !std::isfinite(r) ||
        !std::isfinite(v))
        return fail(MCAMD_ERR_INVALID, "the lookback closed form needs finite S0, T, v > 0 and a finite r");
    if (r == 0.0)
        return fail(MCAMD_ERR_INVALID, "the lookback closed form carries v^2 / (2r): r == 0 is not covered");
    if (int rc = check_lookback_kind(K, strike, payoff)) return rc;
    const bool put = payoff == MCAMD_PAYOFF_PUT;
    const double sq = std::sqrt(T), s = v * sq, D = std::exp(-r * T), G = std::exp(r * T);
    const double lam = v * v / (2.0 * r), shift = 2.0 * r * sq / v;
    const auto N = norm_cdf;
    const double a = (r + 0.5 * v * v) * T / s;
    const auto floating = [&](bool is_put) {
        if (is_put) return S0 * D * N(-a + s) - S0 * N(-a) + S0 * D * lam * (-N(a - shift) + G * N(a));
        return S0 * N(a) - S0 * D * N(a - s) + S0 * D * lam * (N(-a + shift) - G * N(-a));
    };
    if (strike == MCAMD_LOOKBACK_FLOATING) {
        *price = floating(put);
        return MCAMD_OK;
    }
    const double d = (std::log(S0 / K) + (r + 0.5 * v * v) * T) / s;
    const double pw = std::pow(S0 / K, -2.0 * r / (v * v));
    if (!put) {
        if (K > S0) *price = S0 * N(d) - K * D * N(d - s) + S0 * D * lam * (-pw * N(d - shift) + G * N(d));
        else *price = floating(true) + S0 - K * D;
    } else {
        if (K < S0) *price = K * D * N(-d + s) - S0 * N(-d) + S0 * D * lam * (pw * N(-d + shift) - G * N(-d));
        else *price = floating(false) + K * D - S0;
    }
    return MCAMD_OK;
}

// The geometric basket is a lognormal: ln A_T ~ N(m, s^2), m = sum_j w_j (ln S0_j + (r - v_j^2/2) T),
// s^2 = T w'(v o corr o v) w.
int mcamd_basket_geometric_price_f64(const mcamd_basket *basket, double K, double T, double r, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (!basket) return fail(MCAMD_ERR_INVALID, "basket is NULL");
    double L[64];
    if (int rc = check_basket_assets(basket, false, L)) return rc;
    if (!std::isfinite(K) || !(K >= 0.0)) return fail(MCAMD_ERR_INVALID, "a basket option needs a finite K >= 0, got %g", K);
    if (!(T > 0.0) || !std::isfinite(T) || !std::isfinite(r))
        return fail(MCAMD_ERR_INVALID, "the geometric closed form needs a finite T > 0 and a finite r");
    const int d = basket->n_assets;
    double mean = 0.0, var = 0.0;
    for (int j = 0; j < d; ++j) {
        mean += basket->w[j] * (std::log(basket->S0[j]) + (r - 0.5 * basket->v[j] * basket->v[j]) * T);
        for (int k = 0; k < d; ++k)
            var += basket->w[j] * basket->v[j] * basket->corr[8 * j + k] * basket->v[k] * basket->w[k];
    }
    var *= T;
    const double s = std::sqrt(var > 0.0 ? var : 0.0), D = std::exp(-r * T), F = std::exp(mean + 0.5 * var);
    const bool put = basket->payoff == MCAMD_PAYOFF_PUT;
    if (K == 0.0 || !(s > 0.0)) {   // a forward: A_T > 0 = K always, or A_T is not random (weights that cancel)
        const double fwd = K == 0.0 ? F : std::exp(mean);
        *price = D * std::fmax(put ? K - fwd : fwd - K, 0.0);
        return MCAMD_OK;
    }
    const double d1 = (mean - std::log(K)) / s + s, d2 = d1 - s;
    *price = put ? D * (K * norm_cdf(-d2) - F * norm_cdf(-d1)) : D * (F * norm_cdf(d1) - K * norm_cdf(d2));
    return MCAMD_OK;
}

// Margrabe (1978): the option to exchange b S2 for a S1.
int mcamd_exchange_price_f64(double a_S1, double b_S2, double T, double v1, double v2, double rho, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (!(a_S1 > 0.0) || !(b_S2 > 0.0) || !(T > 0.0) || !(v1 > 0.0) || !(v2 > 0.0) || !std::isfinite(a_S1) ||
        !std::isfinite(b_S2) || !std::isfinite(T) || !std::isfinite(v1) || !std::isfinite(v2))
        return fail(MCAMD_ERR_INVALID, "the exchange closed form needs finite a S1, b S2, T, v1, v2 > 0");
    if (!(rho > -1.0 && rho < 1.0))
        return fail(MCAMD_ERR_INVALID, "the exchange closed form needs -1 < rho < 1, got %g", rho);
    const double s = std::sqrt((v1 * v1 + v2 * v2 - 2.0 * rho * v1 * v2) * T);
    const double d1 = std::log(a_S1 / b_S2) / s + 0.5 * s;
    *price = a_S1 * norm_cdf(d1) - b_S2 * norm_cdf(d1 - s);
    return MCAMD_OK;
}

int mcamd_asian_geometric_price_f64(double S0, double K, double T, double r, double v, uint32_t n_steps,
                                    int include_spot, int strike, int payoff, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    return asian_geometric_price(S0, K, T, r, v, n_steps, include_spot, strike, payoff, price);
}

// One asset, one date: S_T / S_0 is lognormal, P[S_T / S_0 >= x] = N(d2(x)) and E[(S_T / S_0) 1{S_T / S_0 <= x}] =
// e^{rT} N(-d1(x)).  Called above L: 1 + c; between B and L: 1; at or below B: the performance itself (B <= 1).
int mcamd_autocall_single_date_price_f64(double T, double r, double v, double call_level, double coupon,
                                         double ki_level, int ki_monitoring, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (!(T > 0.0) || !(v > 0.0) || !std::isfinite(T) || !std::isfinite(r) || !std::isfinite(v))
        return fail(MCAMD_ERR_INVALID, "the single-date autocall closed form needs finite T, v > 0 and a finite r");
    if (int rc = check_autocall_terms(coupon, call_level, 0.0, call_level, ki_monitoring, ki_level)) return rc;
    if (ki_monitoring == MCAMD_AUTOCALL_KI_EVERY_STEP)
        return fail(MCAMD_ERR_INVALID, "the closed form covers MCAMD_AUTOCALL_KI_NONE and MCAMD_AUTOCALL_KI_AT_MATURITY: "
                                       "a knock-in monitored at every step has none");
    const double s = v * std::sqrt(T);
    const auto d2 = [&](double x) { return (-std::log(x) + (r - 0.5 * v * v) * T) / s; };
    const double pL = norm_cdf(d2(call_level));
    double value = (1.0 + coupon) * pL;
    if (ki_monitoring == MCAMD_AUTOCALL_KI_NONE) value += 1.0 - pL;
    else value += (norm_cdf(d2(ki_level)) - pL) + std::exp(r * T) * norm_cdf(-(d2(ki_level) + s));
    *price = std::exp(-r * T) * value;
    return MCAMD_OK;
}

// Volatility in time only: the period log-returns D_p ~ N((r - q - v_p^2 / 2) tau, v_p^2 tau) are independent, so the
// mean of a sum of clipped returns is the sum of the means and that of their product the product.  A return clipped to
// [F, C] is (1 + F) + (e^D - (1 + F))+ - (e^D - (1 + C))+ gross: two calls on e^D.
int mcamd_cliquet_price_f64(int kind, double T, double r, double q, uint32_t n_periods, uint32_t first_period,
                            const double *period_vol, double local_floor, double local_cap, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (!period_vol) return fail(MCAMD_ERR_INVALID, "period_vol is NULL");
    if (int rc = check_cliquet_kind(kind)) return rc;
    if (int rc = check_cliquet_local(local_floor, local_cap)) return rc;
    if (int rc = check_cliquet_kind_bounds(kind, local_floor, local_cap)) return rc;
    if (!(T > 0.0) || !std::isfinite(T) || !std::isfinite(r) || !std::isfinite(q))
        return fail(MCAMD_ERR_INVALID, "the cliquet closed form needs a finite T > 0 and finite r and q");
    if (n_periods == 0 || first_period < 1 || first_period > n_periods)
        return fail(MCAMD_ERR_INVALID, "n_periods must be >= 1 and first_period 1..n_periods, got %u and %u", n_periods,
                    first_period);
    for (uint32_t p = 0; p < n_periods; ++p)
        if (!std::isfinite(period_vol[p]) || !(period_vol[p] > 0.0))
            return fail(MCAMD_ERR_INVALID, "every period volatility must be finite and > 0: period_vol[%u] = %g", p,
                        period_vol[p]);
    const double tau = T / static_cast<double>(n_periods), fwd = std::exp((r - q) * tau);
    const double F = std::fmax(local_floor, -1.0);   // a floor at or below -1 never binds
    double sum = 0.0, prod = 1.0;
    for (uint32_t p = first_period; p <= n_periods; ++p) {
        const double v = period_vol[p - 1], s = v * std::sqrt(tau);
        const auto call = [&](double k) {   // E[(e^D - k)+]
            if (k <= 0.0) return fwd - k;
            if (k == HUGE_VAL) return 0.0;
            const double d1 = ((r - q + 0.5 * v * v) * tau - std::log(k)) / s;
            return fwd * norm_cdf(d1) - k * norm_cdf(d1 - s);
        };
        if (kind == MCAMD_CLIQUET_VARIANCE) {
            const double mean = (r - q - 0.5 * v * v) * tau;
            sum += v * v * tau + mean * mean;
        } else {
            const double E = (1.0 + F) + call(1.0 + F) - call(1.0 + local_cap);
            sum += E - 1.0;
            prod *= E;
        }
    }
    const double P = static_cast<double>(n_periods - first_period + 1);
    const double value = kind == MCAMD_CLIQUET_SUM ? sum : kind == MCAMD_CLIQUET_COMPOUND ? prod - 1.0 : sum / (P * tau);
    *price = std::exp(-r * T) * value;
    return MCAMD_OK;
}

int mcamd_localvol_sigma_f64(const mcamd_localvol_grid *grid, const double *h_sigma, uint32_t n_steps, uint32_t step,
                             double x, double *sigma)
{
    if (!sigma) return fail(MCAMD_ERR_INVALID, "sigma is NULL");
    *sigma = 0.0;
    if (int rc = check_localvol_grid(grid, h_sigma, nullptr)) return rc;
    if (n_steps == 0 || step >= n_steps)
        return fail(MCAMD_ERR_INVALID, "step = %u must lie in [0, n_steps = %u)", step, n_steps);
    if (std::isnan(x)) return fail(MCAMD_ERR_INVALID, "x is NaN");
    const uint64_t row = static_cast<uint64_t>(step) * grid->n_t / n_steps;
    const double dx = (grid->x_max - grid->x_min) / static_cast<double>(grid->n_x - 1);
    const double u = std::fmin(std::fmax((x - grid->x_min) * (1.0 / dx), 0.0), static_cast<double>(grid->n_x - 1));
    const uint32_t k = std::min(static_cast<uint32_t>(u), grid->n_x - 2);
    const double *s = h_sigma + row * grid->n_x + k;
    *sigma = std::fma(u - static_cast<double>(k), s[1] - s[0], s[0]);
    return MCAMD_OK;
}

int mcamd_bs_price_f64(double S0, double K, double T, double r, double q, double v, int payoff, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (!(S0 > 0.0) || !(K > 0.0) || !(T > 0.0) || !(v > 0.0) || !std::isfinite(S0) || !std::isfinite(K) ||
        !std::isfinite(T) || !std::isfinite(v) || !std::isfinite(r) || !std::isfinite(q))
        return fail(MCAMD_ERR_INVALID, "Black-Scholes needs finite S0, K, T, v > 0 and finite r, q");
    if (int rc = check_payoff(payoff)) return rc;
    const double sqrtT = std::sqrt(T);
    const double d1 = (std::log(S0 / K) + (r - q + 0.5 * v * v) * T) / (v * sqrtT), d2 = d1 - v * sqrtT;
    const double Sd = S0 * std::exp(-q * T), Kd = K * std::exp(-r * T);
    *price = payoff == MCAMD_PAYOFF_CALL ? Sd * norm_cdf(d1) - Kd * norm_cdf(d2) : Kd * norm_cdf(-d2) - Sd * norm_cdf(-d1);
    return MCAMD_OK;
}

// Lewis's single integral on the line Im u = -1/2, where the integrand has no pole and decays fastest:
//     call = D (F - sqrt(F K) / pi  int_0^inf Re[e^{iuk} phi(u - i/2)] / (u^2 + 1/4) du),  k = ln(F / K).
int mcamd_heston_price_f64(double S0, double K, double T, double r, double q, double v0, double kappa, double theta,
                           double xi, double rho, int payoff, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (int rc = check_payoff(payoff)) return rc;
    if (int rc = check_heston_model(q, v0, kappa, theta, xi, rho)) return rc;
    if (!(S0 > 0.0) || !(K > 0.0) || !(T > 0.0) || !std::isfinite(S0) || !std::isfinite(K) || !std::isfinite(T) ||
        !std::isfinite(r))
        return fail(MCAMD_ERR_INVALID, "the Heston closed form needs finite S0, K, T > 0 and a finite r");
    const bool call = payoff == MCAMD_PAYOFF_CALL;
    const double D = std::exp(-r * T), F = S0 * std::exp((r - q) * T);
    if (xi < MCAMD_HESTON_XI_MIN) {
        // v is deterministic: Black-Scholes at the average variance theta + (v0 - theta)(1 - e^{-kappa T}) / (kappa T)
        const double kT = kappa * T;
        const double mean_v = theta + (v0 - theta) * (kT > 0.0 ? -std::expm1(-kT) / kT : 1.0);
        *price = mean_v > 0.0 ? bs_value(S0, K, T, r, q, std::sqrt(mean_v), call, nullptr)
                              : D * std::fmax(call ? F - K : K - F, 0.0);
        return MCAMD_OK;
    }
    const double k = std::log(F / K);
    const double integral =
        lewis_integral(k, [&](cplx u) { return heston_log_cf(u, T, v0, kappa, theta, xi, rho); });
    const double c = D * (F - std::sqrt(F * K) / M_PI * integral);
    if (!std::isfinite(c)) return fail(MCAMD_ERR_INVALID, "the Heston integral is not finite at these parameters");
    *price = call ? c : c - D * (F - K);
    return MCAMD_OK;
}

// The model's values of what mcamd_price_heston_greeks estimates (include/mcamd_heston_greeks.h).
int mcamd_heston_greeks_f64(double S0, double K, double T, double r, double q, double v0, double kappa, double theta,
                            double xi, double rho, int payoff, double gamma_eta, const double bump[5], double out[10])
{
    if (out)
        for (int k = 0; k < MCAMD_HESTON_GREEKS; ++k) out[k] = 0.0;
    if (!bump || !out) return fail(MCAMD_ERR_INVALID, "bump and out must be non-NULL");
    double price = 0.0;
    if (int rc = mcamd_heston_price_f64(S0, K, T, r, q, v0, kappa, theta, xi, rho, payoff, &price)) return rc;
    if (!std::isfinite(gamma_eta) || gamma_eta < 0.0)
        return fail(MCAMD_ERR_INVALID, "gamma_eta must be finite and >= 0 (0: no gamma), got %g", gamma_eta);
    for (int k = 0; k < 5; ++k)
        if (!std::isfinite(bump[k]) || bump[k] < 0.0)
            return fail(MCAMD_ERR_INVALID, "bump[%d] must be finite and >= 0 (0: not requested), got %g", k, bump[k]);
    const bool call = payoff == MCAMD_PAYOFF_CALL;
    const double delta = heston_delta(S0, K, T, r, q, v0, kappa, theta, xi, rho, call);
    if (!std::isfinite(delta)) return fail(MCAMD_ERR_INVALID, "the Heston integral is not finite at these parameters");
    double values[MCAMD_HESTON_GREEKS] = {};
    values[MCAMD_HESTON_GREEK_PRICE] = price;
    values[MCAMD_HESTON_GREEK_DELTA] = delta;
    if (gamma_eta > 0.0) {
        const double up = std::exp(gamma_eta), dn = std::exp(-gamma_eta);
        const double d_up = heston_delta(S0 * up, K, T, r, q, v0, kappa, theta, xi, rho, call);
        const double d_dn = heston_delta(S0 * dn, K, T, r, q, v0, kappa, theta, xi, rho, call);
        values[MCAMD_HESTON_GREEK_GAMMA] = (d_up - d_dn) / (S0 * (up - dn));
    }
    values[MCAMD_HESTON_GREEK_RHO] = T * (S0 * delta - price);
    values[MCAMD_HESTON_GREEK_RHO_Q] = -T * S0 * delta;
    for (int k = 0; k < 5; ++k) {
        if (!(bump[k] > 0.0)) continue;
        double side[2];
        for (int s = 0; s < 2; ++s) {
            double p[5] = {v0, kappa, theta, xi, rho};
            p[k] = p[k] + (s == 0 ? bump[k] : -bump[k]);
            if (int rc = mcamd_heston_price_f64(S0, K, T, r, q, p[0], p[1], p[2], p[3], p[4], payoff, &side[s])) return rc;
        }
        values[MCAMD_HESTON_GREEK_V0 + k] = (side[0] - side[1]) / (2.0 * bump[k]);
    }
    for (int k = 0; k < MCAMD_HESTON_GREEKS; ++k) out[k] = values[k];
    return MCAMD_OK;
}

// The forward characteristic function (heston_forward_log_cf) carries the additive cliquet and the variance swap:
// expectations add over dependent periods.
int mcamd_heston_cliquet_price_f64(int kind, double T, double r, double q, double v0, double kappa, double theta,
                                   double xi, double rho, uint32_t n_periods, uint32_t first_period,
                                   double local_floor, double local_cap, double *price)
{
    if (!price) return fail(MCAMD_ERR_INVALID, "price is NULL");
    *price = 0.0;
    if (int rc = check_cliquet_kind(kind)) return rc;
    if (int rc = check_cliquet_local(local_floor, local_cap)) return rc;
    if (int rc = check_cliquet_kind_bounds(kind, local_floor, local_cap)) return rc;
    if (int rc = check_heston_model(q, v0, kappa, theta, xi, rho)) return rc;
    if (!(T > 0.0) || !std::isfinite(T) || !std::isfinite(r))
        return fail(MCAMD_ERR_INVALID, "the Heston cliquet closed form needs a finite T > 0 and a finite r");
    if (n_periods == 0 || first_period < 1 || first_period > n_periods)
        return fail(MCAMD_ERR_INVALID, "n_periods must be >= 1 and first_period 1..n_periods, got %u and %u", n_periods,
                    first_period);
    const double tau = T / static_cast<double>(n_periods);
    if (xi < MCAMD_HESTON_XI_MIN) {
        // v is deterministic: the periods are independent, at the rms volatility of each
        std::vector<double> vol(n_periods);
        for (uint32_t p = 0; p < n_periods; ++p)
            vol[p] = std::sqrt(theta + (v0 - theta) * std::exp(-kappa * (p * tau)) * (decay_gain(kappa, tau) / tau));
        return mcamd_cliquet_price_f64(kind, T, r, q, n_periods, first_period, vol.data(), local_floor, local_cap, price);
    }
    if (kind == MCAMD_CLIQUET_COMPOUND) {
        if (first_period != n_periods)
            return fail(MCAMD_ERR_INVALID, "a compounding cliquet over %u periods has no closed form under Heston: the "
                                           "periods depend on each other through v, so the mean of their product is not "
                                           "the product of their means (one counted period, or xi < %g, is served)",
                        n_periods - first_period + 1, MCAMD_HESTON_XI_MIN);
        kind = MCAMD_CLIQUET_SUM;   // one period: e^{l} - 1 is the clipped return itself
    }
    const double fwd = std::exp((r - q) * tau);
    const double F = std::fmax(local_floor, -1.0);   // a floor at or below -1 never binds
    double sum = 0.0;
    for (uint32_t p = first_period; p <= n_periods; ++p) {
        const double t = (p - 1) * tau;
        const auto lnphi = [&](cplx u) { return heston_forward_log_cf(u, t, tau, v0, kappa, theta, xi, rho); };
        if (kind == MCAMD_CLIQUET_VARIANCE) {
            const auto cumulants = [&](double h, double *k1, double *k2) {
                const cplx f = lnphi(cplx(h, 0.0));
                *k1 = f.imag() / h + (r - q) * tau;
                *k2 = -2.0 * f.real() / (h * h);
            };
            double a1, a2, b1, b2;
            cumulants(kCumulantStep, &a1, &a2);
            cumulants(2.0 * kCumulantStep, &b1, &b2);
            const double k1 = (4.0 * a1 - b1) / 3.0, k2 = (4.0 * a2 - b2) / 3.0;
            sum += k2 + k1 * k1;
        } else {
            // kappa theta = 0: zero absorbs the variance, and a path that enters the period there earns the forward
            // exactly.  That mass, lim_{w -> -inf} M_t(w) = exp(-v0 e^{-kappa t} / (2c)), keeps the characteristic
            // function from decaying; its call is (fwd - k)+ and the integral takes the rest, which decays.
            const double c = 0.25 * xi * xi * decay_gain(kappa, t);
            const double atom = (kappa * theta == 0.0 && c > 0.0) ? std::exp(-v0 * std::exp(-kappa * t) / (2.0 * c)) : 0.0;
            const auto call = [&](double k) {   // E[(e^D - k)+]
                if (k <= 0.0) return fwd - k;
                if (k == HUGE_VAL) return 0.0;
                return fwd - atom * std::fmin(fwd, k) -
                       std::sqrt(fwd * k) / M_PI * lewis_integral(std::log(fwd / k), lnphi, atom);
            };
            sum += (1.0 + F) + call(1.0 + F) - call(1.0 + local_cap) - 1.0;
        }
    }
    if (!std::isfinite(sum)) return fail(MCAMD_ERR_INVALID, "the Heston integral is not finite at these parameters");
    const double P = static_cast<double>(n_periods - first_period + 1);
    *price = std::exp(-r * T) * (kind == MCAMD_CLIQUET_VARIANCE ? sum / (P * tau) : sum);
    return MCAMD_OK;
}

int mcamd_bs_implied_vol_f64(double S0, double K, double T, double r, double q, int payoff, double price, double *vol)
{
    if (!vol) return fail(MCAMD_ERR_INVALID, "vol is NULL");
    *vol = std::nan("");
    if (!(S0 > 0.0) || !(K > 0.0) || !(T > 0.0) || !std::isfinite(S0) || !std::isfinite(K) || !std::isfinite(T) ||
        !std::isfinite(r) || !std::isfinite(q) || !std::isfinite(price))
        return fail(MCAMD_ERR_INVALID, "an implied volatility needs finite S0, K, T > 0 and finite r, q and price");
    if (int rc = check_payoff(payoff)) return rc;
    const bool call = payoff == MCAMD_PAYOFF_CALL;
    const double D = std::exp(-r * T), F = S0 * std::exp((r - q) * T);
    const double lower = D * std::fmax(call ? F - K : K - F, 0.0);
    const double upper = call ? S0 * std::exp(-q * T) : K * D;
    if (!(price > lower) || !(price < upper))
        return fail(MCAMD_ERR_INVALID, "the price %.17g is not strictly inside the no-arbitrage bounds (%.17g, %.17g)", price,
                    lower, upper);
    // The price grows with v from lower to upper: bracket the root, then Newton steps kept inside the bracket and
    // replaced by a bisection whenever they leave it or shrink it too slowly (plain Newton diverges in the wings,
    // where the vega vanishes).  f is "not above" at lo and "above or equal" at hi throughout; a NaN counts as not above.
    double lo = 0.0, hi = 1.0 / std::sqrt(T);
    for (int grow = 0; grow < 64 && !(bs_value(S0, K, T, r, q, hi, call, nullptr) >= price); ++grow) {
        lo = hi;
        hi *= 2.0;
    }
    double x = 0.5 * (lo + hi), dx_old = hi - lo, dx = dx_old, vega = 0.0;
    double f = bs_value(S0, K, T, r, q, x, call, &vega) - price;
    for (int it = 0; it < 400; ++it) {
        const bool newton_leaves = !(((x - hi) * vega - f) * ((x - lo) * vega - f) < 0.0);
        const bool newton_slow = !(std::fabs(2.0 * f) <= std::fabs(dx_old * vega));
        dx_old = dx;
        if (newton_leaves || newton_slow) {
            dx = 0.5 * (hi - lo);
            x = lo + dx;
        } else {
            dx = f / vega;
            x -= dx;
        }
        if (!(std::fabs(dx) > 1e-15 * x)) break;
        f = bs_value(S0, K, T, r, q, x, call, &vega) - price;
        if (f >= 0.0) hi = x;
        else lo = x;
        if (f == 0.0) break;
    }
    *vol = x;
    return MCAMD_OK;
}

// Closed form, host.  Same operation order and the same mixed precision as the reference:
// `0.5 * v * v` and `exp(-r * T)` are evaluated in double and narrowed (inc/BlackandScholes.hpp:37,42).
float mcamd_cnd_f32(float x)
{
    const float p = 0.2316419f;
    const float b1 = 0.31938153f, b2 = -0.356563782f, b3 = 1.781477937f, b4 = -1.821255978f, b5 = 1.330274429f;
    const float one_over_sqrt_twopi = 0.39894228f;
    const float t = 1.0f / (1.0f + p * std::fabs(x));
    const float tail = one_over_sqrt_twopi * expf(-x * x / 2.0f) * t * (t * (t * (t * (t * b5 + b4) + b3) + b2) + b1);
    return x >= 0.0f ? 1.0f - tail : tail;
}

float mcamd_bs_call_f32(float x0, float strike, float T, float r, float sigma)
{
    const float sqrtT = sqrtf(T);
    const float d1 = static_cast<float>(
        (static_cast<double>(logf(x0 / strike)) + (static_cast<double>(r) + 0.5 * sigma * sigma) * T) /
        static_cast<double>(sigma * sqrtT));
    const float d2 = d1 - sigma * sqrtT;
    const float n1 = mcamd_cnd_f32(d1), n2 = mcamd_cnd_f32(d2);
    return static_cast<float>(static_cast<double>(x0 * n1) -
                              static_cast<double>(strike) * std::exp(static_cast<double>(-r * T)) * n2);
}

double mcamd_bs_call_f64(double x0, double strike, double T, double r, double sigma)
{
    const double sqrtT = std::sqrt(T);
    const double d1 = (std::log(x0 / strike) + (r + 0.5 * sigma * sigma) * T) / (sigma * sqrtT);
    const double d2 = d1 - sigma * sqrtT;
    return x0 * norm_cdf(d1) - strike * std::exp(-r * T) * norm_cdf(d2);
}

}  // extern "C"
