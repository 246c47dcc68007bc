/* mcamd_heston_greeks.h — Greeks of a European option under Heston stochastic volatility, from ONE simulation.
 *
 * A public header of its own beside mcamd.h, which it includes.  Additive to ABI version 5: first carried by the build
 * that ships csrc/heston_greeks.hip (no struct or function of mcamd.h changed, so MCAMD_ABI_VERSION stays 5; a caller
 * finds out with dlsym).  The same library carries these functions.
 *
 * ---- What is estimated, and how ----
 * The paths are mcamd_price_heston's (mcamd.h: model, scheme, draws, step, the exponential that ends a path).  One call
 * returns price, delta, gamma, rho (d / dr), rho_q (d / dq) and the sensitivities to v0, kappa, theta, xi and the
 * model's correlation rho, where eleven calls of mcamd_price_heston would walk nearly the same paths eleven times and
 * make the same Philox blocks and Box-Muller fills eleven times.
 *   Spot and rates: pathwise, from the ONE base walk.  X = ln(S / S0) does not depend on S0, so S_T is homogeneous in
 *       S0; every step adds (r - q) dt to X, so dX_n / dr = T and dX_n / dq = -T exactly.  With sgn = +1 for a call and
 *       -1 for a put and d = sgn S_T 1{h > 0}:  d(payoff) / dS0 = d / S0,  d / dr of the discounted payoff =
 *       e^{-rT} T (d - y),  d / dq = -e^{-rT} T d.
 *   Gamma: the central difference of the pathwise delta in the log-spot over a half-width eta = gamma_eta,
 *       (Delta(S0 e^{eta}) - Delta(S0 e^{-eta})) / (S0 (e^{eta} - e^{-eta})), read off the same S_T: by homogeneity the
 *       path from S0 e^{+-eta} ends at S_T e^{+-eta}.
 *   Model parameters: NOT a tangent recurrence.  The tangent of s = sqrt(v+) is 1 / (2 s), the scheme visits v+ = 0 on
 *       everyday inputs (a model that fails Feller's condition is truncated most of the time), E[1 / v+] then diverges,
 *       and a tangent estimator has no finite variance: its standard error would mean nothing.  They are central
 *       differences on common random numbers instead: each requested parameter p gets two more (X, v) walks inside the
 *       same kernel, one at p + bump and one at p - bump, on the SAME z and z' of every step.  Each bumped walk is, by
 *       construction, mcamd_price_heston's path at the bumped parameter, bit for bit.
 *
 * ---- Definitions ----
 *   Walks.  Walk 0 is the base walk.  Then, for each requested parameter (bump[k] > 0) in the index order v0, kappa,
 *       theta, xi, rho, a "+" walk at the parameter + bump[k] and a "-" walk at the parameter - bump[k]; P is the number
 *       of requested parameters, 1 + 2 P the number of walks.  The bumped value is formed in double on the host.  Each
 *       walk's step constants (kappa dt, kappa theta dt, xi sqrt(dt), rho, sqrt(1 - rho^2)) and its v0 are formed from
 *       the walk's own model exactly as mcamd_price_heston forms them (in double, narrowed once); nothing is derived
 *       from the base walk's constants.  (r - q) dt, dt / 2 and sqrt(dt) do not depend on the model: the same bits in
 *       every walk.
 *   Draws.  z and z' of mcamd_price_heston, made ONCE per path and step block; every walk of the path takes them.
 *   Per step, every walk w by mcamd_price_heston's step, fused operation for fused operation:
 *       v+ = max(v_w, 0),  s = sqrt(v+),  w' = fma(rho_w, z, sqrt(1 - rho_w^2) z')
 *       X_w += fma(s sqrt(dt), z, fma(-v+, dt / 2, (r - q) dt))
 *       v_w += fma(s (xi_w sqrt(dt)), w', fma(-v+, kappa_w dt, kappa_w theta_w dt)).
 *   Per path, after the loop, in the path precision (u = e^{eta} and ui = e^{-eta} are formed in double and narrowed
 *   once; each product is ONE multiply, fused with nothing):
 *       row 0:  h  = max(+-(S_T - K), 0) at the base walk's S_T = S0 e^{X_0}: mcamd_price_heston's sample
 *       row 1:  d  = sgn S_T where h > 0, else 0
 *       row 2:  g  = sgn S_T ([payoff(S_T u) > 0] - [payoff(S_T ui) > 0]),  payoff(s) = max(+-(s - K), 0):
 *                    S_T or 0, never negative; all zeros when gamma_eta = 0
 *       rows 3 + 2 j, 4 + 2 j:  h+ and h- of the j-th requested parameter: max(+-(S0 e^{X_w} - K), 0) of its two walks,
 *                    by the same exponential and payoff as row 0.
 *   In fp64, from the widened rows:  y = h;  e = d - y (one subtraction);  c_j = h+ - h- (one subtraction).
 *       The rho sample is T e and the rho_q sample -T d; the factors are applied when the record is finalized.
 *   trunc and rv: the base walk's, as mcamd_price_heston defines them.
 *
 * ---- The record ----
 * 9 + 2 P doubles, summed by the kernel in one fixed order, then n, then zeros up to MCAMD_HESTON_GREEKS_STATS = 32:
 *       [0] sum y      [1] sum y^2    [2] sum d      [3] sum d^2    [4] sum e^2    [5] sum g      [6] sum g^2
 *       [7 + 2 j] sum c_j   [8 + 2 j] sum c_j^2                       j = 0 .. P - 1, the requested parameters in order
 *       [7 + 2 P] sum trunc (the base walk's truncated steps)
 *       [8 + 2 P] sum rv    (the base walk's sum of the paths' average variance)
 *       [9 + 2 P] n         (the paths of the shard)
 *       [10 + 2 P .. 32)  0
 * sum e = [2] - [0].  A sample depends on its global path id alone, so shards of ONE job (same P) add element by
 * element and one all-reduce of the 32 doubles serves multi-GPU use.  One launch, one fixed order of summation: two
 * runs of one job give the same bits.  Every square is fma(x, x, acc).
 *
 * ---- Finalize (mcamd_finalize_heston_greeks_stats; the synchronous call does the same) ----
 * With D = e^{-rT}, N = n, mean(s) = s / N and se(s, ss) = sqrt(max((ss - N mean^2) / (N - 1), 0) / N) as
 * mcamd_finalize computes it (0 for N < 2):
 *       price = D mean([0])                      se = D se([0], [1])
 *       delta = D mean([2]) / S0                 se = D se([2], [3]) / S0
 *       gamma = D mean([5]) / (S0^2 (e^{eta} - e^{-eta}))      se likewise from ([5], [6]);  0 and 0 when gamma_eta = 0
 *       rho   = T D mean([2] - [0])              se = T D se([2] - [0], [4])
 *       rho_q = -T D mean([2])                   se = T D se([2], [3])
 *       parameter k = D mean([7 + 2 j]) / (2 bump[k])          se = D se([7 + 2 j], [8 + 2 j]) / (2 bump[k])
 * A value that was not requested is 0 with standard error 0.  truncated_steps = [7 + 2 P], mean_variance =
 * [8 + 2 P] / N.  mcamd_finalize_heston_greeks_stats reads S0, T and r of opt and gamma_eta and bump of job; it leaves
 * work_steps, the timings and the launch shape 0.  It refuses NULL pointers, what the pricing call refuses of the job
 * alone, S0 <= 0 and a non-finite S0, T or r.
 *
 * ---- Outputs ----
 * d_samples (nullable, device): (3 + 2 P) n_paths_local values of the path precision, row-major in the order above:
 * [row n_paths_local + local path].
 * out: value and std_err indexed MCAMD_HESTON_GREEK_*; n; truncated_steps, mean_variance and work_steps as
 * mcamd_heston_result.  On a grid of up to 256 workgroups (65536 paths) the block records are added in
 * mcamd_price_heston's order, and price, its standard error, truncated_steps and mean_variance are that call's bits;
 * beyond, the last workgroup adds the block records in ONE sweep where mcamd_price_heston takes four interleaved ones,
 * and the last bits may differ.
 * The enqueue form leaves the 32-double record in d_stats (device) in stream order; mcamd_enqueued_kernel_ms covers it.
 * An empty shard returns zeros and launches nothing; its enqueue form writes a zero record in stream order.
 *
 * ---- Refusals (MCAMD_ERR_INVALID before any device work and before the context is looked at, in this order) ----
 * out (d_stats in the enqueue form, once the context is there) NULL; everything mcamd_price_heston refuses of opt, sim
 * and heston, in its order; job NULL; job->reserved != 0; gamma_eta negative or not finite; a bump negative or not
 * finite; then, for each requested parameter in order, the "+" and the "-" model as mcamd_price_heston refuses a model
 * (v0 - bump >= 0, kappa - bump >= 0, theta - bump >= 0, xi - bump >= 0, |rho +- bump| <= 1), the message naming the
 * parameter; then the context.
 *
 * ---- Closed form (mcamd_heston_greeks_f64) ----
 * out[10], indexed MCAMD_HESTON_GREEK_*, of the MODEL (not of the scheme, which approaches it at first order in dt):
 *       price: mcamd_heston_price_f64.
 *       delta: analytic, by differentiating the Lewis integral under the integral sign.  With F = S0 e^{(r - q) T},
 *              k = ln(F / K) and D = e^{-rT}, d / dS0 of sqrt(F K) e^{iuk} is sqrt(F K) (1/2 + iu) e^{iuk} / S0, so
 *                  delta_call = (D / S0) (F - sqrt(F K) / pi  int_0^U Re[(1/2 + iu) e^{iuk} phi(u - i/2)] / (u^2 + 1/4) du)
 *              by the quadrature rule of mcamd_heston_price_f64, its truncation envelope multiplied by U (the factor
 *              |1/2 + iu| the integrand gains);  delta_put = delta_call - e^{-qT}.  Below xi = MCAMD_HESTON_XI_MIN the
 *              Black-Scholes delta with dividend yield at the average variance (the step function of the forward where
 *              that variance is 0).
 *       gamma: (delta(S0 e^{eta}) - delta(S0 e^{-eta})) / (S0 (e^{eta} - e^{-eta})), the finite difference the kernel
 *              estimates; 0 at gamma_eta = 0.
 *       rho = T (S0 delta - price),  rho_q = -T S0 delta  (the price is homogeneous of degree one in (S0, K) and
 *              depends on r and q through D and F alone).
 *       v0, kappa, theta, xi, rho of the model: (price(p + bump) - price(p - bump)) / (2 bump) of
 *              mcamd_heston_price_f64, exactly that expression; 0 where the bump is 0.
 * Refuses what mcamd_heston_price_f64 refuses, NULL bump or out, a negative or non-finite gamma_eta or bump, and a
 * bumped model that mcamd_heston_price_f64 refuses.
 *
 * Left out on purpose: theta (the time decay); Greeks of the smile, cliquet and barrier calls; second-order parameter
 * sensitivities; a mcamd_group_* form and a shim name. */
#ifndef MCAMD_HESTON_GREEKS_H
#define MCAMD_HESTON_GREEKS_H

#include "mcamd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCAMD_HESTON_GREEK_PRICE 0
#define MCAMD_HESTON_GREEK_DELTA 1
#define MCAMD_HESTON_GREEK_GAMMA 2
#define MCAMD_HESTON_GREEK_RHO   3   /* d / dr */
#define MCAMD_HESTON_GREEK_RHO_Q 4   /* d / dq */
#define MCAMD_HESTON_GREEK_V0    5
#define MCAMD_HESTON_GREEK_KAPPA 6
#define MCAMD_HESTON_GREEK_THETA 7
#define MCAMD_HESTON_GREEK_XI    8
#define MCAMD_HESTON_GREEK_CORR  9   /* d / d(rho of the model) */
#define MCAMD_HESTON_GREEKS 10
#define MCAMD_HESTON_GREEKS_STATS 32

typedef struct mcamd_heston_greeks_job {   /* 56 bytes */
    double gamma_eta;        /* 0: no gamma; else the log-spot half-width, > 0 */
    double bump[5];          /* absolute half-widths for v0, kappa, theta, xi, rho; 0 = not requested, else > 0 */
    double reserved;         /* must be 0 */
} mcamd_heston_greeks_job;

typedef struct mcamd_heston_greeks {   /* 208 bytes */
    double value[10];        /* indexed MCAMD_HESTON_GREEK_* */
    double std_err[10];
    uint64_t n;              /* paths */
    double truncated_steps;  /* the base walk's lane-steps entered with v < 0 */
    double mean_variance;    /* mean over the shard of the base walk's average variance */
    double work_steps;       /* 64 x the steps each wavefront ran: always the full count */
    float kernel_ms;         /* HIP-event time of the kernel (it finishes its own sum: the whole call's device work) */
    float total_ms;
    uint32_t grid;           /* launch shape the engine chose */
    uint32_t block;
} mcamd_heston_greeks;

int mcamd_price_heston_greeks(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim, const mcamd_heston *heston,
                              const mcamd_heston_greeks_job *job, void *d_samples, mcamd_heston_greeks *out);
int mcamd_price_heston_greeks_enqueue(mcamd_ctx *ctx, const mcamd_option *opt, const mcamd_sim *sim,
                                      const mcamd_heston *heston, const mcamd_heston_greeks_job *job, void *d_samples,
                                      double *d_stats);
int mcamd_finalize_heston_greeks_stats(const double stats[32], const mcamd_option *opt,
                                       const mcamd_heston_greeks_job *job, mcamd_heston_greeks *out);
int mcamd_heston_greeks_f64(double S0, double K, double T, double r, double q, double v0, double kappa, double theta,
                            double xi, double rho, int payoff, double gamma_eta, const double bump[5], double out[10]);

#ifdef __cplusplus
}
#endif

#endif /* MCAMD_HESTON_GREEKS_H */
