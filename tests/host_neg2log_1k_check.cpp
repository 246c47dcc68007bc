// host_neg2log_1k_check.cpp — CPU unit test of f64::neg2log_1k (csrc/fast64.hpp), the six-operation -2 ln u of the
// pair-sum loops, on its 1024-entry table: compiled with g++ and run by tests/test_neg2log_1k.py.  Prints one JSON
// line with the worst errors against long-double libm.  Errors as tests/host_fast64_check.cpp defines them.
//
//   host_neg2log_1k_check [n_random]             the accuracy sweep
//   host_neg2log_1k_check --eval IN OUT          IN: raw little-endian doubles u; OUT: neg2log_1k(u) for each, raw
//                                                doubles (what tests/test_gpu_neg2log_1k.py compares the device with)
#include "fast64.hpp"

#define MCAMD_TAB_DECL static const
#include "tables64.inc"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace mcamd::f64;

static const D2 *const kTab1k = reinterpret_cast<const D2 *>(kLogTab1k);
static const long double PI = 3.14159265358979323846264338327950288L;
static const long double SQ2 = 1.41421356237309504880168872420969808L;

static double ulp_err(double got, long double want)
{
    int e;
    std::frexp(static_cast<double>(want), &e);
    const long double ulp = std::ldexp(1.0L, e - 53);
    return static_cast<double>(fabsl(static_cast<long double>(got) - want) / ulp);
}

struct Worst {
    long n = 0;
    double nonpositive = 0;   // inputs with a result that is not > 0
    double ulp = 0;           // u <= 1 - 2^-9: error of -2 ln u in ulp
    double near_one_abs = 0;  // 1 - 2^-9 < u < 1: absolute error
    double radius_rel = 0;    // sqrt_unclamped(a) against sqrt(-2 ln u), relative to 1 + r
    double pair_rel = 0;      // sqrt_unclamped(a) sin_bits_rotated sqrt 2 against r (sin + cos), relative to 1 + r
    double a_at_one = -1;     // the result at u = 1
    double radius_at_one = -1;
    double pair_at_one = 0;   // largest |pair sum| seen at u = 1, in units of sqrt 2 (as PairSum<double> holds it)
};

static D2 g_rot[MCAMD_TAB_N];

// one argument u in [2^-53, 1] with the angle words (z, w)
static void check_u(Worst &W, double u, uint32_t z, uint32_t w)
{
    const double a = neg2log_1k(u, kTab1k);
    ++W.n;
    if (!(a > 0.0)) { W.nonpositive += 1; return; }
    const double r = sqrt_unclamped(a);
    const double rs = sin_bits_rotated<false>(z, w, g_rot, nullptr);
    if (u == 1.0) {
        W.a_at_one = a;
        W.radius_at_one = r;
        if (std::fabs(r * rs) > W.pair_at_one) W.pair_at_one = std::fabs(r * rs);
        return;
    }
    const long double want_a = -2.0L * logl(static_cast<long double>(u));
    if (u <= 1.0 - 0x1p-9) {
        const double e = ulp_err(a, want_a);
        if (e > W.ulp) W.ulp = e;
    } else {
        const double e = static_cast<double>(fabsl(static_cast<long double>(a) - want_a));
        if (e > W.near_one_abs) W.near_one_abs = e;
    }
    const long double want_r = sqrtl(want_a);
    const double er = static_cast<double>(fabsl(static_cast<long double>(r) - want_r) / (1.0L + want_r));
    if (er > W.radius_rel) W.radius_rel = er;
    const uint64_t v2 = static_cast<uint64_t>(z) ^ (static_cast<uint64_t>(w) << 21);
    const long double ang = PI * static_cast<long double>(std::fma(static_cast<double>(v2), 0x1p-52, 0x1p-52));
    const long double want = want_r * (sinl(ang) + cosl(ang));
    const double ep = static_cast<double>(fabsl(static_cast<long double>(r * rs) * SQ2 - want) / (1.0L + want_r));
    if (ep > W.pair_rel) W.pair_rel = ep;
}

// the uniform the kernels draw from v: u = (v + 1) 2^-53
static void check(Worst &W, uint64_t v, uint32_t z, uint32_t w)
{
    check_u(W, std::fma(static_cast<double>(v), 0x1p-53, 0x1p-53), z, w);
}

static int eval_file(const char *in, const char *out)
{
    std::FILE *f = std::fopen(in, "rb");
    if (!f) return 2;
    std::vector<double> u;
    double buf[4096];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), 4096, f)) > 0) u.insert(u.end(), buf, buf + got);
    std::fclose(f);
    for (double &x : u) x = neg2log_1k(x, kTab1k);
    f = std::fopen(out, "wb");
    if (!f) return 2;
    const size_t put = std::fwrite(u.data(), sizeof(double), u.size(), f);
    return (std::fclose(f) == 0 && put == u.size()) ? 0 : 2;
}

int main(int argc, char **argv)
{
    if (argc == 4 && std::strcmp(argv[1], "--eval") == 0) return eval_file(argv[2], argv[3]);
    const long n = argc > 1 ? std::atol(argv[1]) : 8000000;
    for (int i = 0; i < MCAMD_TAB_N; ++i) {   // the sin/cos table as MathCtx<double>::init<true>() copies it
        const int j = (i + MCAMD_TAB_N / 8) & (MCAMD_TAB_N - 1);
        g_rot[i] = D2{kSinCosTab[j][0], kSinCosTab[j][1]};
    }
    std::mt19937_64 gen(20261020);
    Worst W;
    // random u over the whole range
    for (long i = 0; i < n; ++i) {
        const uint64_t b = gen();
        check(W, gen() >> 11, static_cast<uint32_t>(b), static_cast<uint32_t>(b >> 32));
    }
    // per leading exponent: u in [2^-e, 2^-(e-1)), e = 1 .. 53, i.e. v + 1 in [2^(53-e), 2^(54-e))
    const long per_exp = n / 40;
    for (int e = 1; e <= 53; ++e) {
        const uint64_t lo = uint64_t(1) << (53 - e);
        for (long i = 0; i < per_exp; ++i) {
            const uint64_t b = gen();
            check(W, lo + (lo > 1 ? gen() % lo : 0) - 1, static_cast<uint32_t>(b), static_cast<uint32_t>(b >> 32));
        }
    }
    // the values below 1, one by one: u = 1 - j 2^-53, j = 0 .. n/2 (j = 0 is u = 1)
    for (long j = 0; j <= n / 2; ++j) {
        const uint64_t b = gen();
        check(W, (uint64_t(1) << 53) - 1 - static_cast<uint64_t>(j), static_cast<uint32_t>(b), static_cast<uint32_t>(b >> 32));
    }
    // u = 1 with the angles at which the pair sum is largest (rotated sine = +-1) and a sweep of arcs; u = 2^-53
    for (uint32_t w = 0; w < 4096; ++w) check(W, (uint64_t(1) << 53) - 1, 0x9e3779b9u * w, w << 20);
    check(W, 0, 1u, 2u);
    // every chunk boundary +- 3 ulp at every exponent: z = 0.6875 + i 2^-10 steps of the bit pattern, u = 2^k z
    for (int k = -53; k <= 0; ++k)
        for (uint64_t i = 0; i <= 1024; ++i) {
            uint64_t zb = 0x3FE6000000000000ull + (i << 42);
            double z;
            std::memcpy(&z, &zb, 8);
            const double ub = std::ldexp(z, k);
            for (int d = -3; d <= 3; ++d) {
                uint64_t bits;
                std::memcpy(&bits, &ub, 8);
                bits += static_cast<uint64_t>(static_cast<int64_t>(d));
                double u;
                std::memcpy(&u, &bits, 8);
                if (!(u >= 0x1p-53 && u <= 1.0)) continue;
                const uint64_t b = gen();   // below 1/2 these are off the kernels' 2^-53 grid: the function holds there too
                check_u(W, u, static_cast<uint32_t>(b), static_cast<uint32_t>(b >> 32));
            }
        }
    std::printf("{\"n\": %ld, \"nonpositive\": %g, \"ulp\": %.3f, \"near_one_abs\": %.3g, \"radius_rel\": %.3g, "
                "\"pair_sum_rel\": %.3g, \"a_at_one\": %.17g, \"radius_at_one\": %.17g, \"pair_at_one\": %.17g}\n",
                W.n, W.nonpositive, W.ulp, W.near_one_abs, W.radius_rel, W.pair_rel, W.a_at_one, W.radius_at_one,
                W.pair_at_one);
    return 0;
}
