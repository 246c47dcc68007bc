// host_neg2log_masked_exponent_check.cpp — CPU check that f64::neg2log_1k (csrc/fast64.hpp), which forms its exponent
// term from the masked word k 2^20 and the constant kM2Ln2 2^-20, returns the bits of the formula it replaced, which
// shifted k out of the word and multiplied by kM2Ln2.  Compiled with g++ and run by
// tests/test_neg2log_masked_exponent.py; prints one JSON line of counts.
//
//   host_neg2log_masked_exponent_check [n_random]
#include "fast64.hpp"

#define MCAMD_TAB_DECL static const
#include "tables64.inc"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace mcamd::f64;

static const D2 *const kTab1k = reinterpret_cast<const D2 *>(kLogTab1k);

static uint64_t bits_of(double x)
{
    uint64_t b;
    std::memcpy(&b, &x, 8);
    return b;
}

// The formula before the change, kept as a plain reference: k by an arithmetic shift, converted, times -2 ln 2.
static double neg2log_1k_shifted(double u, const D2 *tab1k)
{
    const uint32_t hx = hi32(u);
    const uint32_t tmp = hx - 0x3fe60000u;
    const int32_t k = static_cast<int32_t>(tmp) >> 20;
    const double z = make_double(lo32(u), hx - (tmp & 0xfff00000u));
    const D2 e = *reinterpret_cast<const D2 *>(reinterpret_cast<const char *>(tab1k) + ((tmp >> 6) & 0x3ff0u));
    const double t = std::fma(z, e.a, 2.0);
    const double w = std::fma(static_cast<double>(k), kM2Ln2, e.b);
    double q = std::fma(t, 1.0 / 32.0, 1.0 / 12.0);
    q = std::fma(t, q, 0.25);
    const double h = std::fma(t, q, 1.0);
    return std::fma(t, h, w);
}

struct Count {
    long terms = 0, term_mismatch = 0;   // exponent x row
    long args = 0, arg_mismatch = 0;     // arguments u
    long boundaries = 0;
    int saw_one = 0, saw_smallest = 0;
    double first_bad = 0;
};

static void check_u(Count &c, double u)
{
    ++c.args;
    if (u == 1.0) c.saw_one = 1;
    if (u == 0x1p-53) c.saw_smallest = 1;
    if (bits_of(neg2log_1k(u, kTab1k)) != bits_of(neg2log_1k_shifted(u, kTab1k))) {
        if (!c.arg_mismatch) c.first_bad = u;
        ++c.arg_mismatch;
    }
}

int main(int argc, char **argv)
{
    const long n = argc > 1 ? std::atol(argv[1]) : 4000000;
    Count c;
    // every exponent the reduction can meet (u = 2^k z, z in [0.6875, 1.375), u in [2^-53, 1]) against every row
    for (int k = -53; k <= 0; ++k)
        for (int i = 0; i < MCAMD_LOG1K_N; ++i) {
            const uint32_t k20 = static_cast<uint32_t>(k) << 20;    // what tmp & 0xfff00000 holds
            const double got = neg2log_1k_exponent_term(k20, kTab1k[i].b);
            const double want = std::fma(static_cast<double>(k), kM2Ln2, kTab1k[i].b);
            ++c.terms;
            c.term_mismatch += bits_of(got) != bits_of(want);
        }
    // the uniforms the kernels draw, u = (v + 1) 2^-53: random v, an eighth of them spread over the small exponents
    std::mt19937_64 gen(20261021);
    for (long j = 0; j < n; ++j) {
        uint64_t v = gen() >> 11;
        if (j % 8 == 0) v >>= gen() % 53;
        check_u(c, std::fma(static_cast<double>(v), 0x1p-53, 0x1p-53));
    }
    check_u(c, 1.0);
    check_u(c, 0x1p-53);
    // every chunk boundary +- 3 ulp at every exponent: z = 0.6875 + i 2^-10 steps of the bit pattern, u = 2^k z
    for (int k = -53; k <= 0; ++k)
        for (uint64_t i = 0; i <= 1024; ++i) {
            const uint64_t zb = 0x3FE6000000000000ull + (i << 42);
            double z;
            std::memcpy(&z, &zb, 8);
            const double ub = std::ldexp(z, k);
            for (int d = -3; d <= 3; ++d) {
                uint64_t b = bits_of(ub) + static_cast<uint64_t>(static_cast<int64_t>(d));
                double u;
                std::memcpy(&u, &b, 8);
                if (!(u >= 0x1p-53 && u <= 1.0)) continue;
                ++c.boundaries;
                check_u(c, u);
            }
        }
    std::printf("{\"terms\": %ld, \"term_mismatch\": %ld, \"args\": %ld, \"arg_mismatch\": %ld, \"boundaries\": %ld, "
                "\"saw_one\": %d, \"saw_smallest\": %d, \"first_bad\": %.17g}\n",
                c.terms, c.term_mismatch, c.args, c.arg_mismatch, c.boundaries, c.saw_one, c.saw_smallest, c.first_bad);
    return 0;
}
