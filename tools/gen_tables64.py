#!/usr/bin/env python3
"""Generates monte-carlo-project-cuda_amd/csrc/tables64.inc: the lookup tables of the hand-written fp64
math used by the pricing kernels (fast64.hpp).  Build-time tool (needs mpmath); the generated file is
committed, so neither the library nor the tests depend on mpmath.

  LOG    512 x (-2/c_i, -2 ln c_i)      -2 ln(z) = -2 ln c_i + g(t), t = fma(z, -2/c_i, 2), |t| < 2^-9
  SINCOS 512 x (sin, cos)(2 pi (j + 1/2)/512)   nodes at the arc midpoints (fast64.hpp sincos_bits)
  LOG1K  1024 x (-2/c_i, -2 ln c_i)     the same with |t| < 2^-10, for the pair-sum kernels (fast64.hpp neg2log_1k)
  EXP_HI 256 x 2^(i/256),  EXP_LO 256 x 2^(i/65536)   two-level table of 2^(k/65536) (fast64.hpp ExpAcc)
(20 KB in all: 512 entries keep the log / sin / cos polynomials at degree <= 4)
Table layout follows the standard "reduce with a small table, finish with a short polynomial" scheme
(the same idea as in widely used libm implementations); the entries are computed here from scratch
with 60-digit arithmetic.
"""
import os
import struct

import mpmath as mp

mp.mp.dps = 60
N = 512
LOGB = 9  # log2(N)
OFF = 0x3FE6000000000000  # 0.6875: z is normalised to [0.6875, 1.375)


def dbl(x) -> float:
    return float(mp.mpf(x))  # mpmath rounds to nearest double


def as_double(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def hexf(x: float) -> str:
    return float(x).hex()


def log_table():
    rows = []
    for i in range(N):
        lo = as_double(OFF + (i << (52 - LOGB)))
        hi = as_double(OFF + ((i + 1) << (52 - LOGB)))
        if hi == 1.0:
            # chunk [1 - 2^-10, 1): c = 1 exactly, so -2 ln(u) keeps full relative accuracy as u -> 1-
            invc = 1.0
        else:
            c = (mp.mpf(lo) + mp.mpf(hi)) / 2
            invc = dbl(1 / c)
        # c is DEFINED as the exact reciprocal of the rounded invc, so ln c below matches fma(z, invc, -1)
        logc = mp.log(1 / mp.mpf(invc)) if invc != 1.0 else mp.mpf(0)
        rows.append((-2.0 * invc, dbl(-2 * logc)))
    # u = 1 (z = 1.0 exactly, k = 0) lands at the bottom of the chunk that starts at 1.0; there -2 ln c_i and the
    # polynomial cancel to 0 +- 4e-19.  Bias that one entry by +4e-18 so that neg2log(u) > 0 for EVERY u in (0, 1]
    # and the Box-Muller radius needs no clamp in front of its reciprocal square root.  Everywhere else in that chunk
    # (u in [2^k, ...), k <= -1) the result is >= 1.38, where 4e-18 is 1/50 ulp.
    i_one = (0x3FF0000000000000 - OFF) >> (52 - LOGB)
    a, b = rows[i_one]
    rows[i_one] = (a, b + 4e-18)
    return rows


N1K = 1024
LOGB1K = 10
# What neg2log_1k returns at u = 1 without a bias is its truncation: the chain stops at t^4/32, and the dropped
# t^5/80 (t = 2 - 2/c of the chunk [1, 1 + 2^-10), 9.76e-4) leaves -1.108e-17 there.  log_table_1k() evaluates the
# chain operation by operation, as the device does (every step is one fma, so the bits are the device's), and asserts
# what the bias has to give: a result at u = 1 that is strictly positive, and small enough that the largest pair sum
# there, sqrt(2 a), stays within the 3e-9 the device tests allow at u = 1.  1.55e-17 leaves a = 4.4e-18 (radius
# 2.1e-9; the 512-entry table's 4e-18 leaves 3.6e-18).  Everywhere else in that chunk the result is >= 1.38, where
# the bias is 1/14 ulp.
BIAS_1K = 1.55e-17


def fma(a: float, b: float, c: float) -> float:
    return dbl(mp.mpf(a) * mp.mpf(b) + mp.mpf(c))  # the 60-digit sum is exact, so this rounds once


def neg2log_1k_of_one(row) -> float:
    """fast64.hpp neg2log_1k at u = 1 (z = 1, k = 0) on the table row that serves it, operation by operation."""
    a, b = row
    t = fma(1.0, a, 2.0)
    q = fma(t, 1.0 / 32.0, 1.0 / 12.0)
    q = fma(t, q, 0.25)
    h = fma(t, q, 1.0)
    return fma(t, h, b)


def log_table_1k():
    """The 1024-entry table of the pair-sum kernels (fast64.hpp neg2log_1k): built as log_table() builds the
    512-entry one, |t| < 2^-10, so that -2 ln(1 - t/2) can stop at t^4/32 (t^5/80 < 1.1e-17 absolute)."""
    rows = []
    for i in range(N1K):
        lo = as_double(OFF + (i << (52 - LOGB1K)))
        hi = as_double(OFF + ((i + 1) << (52 - LOGB1K)))
        if hi == 1.0:
            invc = 1.0  # chunk [1 - 2^-11, 1): c = 1 exactly
        else:
            c = (mp.mpf(lo) + mp.mpf(hi)) / 2
            invc = dbl(1 / c)
        logc = mp.log(1 / mp.mpf(invc)) if invc != 1.0 else mp.mpf(0)
        rows.append((-2.0 * invc, dbl(-2 * logc)))
    i_one = (0x3FF0000000000000 - OFF) >> (52 - LOGB1K)
    cancel = neg2log_1k_of_one(rows[i_one])
    assert abs(cancel) < BIAS_1K <= 5e-17, cancel
    a, b = rows[i_one]
    rows[i_one] = (a, b + BIAS_1K)
    at_one = neg2log_1k_of_one(rows[i_one])
    assert 0.0 < at_one <= BIAS_1K and (2 * at_one) ** 0.5 <= 3e-9, at_one
    return rows


def main():
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "monte-carlo-project-cuda_amd",
                       "csrc", "tables64.inc")
    L = log_table()
    SC = [(dbl(mp.sin(2 * mp.pi * (j + mp.mpf(1) / 2) / N)), dbl(mp.cos(2 * mp.pi * (j + mp.mpf(1) / 2) / N)))
          for j in range(N)]
    EXH = [dbl(mp.power(2, mp.mpf(i) / 256)) for i in range(256)]
    EXL = [dbl(mp.power(2, mp.mpf(i) / 65536)) for i in range(256)]
    with open(out, "w") as f:
        f.write("// tables64.inc — GENERATED by tools/gen_tables64.py (mpmath, 60 digits). Do not edit.\n")
        f.write("// clang-format off\n")
        f.write(f"#define MCAMD_TAB_N {N}\n")
        f.write("MCAMD_TAB_DECL double kLogTab[MCAMD_TAB_N][2] = {  // {-2/c_i, -2 ln c_i}\n")
        for a, b in L:
            f.write(f"    {{{hexf(a)}, {hexf(b)}}},\n")
        f.write("};\nMCAMD_TAB_DECL double kSinCosTab[MCAMD_TAB_N][2] = {  // {sin, cos}(2 pi (j + 1/2) / N)\n")
        for a, b in SC:
            f.write(f"    {{{hexf(a)}, {hexf(b)}}},\n")
        f.write("};\nMCAMD_TAB_DECL double kExpHiTab[256] = {  // 2^(i/256)\n")
        for a in EXH:
            f.write(f"    {hexf(a)},\n")
        f.write("};\nMCAMD_TAB_DECL double kExpLoTab[256] = {  // 2^(i/65536)\n")
        for a in EXL:
            f.write(f"    {hexf(a)},\n")
        f.write("};\n")
        f.write(f"#define MCAMD_LOG1K_N {N1K}\n")
        f.write("MCAMD_TAB_DECL double kLogTab1k[MCAMD_LOG1K_N][2] = {  // {-2/c_i, -2 ln c_i}, 1024 chunks\n")
        for a, b in log_table_1k():
            f.write(f"    {{{hexf(a)}, {hexf(b)}}},\n")
        f.write("};\n")
        f.write("// clang-format on\n")
    c1 = mp.log(2) / 65536
    consts = {
        "kM2Ln2": dbl(-2 * mp.log(2)),                 # -2 ln 2
        "kExpScale": dbl(65536 / mp.log(2)),           # exponent units of ExpAcc: y = x * 65536 / ln 2
        "kExpC1": dbl(c1),                             # e^(rr c1) - 1 = rr (c1 + c2 rr), |rr| <= 1/2
        "kExpC2": dbl(c1 * c1 / 2),
        # sin / cos of d = f kappa, kappa = 2 pi / N, as polynomials in f (fast64.hpp sincos_bits)
        "kSinF1": dbl(2 * mp.pi / N),
        "kSinF3": dbl(-(2 * mp.pi / N) ** 3 / 6),
        "kSinF5": dbl((2 * mp.pi / N) ** 5 / 120),
        "kCosF2": dbl(-(2 * mp.pi / N) ** 2 / 2),
        "kCosF4": dbl((2 * mp.pi / N) ** 4 / 24),
    }
    with open(out.replace("tables64.inc", "tables64_consts.inc"), "w") as f:
        f.write("// tables64_consts.inc — GENERATED by tools/gen_tables64.py. Do not edit.\n// clang-format off\n")
        for k, v in consts.items():
            f.write(f"static constexpr double {k} = {hexf(v)};\n")
        f.write("// clang-format on\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
