"""Accuracy bounds of the hand-written fp64 math (csrc/fast64.hpp, csrc/mc_device.hpp PairSum), shared by the host
check (tests/test_fast64.py: the header compiled with g++) and the device check (tests/test_gpu_device_math.py: the
same functions compiled for gfx950 with the library's flags).  Errors as tests/host_fast64_check.cpp defines them:
ulp of the fp64 result against an extended-precision reference; absolute for sin / cos; the pair sum relative to
1 + r (r the Box-Muller radius)."""

NEG2LOG_ULP = 2.0              # -2 ln u, u in [2^-53, 1]
SQRT_POS_ULP = 1.0             # sqrt_pos: seed + coupled Newton step + correction
SQRT_UNCLAMPED_ULP = 2.0       # sqrt_unclamped: one cubic step on the v_rsq_f64 seed, five operations
SQRT_SCALED_ULP = 2.0          # k sqrt(a), the same step and the scaling in six operations
SINCOS_ABS = 2.5e-16           # sincos_bits and sin_bits_rotated, both outputs
PAIR_SUM_REL = 6e-16           # a whole pair sum r (sin a + cos a), and the single normals, relative to 1 + r
MUL_EXP_ULP = 4.5              # one factor S e^x, |x| <= 1
MUL_EXP_WIDE_ULP_PER_UNIT_X = 3.5   # |x| up to 300: the error grows with the exponent's own ulp
PRODUCT252_ULP = 64.0          # 252-factor running product: rounding random-walks as sqrt(n)
F32_NORMAL_ABS = 4e-6          # fp32 Box-Muller normal (hardware v_log / v_sqrt / v_sin / v_cos), per normal
