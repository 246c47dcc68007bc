"""CPU unit test of the hand-written fp64 math the kernels use (csrc/fast64.hpp): the header also
compiles with plain g++, so its accuracy is pinned against long-double libm without a GPU."""
import json
import os
import subprocess

from conftest import ROOT
import fast64_bounds as bd


def test_fast64_accuracy_against_long_double_libm(tmp_path):
    exe = tmp_path / "f64check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "monte-carlo-project-cuda_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_fast64_check.cpp"), "-o", str(exe)])
    r = json.loads(subprocess.check_output([str(exe), "2000000"]))
    assert r["uniform_mismatch"] == 0          # u and the angle are bit-identical to rocRAND's construction
    assert r["neg2log_ulp"] <= bd.NEG2LOG_ULP
    assert r["sqrt_ulp"] <= bd.SQRT_POS_ULP
    assert r["sqrt_scaled_ulp"] <= bd.SQRT_SCALED_ULP  # k sqrt(a) in six operations (one cubic step)
    assert r["neg2log_nonpositive"] == 0                 # -2 ln u > 0 for every u in (0, 1]: the radius needs no clamp
    assert r["sin_abs"] <= bd.SINCOS_ABS and r["cos_abs"] <= bd.SINCOS_ABS
    # the pair-sum loop of the window-less pricing kernel (mc_device.hpp PairSum): sqrt in five operations, the sine of
    # the angle rotated by pi/4 from the rotated table, and a whole pair sum r sqrt2 sin(a + pi/4) against z0 + z1
    assert r["sqrt_unclamped_ulp"] <= bd.SQRT_UNCLAMPED_ULP
    assert r["sin_rotated_abs"] <= bd.SINCOS_ABS and r["cos_rotated_abs"] <= bd.SINCOS_ABS
    assert r["pair_sum_rel"] <= bd.PAIR_SUM_REL
    assert r["mul_exp_ulp"] <= bd.MUL_EXP_ULP  # one factor S e^x, |x| <= 1: 2 table entries + 3 multiplies
    assert r["mul_exp_wide_ulp_per_unit_x"] <= bd.MUL_EXP_WIDE_ULP_PER_UNIT_X  # |x| up to 300: the error grows with the exponent's own ulp
    assert r["product252_ulp"] <= bd.PRODUCT252_ULP  # 252-factor recurrence: rounding random-walks as sqrt(n)
    # cheap barrier test: |k + (P - 1) kappa - log2(prod) 65536| as a fraction of the band that defers to the exact test
    assert 0.0 < r["barrier_band_used"] < 1.0


def test_tables_are_reproducible_from_the_generator():
    # the committed tables are what tools/gen_tables64.py writes (needs mpmath; skip without it)
    import pytest
    pytest.importorskip("mpmath")
    inc = os.path.join(ROOT, "monte-carlo-project-cuda_amd", "csrc", "tables64.inc")
    before = open(inc).read()
    subprocess.check_call(["python3", os.path.join(ROOT, "tools", "gen_tables64.py")], stdout=subprocess.DEVNULL)
    assert open(inc).read() == before


def test_fast64_clean_under_asan_ubsan(tmp_path):
    # host-side sanitizer run of the same header (GPU sanitizers are not available on the pool)
    exe = tmp_path / "f64check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "monte-carlo-project-cuda_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_fast64_check.cpp"), "-o", str(exe)])
    r = json.loads(subprocess.check_output([str(exe), "200000"]))
    assert r["uniform_mismatch"] == 0 and r["neg2log_ulp"] <= bd.NEG2LOG_ULP
