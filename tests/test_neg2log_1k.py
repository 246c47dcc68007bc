"""CPU unit test of f64::neg2log_1k (csrc/fast64.hpp): -2 ln u in six fp64 operations on a 1024-entry table, used by
the pair-sum loops only (csrc/mc_device.hpp PairSum<double>).  The header compiles with plain g++, so the function is
pinned against long-double libm without a GPU (tests/host_neg2log_1k_check.cpp): 8e6 random uniforms, 2e5 per leading
exponent, the 4e6 uniforms below 1 one by one, u = 1, u = 2^-53, and all 1024 chunk boundaries +- 3 ulp at every
exponent.

Bounds, with where each comes from:
  ULP             the project's bound for -2 ln u (tests/fast64_bounds.py NEG2LOG_ULP), for u <= 1 - 2^-9.
  NEAR_ONE_ABS    above that the series' dropped term t^5/80, |t| < 2^-10, is up to 1.1e-17 absolute — ~100 ulp of a
                  result below 2e-3 — so the bound there is absolute: 2.5e-17.  It is what the radius carries into a
                  path's sum.
  RADIUS_REL      sqrt(a) against sqrt(-2 ln u), relative to 1 + r: 3e-16 (1.74e-16 in a prototype of this form, with
                  room for the rounding of the table rows).
  PAIR_SUM_REL    the whole pair sum, the project's existing bound (tests/fast64_bounds.py).
  At u = 1 the table row is biased so that the result is positive; the radius there is at most sqrt(bias)."""
import json
import math
import subprocess

import pytest

import fast64_bounds as bd
import neg2log_1k_harness as h

ULP = bd.NEG2LOG_ULP
NEAR_ONE_ABS = 2.5e-17
RADIUS_REL = 3e-16


def check(r):
    print(json.dumps(r))
    assert r["nonpositive"] == 0                       # a > 0 for every input: the radius needs no clamp
    assert r["ulp"] <= ULP
    assert r["near_one_abs"] <= NEAR_ONE_ABS
    assert r["radius_rel"] <= RADIUS_REL
    assert r["pair_sum_rel"] <= bd.PAIR_SUM_REL
    assert 0.0 < r["a_at_one"] <= h.BIAS_1K
    assert 0.0 < r["radius_at_one"] <= math.sqrt(h.BIAS_1K)
    assert 0.0 < r["pair_at_one"] <= r["radius_at_one"]   # in units of sqrt 2, as PairSum<double> holds it


def test_neg2log_1k_accuracy_against_long_double_libm(tmp_path):
    exe = h.compile_host(tmp_path)
    check(json.loads(subprocess.check_output([exe, "8000000"])))


def test_neg2log_1k_clean_under_asan_ubsan(tmp_path):
    # the same stand-alone checker under the host sanitizers
    exe = h.compile_host(tmp_path, extra=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    check(json.loads(subprocess.check_output([exe, "400000"])))


def test_tables_hold_the_1k_log_table_the_generator_writes():
    mp = pytest.importorskip("mpmath")
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("gen_tables64", os.path.join(h.ROOT, "tools", "gen_tables64.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    assert g.BIAS_1K == h.BIAS_1K
    rows = g.log_table_1k()          # asserts the bias against its own evaluation of the chain at u = 1
    text = open(os.path.join(h.CSRC, "tables64.inc")).read()
    body = text.split("kLogTab1k[MCAMD_LOG1K_N][2]")[1].split("};")[0]
    got = [tuple(float.fromhex(x.strip()) for x in ln.strip(" {},\n").split(",")) for ln in body.splitlines()[1:] if "{" in ln]
    assert got == rows and len(rows) == 1024


def test_device_harness_compiles_with_the_library_flags(tmp_path):
    # so that a header change that breaks tests/neg2log_1k_check.hip shows on every CPU run
    h.load_device(h.compile_device(tmp_path))
    u = h.device_inputs()
    assert u.size == 1 << 16 and u.min() == 2.0 ** -53 and u.max() == 1.0
