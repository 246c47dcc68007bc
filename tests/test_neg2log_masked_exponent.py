"""CPU test that f64::neg2log_1k (csrc/fast64.hpp) kept its bits when its exponent term changed form.

The function writes u = 2^k z and needs w = k (-2 ln 2) + b, b from the table row.  It used to shift k out of the word
tmp = hi32(u) - 0x3fe60000 (an arithmetic shift by 20), convert it and multiply by kM2Ln2.  It now converts the word it
masks for z anyway, tmp & 0xfff00000 = k 2^20 as an int32, and multiplies by kM2Ln2 2^-20.  Both scalings are exact
powers of two (|k 2^20| < 2^26 is exact in a double, kM2Ln2 2^-20 is far from underflow), so the product is the same
real number and the fma rounds to the same bits — for every input, not to a tolerance.  Checked by
tests/host_neg2log_masked_exponent_check.cpp on the host build of the header (plain g++, as tests/test_neg2log_1k.py
builds its checker):
  * the term itself for every exponent k in [-53, 0] against every one of the 1024 rows;
  * the whole function against the earlier formula, kept in the checker as a plain reference, on 4e6 uniforms
    (v + 1) 2^-53, on u = 1 and u = 2^-53, and on all 1025 chunk boundaries +- 3 ulp at every exponent."""
import json
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "monte-carlo-project-cuda_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host_neg2log_masked_exponent_check.cpp")


def run(tmp_path, n, extra=("-O2",)):
    exe = os.path.join(str(tmp_path), "n1kmasked")
    subprocess.check_call(["g++", *extra, "-std=c++17", "-ffp-contract=off", "-I" + CSRC, SRC, "-o", exe])
    r = json.loads(subprocess.check_output([exe, str(n)]))
    print(json.dumps(r))
    return r


def test_exponent_term_and_function_keep_their_bits(tmp_path):
    r = run(tmp_path, 4_000_000)
    assert r["terms"] == 54 * 1024 and r["term_mismatch"] == 0
    assert r["saw_one"] == 1 and r["saw_smallest"] == 1
    assert r["boundaries"] > 300_000                     # 54 exponents x 1025 boundaries x 7, less those outside [2^-53, 1]
    assert r["args"] >= 4_000_000 + 2 + r["boundaries"]
    assert r["arg_mismatch"] == 0, r["first_bad"]


def test_checker_is_clean_under_asan_ubsan(tmp_path):
    # the same stand-alone program under the host sanitizers (the shift of a negative exponent is done on unsigned words)
    r = run(tmp_path, 200_000, extra=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert r["term_mismatch"] == 0 and r["arg_mismatch"] == 0
