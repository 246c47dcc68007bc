"""Builds the two programs the neg2log_1k tests run: tests/host_neg2log_1k_check.cpp with g++ (the host build of
csrc/fast64.hpp, as tests/test_fast64.py builds its checker) and tests/neg2log_1k_check.hip with the library's own
compile flags (as tests/device_math_harness.py builds its harness)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "monte-carlo-project-cuda_amd", "csrc")
HOST_SRC = os.path.join(ROOT, "tests", "host_neg2log_1k_check.cpp")
DEVICE_SRC = os.path.join(ROOT, "tests", "neg2log_1k_check.hip")
BIAS_1K = 1.55e-17      # tools/gen_tables64.py: what the row that serves u = 1 is raised by


def compile_host(out_dir, extra=("-O2",)) -> str:
    exe = os.path.join(str(out_dir), "n1kcheck")
    subprocess.check_call(["g++", *extra, "-std=c++17", "-ffp-contract=off", "-I" + CSRC, HOST_SRC, "-o", exe])
    return exe


def host_eval(exe: str, u: np.ndarray, work_dir) -> np.ndarray:
    """neg2log_1k(u) of the host build, element by element."""
    fin, fout = os.path.join(str(work_dir), "u.f64"), os.path.join(str(work_dir), "a.f64")
    np.ascontiguousarray(u, dtype="<f8").tofile(fin)
    subprocess.check_call([exe, "--eval", fin, fout])
    return np.fromfile(fout, dtype="<f8")


def compile_device(out_dir) -> str:
    bmod = importlib.import_module("monte-carlo-project-cuda_amd.build")
    so = os.path.join(str(out_dir), "libneg2log1kcheck.so")
    subprocess.check_call([bmod.hipcc(), *bmod._flags(), "-shared", DEVICE_SRC, "-o", so])
    return so


def load_device(so: str):
    L = C.CDLL(so)
    L.n1k_eval.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p]
    return L


def chunk_boundaries(k: int) -> np.ndarray:
    """u = 2^k z for the 1025 chunk boundaries z = 0.6875 .. 1.375 of the 1024-entry table, each +- 3 ulp, kept where
    2^-53 <= u <= 1."""
    zb = np.uint64(0x3FE6000000000000) + (np.arange(1025, dtype=np.uint64) << np.uint64(42))
    ub = np.ldexp(zb.view(np.float64), k).view(np.uint64)
    u = (ub[:, None] + np.arange(-3, 4, dtype=np.int64).astype(np.uint64)[None, :]).ravel().view(np.float64)
    return u[(u >= 2.0 ** -53) & (u <= 1.0)]


def device_inputs(n: int = 1 << 16, seed: int = 20261020) -> np.ndarray:
    """n arguments: u = 1, u = 2^-53, every chunk boundary +- 3 ulp in the top binades (k = 0, -1: all 1024 chunks) and
    at every thirteenth exponent below, the 4096 uniforms next to 1, and random uniforms (v + 1) 2^-53 for the rest."""
    edges = [np.array([1.0, 2.0 ** -53])] + [chunk_boundaries(k) for k in (0, -1, -13, -26, -39, -52)]
    edges.append(1.0 - np.arange(4096) * 2.0 ** -53)
    e = np.unique(np.concatenate(edges))
    assert e.size < n
    r = np.random.default_rng(seed)
    v = r.integers(0, 1 << 53, size=n - e.size, dtype=np.uint64)
    small = (np.arange(v.size) % 8 == 0)       # an eighth of them spread over the small exponents
    v[small] >>= r.integers(0, 53, size=int(small.sum()), dtype=np.uint64)
    u = np.concatenate([e, (v.astype(np.float64) + 1.0) * 2.0 ** -53])   # v < 2^53: v + 1 exact except at 2^53 - 1 -> 1.0
    return u
