"""Builds tests/american_solve_check.hip (the solver / decision harness of the American pricer) with the library's own
compile flags, so the harness runs am_solve, am_exercise and am_continuation as american.hip compiles them: -O3, the
same includes, hipcc's contraction default for .hip sources."""
import ctypes as C
import importlib
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "american_solve_check.hip")


def compile_harness(out_dir) -> str:
    bmod = importlib.import_module("monte-carlo-project-cuda_amd.build")
    so = os.path.join(str(out_dir), "libamsolvecheck.so")
    subprocess.check_call([bmod.hipcc(), *bmod._flags(), "-shared", SRC, "-o", so])
    return so


def load(so: str):
    L = C.CDLL(so)
    p, u64 = C.c_void_p, C.c_uint64
    L.as_solve.argtypes = [u64, C.c_int, p, C.c_double, p, p]
    L.as_decide.argtypes = [u64, C.c_int, p, p, p, C.c_int, p, p, p, p]
    return L
