"""Builds tests/device_math_check.hip (the device-math harness) with the library's own compile flags, so the harness
runs the arithmetic the kernels run: -O3, the same includes, hipcc's contraction default for .hip sources."""
import ctypes as C
import importlib
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "device_math_check.hip")


def compile_harness(out_dir) -> str:
    bmod = importlib.import_module("monte-carlo-project-cuda_amd.build")
    so = os.path.join(str(out_dir), "libdevmathcheck.so")
    subprocess.check_call([bmod.hipcc(), *bmod._flags(), "-shared", SRC, "-o", so])
    return so


def load(so: str):
    L = C.CDLL(so)
    p, u32, u64, d = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double
    L.dm_radius.argtypes = [u64, p, p, p, p, p, p, p]
    L.dm_sincos.argtypes = [u64, p, p, p, p]
    L.dm_rotated.argtypes = [u64, p, p, p, p, p]
    L.dm_box_muller64.argtypes = [u64, p, p, p]
    L.dm_pairsum64.argtypes = [u64, p, p, p]
    L.dm_f32.argtypes = [u64, p, p]
    L.dm_exp.argtypes = [u64, p, p, p, p, p]
    L.dm_path.argtypes = [u32, u32, p, p, p, p, p, p]
    L.dm_consts.argtypes = [u32, d, d, C.POINTER(d), C.POINTER(d)]
    L.dm_consts.restype = None
    L.dm_barrier.argtypes = [u32, u32, p, p, p, p, p, C.c_int, p, p]
    return L


def consts(L, n_steps: int, B: float, S_start: float):
    """(logB, win_delta) as make_consts<double> computes them on the host."""
    lb, wd = C.c_double(), C.c_double()
    L.dm_consts(n_steps, B, S_start, C.byref(lb), C.byref(wd))
    return lb.value, wd.value
