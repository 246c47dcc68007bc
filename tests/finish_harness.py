"""Builds tests/finish_check.hip (the record-finish harness) with the library's own compile flags and links it against
the built library, whose launch_small_final, launch_final_reduce and launch_smile_finish it calls: the harness runs the
finish the pricing kernels run, the same headers at the same -O3."""
import ctypes as C
import importlib
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "finish_check.hip")


def compile_harness(out_dir) -> str:
    bmod = importlib.import_module("monte-carlo-project-cuda_amd.build")
    if not os.path.exists(bmod.LIB):
        raise RuntimeError("the finish harness links against the built library: build it first")
    so = os.path.join(str(out_dir), "libfinishcheck.so")
    subprocess.check_call([bmod.hipcc(), *bmod._flags(), "-shared", SRC, "-L" + bmod.PKG, "-lmcamd", "-Wl,-rpath," + bmod.PKG,
                           "-o", so])
    return so


def load(so: str):
    L = C.CDLL(so)
    p, u32, i, d = C.c_void_p, C.c_uint32, C.c_int, C.c_double
    L.fc_block_sum.argtypes = [i, i, i, i, u32, p, p]
    L.fc_small_final_sum.argtypes = [i, i, p, p, u32, p]
    L.fc_handoff.argtypes = [i, i, u32, u32, p, d, d, p, p, p, u32, i]
    L.fc_write_final.argtypes = [p, i, d, p]
    L.fc_library_sum.argtypes = [i, p, p, u32, i, d, p, u32, C.POINTER(i), p]
    L.fc_smile_finish.argtypes = [p, u32, u32, p, d, C.POINTER(i)]
    return L
