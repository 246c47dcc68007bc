"""The kernel time an overlapped enqueue is charged (csrc/enqueue_intervals.hpp), without a GPU: the part of
its start-to-end interval after its predecessor's kernel ended, and the ring bookkeeping that finds the predecessor.
tests/host_enqueue_intervals_check.cpp is a stand-alone program around the header; it is built and run here under the
host sanitizers.  It covers a predecessor that ended before the job's start, after its start and after its end (0, never
negative), no predecessor, an in-order call inside a run, the ring wrapping at 64 (twice), and kernels of a run that end
in another order than they were enqueued in (the charge follows the ends)."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_interval_arithmetic_and_ring_under_asan_ubsan(tmp_path):
    exe = tmp_path / "enqueue_intervals_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "monte-carlo-project-cuda_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_enqueue_intervals_check.cpp"), "-o", str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    r = json.loads(done.stdout)
    assert r["failures"] == 0 and r["cases"] >= 1040
