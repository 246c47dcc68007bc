"""CPU check of the device-math harness (tests/device_math_check.hip, run on the GPU by tests/test_gpu_device_math.py):
it must compile for gfx950 with the library's own flags, so that a change to a header or a flag that breaks it shows on
every CPU run and not first on a GPU machine.  Also pins the host constants the barrier-band test is built on."""
import math

import device_math_harness as dmh


def test_harness_compiles_with_the_library_flags(tmp_path):
    L = dmh.load(dmh.compile_harness(tmp_path))
    # the band of the cheap barrier test: finite up to L = n * 5.295e-6 <= 0.3 (56 000 steps), +inf beyond (57 000)
    lb, wd = dmh.consts(L, 56000, 110.0, 100.0)
    assert math.isfinite(wd) and wd > 0 and abs(lb / (math.log(1.1) * 65536 / math.log(2)) - 1) < 1e-15
    assert dmh.consts(L, 57000, 110.0, 100.0)[1] == math.inf
    assert 1e-6 < dmh.consts(L, 1, 100.0, 100.0)[1] < 3e-6
