"""CPU test of what the fp64 pair-sum loop (csrc/mc_device.hpp pair_sums_of_paths) promises about its machine code, read
from the cross-compiled gfx950 assembly by tools/loop_reads.py:
  * the headline kernel's loop holds 144 VALU instructions in 500 nominal issue cycles, i.e. 62.5 slots per path-step,
    bench.py's floor, with the same opcodes in all four variance-reduction variants, and no arithmetic shift is left of
    f64::neg2log_1k's exponent (it converts the masked word);
  * the pathwise Greeks kernel, which walks the same loop, lost the shift too;
  * the pricing kernels stay within 128 VGPRs (four workgroups per CU) and nothing uses scratch."""
import importlib.util
import os

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def loops():
    spec = importlib.util.spec_from_file_location("loop_reads", os.path.join(ROOT, "tools", "loop_reads.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    d = mod.digest()
    for sym, row in d.items():
        print(sym, {k: v for k, v in row.items() if k != "opcodes"})
    assert len(d) == 5
    return d


def price_kernels(loops):
    return {s: d for s, d in loops.items() if "price_kernel" in s}


def test_the_headline_loop_stands_at_the_slot_floor_in_every_variant(loops):
    pk = price_kernels(loops)
    assert len(pk) == 4
    for sym, d in pk.items():
        assert d["valu"] == 144 and d["issue_cycles"] == 500, (sym, d["valu"], d["issue_cycles"])
    first = next(iter(pk.values()))["opcodes"]
    assert all(d["opcodes"] == first for d in pk.values())
    assert first["ds_read_b128"] == 4 and first["v_mad_u64_u32"] == 36 and first["v_rsq_f64_e32"] == 2
    assert all("v_ashrrev_i32_e32" not in d["opcodes"] for d in loops.values())


def test_registers_keep_four_workgroups_per_cu(loops):
    for sym, d in loops.items():
        assert d["scratch"] == 0 and d["reads"] == 4 and d["reads_never_waited_for"] == 0, sym
    for sym, d in price_kernels(loops).items():
        assert d["vgpr"] <= 128 and d["lds"] <= 160 * 1024 // 4, (sym, d["vgpr"], d["lds"])
