"""CPU: what the built code objects say about the level-2 pass of the segmented sums (k_sum_gt_wire), after
tests/test_kernel_resources_cpu.py: the pass multiplies as k_gt_mul_wire does — accumulator and element in registers,
the stage as the products' scratch — and is held to that kernel's budget: no scratch memory, at most 256 registers (two
waves per SIMD), at most 80 KB of LDS (two workgroups per CU).

At 37 limbs the figure reached is 20 bytes of scratch per lane (five registers): the accumulator — two values of 37
limbs — is live across the whole loop beside the products' 6 x 37 registers, where k_gt_mul_wire<37>, whose operands
die with the one product, has 23 registers to spare ("Segmented sums").  The bound for 37 limbs is that
figure; registers and LDS hold the budget at every limb count."""
import os

import pytest

from conftest import ROOT
from test_kernel_resources_cpu import LLVM, kernel_notes


SCRATCH = {36: 0, 19: 0, 37: 20}       # bytes per lane


@pytest.mark.parametrize("nl", [36, 37, 19])
def test_level2_sum_pass_holds_the_budget_of_the_fused_add(nl):
    obj = os.path.join(ROOT, "bgn_amd", "csrc", "build", "kern_nl%d.o" % nl)
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no built kernel objects / LLVM tools here")
    notes = kernel_notes(obj)
    mine = [v for k, v in notes.items() if "k_sum_gt_wireILi%dE" % nl in k]
    assert len(mine) == 1, [k for k in notes if "k_sum" in k]
    f = mine[0]
    print("k_sum_gt_wire<%d>: %s" % (nl, f))
    assert f["private_segment_fixed_size"] <= SCRATCH[nl], f         # nothing spilled to scratch memory (37 limbs: five registers)
    assert f["vgpr_count"] + f["agpr_count"] <= 256, f               # two waves per SIMD
    assert f["group_segment_fixed_size"] <= 80 * 1024, f             # two workgroups per CU
