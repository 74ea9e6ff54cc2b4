"""ISA guard of the low-rank time-mix kernels (csrc/wkv6_lowrank.hip), no GPU needed: hipcc cross-compiles gfx950.  From the kernel
metadata alone, as tests/test_isa_ce_cpu.py does for the cross-entropy kernels: each of the six instantiations (shrink with and without
the lerp in front; expand with the lerp epilogue at D = 32 and 64, with the bias epilogue at Dd = 64 and 128) exists exactly once, spills
no vector register and has no private segment."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_listing                                                  # noqa: E402

KERNELS = (["lowrank_shrink_kernelILb%dEEE" % lerp for lerp in (1, 0)]
           + ["lowrank_expand_kernelILi%dELb%dEEE" % (r, lerp) for r, lerp in ((32, 1), (64, 1), (64, 0), (128, 0))])


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_the_lowrank_kernels_spill_nothing_and_have_no_private_segment():
    asm = isa_listing.listing("wkv6_lowrank.hip")
    spills, scratch = isa_listing.kernel_meta(asm, "vgpr_spill_count"), isa_listing.kernel_meta(asm, "private_segment_fixed_size")
    assert len([n for n in spills if "lowrank_" in n]) == len(KERNELS), sorted(spills)
    for w in KERNELS:
        hit = [n for n in spills if w in n]
        assert len(hit) == 1, (w, hit)
        assert spills[hit[0]] == 0 and scratch[hit[0]] == 0, (hit[0], spills[hit[0]], scratch[hit[0]])
