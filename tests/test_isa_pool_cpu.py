"""ISA guard of the packed pooling kernels (csrc/wkv6_pool.hip), no GPU needed: hipcc cross-compiles gfx950.  From the kernel metadata
alone, as tests/test_isa_spills_cpu.py does for the other packed features: each of the six instantiations (forward and backward, three kinds)
exists exactly once, spills no vector register and has no private segment."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_listing                                                  # noqa: E402

KERNELS = [f"pool_{way}_kernelILi{kind}EE" for way in ("fwd", "bwd") for kind in (0, 1, 2)]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_the_pool_kernels_spill_nothing_and_have_no_private_segment():
    asm = isa_listing.listing("wkv6_pool.hip")
    spills, scratch = isa_listing.kernel_meta(asm, "vgpr_spill_count"), isa_listing.kernel_meta(asm, "private_segment_fixed_size")
    for w in KERNELS:
        hit = [n for n in spills if w in n]
        assert len(hit) == 1, (w, hit)
        assert spills[hit[0]] == 0 and scratch[hit[0]] == 0, (hit[0], spills[hit[0]], scratch[hit[0]])
