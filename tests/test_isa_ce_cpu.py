"""ISA guard of the LM-head cross-entropy kernels (csrc/wkv6_ce.hip), no GPU needed: hipcc cross-compiles gfx950.  From the kernel metadata
alone, as tests/test_isa_pool_cpu.py does for the pooling kernels: each of the nine instantiations (bf16 / fp16 / fp32 logits; statistics
only, fused, gradient from stored statistics) exists exactly once, spills no vector register and has no private segment."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_listing                                                  # noqa: E402

KERNELS = [f"ce_rows_kernelI{io}Li{mode}EE" for io in ("t", "DF16_", "f") for mode in (0, 1, 2)]      # t: unsigned short, raw bf16


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_the_ce_kernels_spill_nothing_and_have_no_private_segment():
    asm = isa_listing.listing("wkv6_ce.hip")
    spills, scratch = isa_listing.kernel_meta(asm, "vgpr_spill_count"), isa_listing.kernel_meta(asm, "private_segment_fixed_size")
    for w in KERNELS:
        hit = [n for n in spills if w in n]
        assert len(hit) == 1, (w, hit)
        assert spills[hit[0]] == 0 and scratch[hit[0]] == 0, (hit[0], spills[hit[0]], scratch[hit[0]])
