"""ISA guard of the beam-search candidate kernels (csrc/wkv6_beam.hip), no GPU needed: hipcc cross-compiles gfx950.  From the kernel metadata
alone, as tests/test_isa_ce_cpu.py does: each instantiation -- beam_rows_kernel<float | _Float16 | unsigned short (raw bf16)> and
beam_merge_kernel -- exists exactly once, spills no vector register and has no private segment; the row kernel stays inside the 128 VGPRs
that its 16 waves a workgroup (4 a SIMD) leave a lane, and the file has no other kernel."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_listing                                                  # noqa: E402

ROW_KERNELS = ["beam_rows_kernelIfEE", "beam_rows_kernelIDF16_EE", "beam_rows_kernelItEE"]
KERNELS = ROW_KERNELS + ["beam_merge_kernel"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_the_beam_kernels_spill_nothing_and_have_no_private_segment():
    asm = isa_listing.listing("wkv6_beam.hip")
    spills, scratch, vgprs = (isa_listing.kernel_meta(asm, key) for key in ("vgpr_spill_count", "private_segment_fixed_size", "vgpr_count"))
    lds = isa_listing.kernel_meta(asm, "group_segment_fixed_size")
    for w in KERNELS:
        hit = [n for n in spills if w in n]
        assert len(hit) == 1, (w, hit)
        assert spills[hit[0]] == 0 and scratch[hit[0]] == 0, (hit[0], spills[hit[0]], scratch[hit[0]])
        if w in ROW_KERNELS:
            assert vgprs[hit[0]] <= 128 and lds[hit[0]] <= 16 * 1024, (hit[0], vgprs[hit[0]], lds[hit[0]])
        else:
            assert lds[hit[0]] <= 64 * 1024, (hit[0], lds[hit[0]])
    assert len(spills) == len(KERNELS)                              # and the file has no other kernel
