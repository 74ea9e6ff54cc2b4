"""ISA guard of the device-side sampler (csrc/wkv6_sample.hip), no GPU needed: hipcc cross-compiles gfx950.  From the kernel metadata alone:
each of the three instantiations -- sample_slots_kernel<float | _Float16 | unsigned short (raw bf16)> -- spills no vector register, has no
private segment, and stays inside the 128 VGPRs that its 16 waves a workgroup (4 a SIMD) leave a lane."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_listing                                                  # noqa: E402

KERNELS = ["sample_slots_kernelIfEE", "sample_slots_kernelIDF16_EE", "sample_slots_kernelItEE"]

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


@needs_hipcc
def test_the_sampler_spills_nothing_and_fits_four_waves_a_simd():
    asm = isa_listing.listing("wkv6_sample.hip")
    spills, scratch, vgprs = (isa_listing.kernel_meta(asm, key) for key in ("vgpr_spill_count", "private_segment_fixed_size", "vgpr_count"))
    lds = isa_listing.kernel_meta(asm, "group_segment_fixed_size")
    for w in KERNELS:
        hit = [n for n in spills if w in n]
        assert len(hit) == 1, (w, hit)
        assert spills[hit[0]] == 0 and scratch[hit[0]] == 0, (hit[0], spills[hit[0]], scratch[hit[0]])
        assert vgprs[hit[0]] <= 128, (hit[0], vgprs[hit[0]])
        assert lds[hit[0]] <= 16 * 1024, (hit[0], lds[hit[0]])
    assert len(spills) == len(KERNELS)                              # and the file has no other kernel
