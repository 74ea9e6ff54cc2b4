"""ISA guard of the token-shift slot-pool kernels of wkv6_mix.hip (ddlerp_fwd_slots_kernel<NS, HAS_M> in its four instantiations,
shift_keep_kernel), no GPU needed: hipcc cross-compiles gfx950.  From the kernel metadata alone: none of the five spills a vector register
or has a private segment."""
import os
import shutil
import subprocess
import tempfile

import pytest

from test_varlen_isa_cpu import FLAGS, ROOT, kernel_meta

# (NS = 1, no m), (NS = 5, m), (NS = 1, m), (NS = 2, no m): the pairs of dispatch_slot_lerp
WANTED = ["ddlerp_fwd_slots_kernelILi1ELb0E", "ddlerp_fwd_slots_kernelILi5ELb1E", "ddlerp_fwd_slots_kernelILi1ELb1E",
          "ddlerp_fwd_slots_kernelILi2ELb0E", "shift_keep_kernel"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_slot_pool_kernels_spill_nothing():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "wkv6_mix.s")
        subprocess.check_call(["hipcc"] + FLAGS + ["-o", out, os.path.join(ROOT, "rwkv_lm_ext_amd", "csrc", "wkv6_mix.hip")])
        asm = open(out).read()
    spills, scratch = kernel_meta(asm, "vgpr_spill_count"), kernel_meta(asm, "private_segment_fixed_size")
    for w in WANTED:
        hit = [n for n in spills if w in n]
        assert len(hit) == 1, (w, hit)
        assert spills[hit[0]] == 0, (hit[0], spills[hit[0]])
        assert scratch[hit[0]] == 0, (hit[0], scratch[hit[0]])
