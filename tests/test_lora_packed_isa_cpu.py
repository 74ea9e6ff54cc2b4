"""ISA guard of the per-sequence LoRA kernels of wkv6_lora.hip (lora_shrink_kernel<R> and lora_expand_kernel<R>, R = 8, 16, 32, 64), no GPU
needed: hipcc cross-compiles gfx950.  From the kernel metadata alone: none of the eight spills a vector register or has a private segment."""
import os
import shutil
import subprocess
import tempfile

import pytest

from test_varlen_isa_cpu import FLAGS, ROOT, kernel_meta

WANTED = [f"lora_{kind}_kernelILi{r}EE" for kind in ("shrink", "expand") for r in (8, 16, 32, 64)]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_lora_kernels_spill_nothing():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "wkv6_lora.s")
        subprocess.check_call(["hipcc"] + FLAGS + ["-o", out, os.path.join(ROOT, "rwkv_lm_ext_amd", "csrc", "wkv6_lora.hip")])
        asm = open(out).read()
    spills, scratch = kernel_meta(asm, "vgpr_spill_count"), kernel_meta(asm, "private_segment_fixed_size")
    for w in WANTED:
        hit = [n for n in spills if w in n]
        assert len(hit) == 1, (w, hit)
        assert spills[hit[0]] == 0, (hit[0], spills[hit[0]])
        assert scratch[hit[0]] == 0, (hit[0], scratch[hit[0]])
