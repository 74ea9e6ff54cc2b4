"""ISA guard of the chunked instantiations the split call adds (chunk_fwd_varlen_seg_state_kernel: the state pass per item,
chunk_fwd_varlen_seg_kernel: the forward per item), no GPU needed: hipcc cross-compiles gfx950.  From the kernel metadata, read with the helper
of test_varlen_isa_cpu.py: neither spills a vector register, neither has a private segment."""
import os
import shutil
import subprocess
import tempfile

import pytest

from test_varlen_isa_cpu import FLAGS, ROOT, kernel_meta

WANTED = ["chunk_fwd_varlen_seg_state_kernel", "chunk_fwd_varlen_seg_kernel"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_split_instantiations_spill_nothing_and_use_no_scratch():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "wkv6_chunk.s")
        subprocess.check_call(["hipcc"] + FLAGS + ["-o", out, os.path.join(ROOT, "rwkv_lm_ext_amd", "csrc", "wkv6_chunk.hip")])
        asm = open(out).read()
    spills, scratch = kernel_meta(asm, "vgpr_spill_count"), kernel_meta(asm, "private_segment_fixed_size")
    for w in WANTED:
        hit = [n for n in spills if w + "E" in n]           # (the mangled name: the kernel's own name, then E and the argument types)
        assert len(hit) == 1, (w, hit)
        assert spills[hit[0]] == 0, (hit[0], spills[hit[0]])
        assert scratch[hit[0]] == 0, (hit[0], scratch[hit[0]])
