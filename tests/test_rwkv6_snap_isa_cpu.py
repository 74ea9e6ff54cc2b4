"""ISA guard of the snapshot instantiations of the packed stateful inference kernels (chunk_fwd_varlen_snap_kernel of wkv6_chunk.hip,
scan_fwd_kernel<T, 8, false, SNAP = true> of wkv6_scan.hip), no GPU needed: hipcc cross-compiles gfx950.  From the kernel metadata alone:
none of the four spills a vector register or has a private segment."""
import os
import shutil
import subprocess
import tempfile

import pytest

from test_varlen_isa_cpu import FLAGS, ROOT, kernel_meta

# scan_fwd_kernel<float | _Float16 | unsigned short (raw bf16), 8 waves, false, SNAP = true>
WANTED = {"wkv6_chunk.hip": ["chunk_fwd_varlen_snap_kernel"],
          "wkv6_scan.hip": ["scan_fwd_kernelIfLi8ELb0ELb1E", "scan_fwd_kernelIDF16_Li8ELb0ELb1E", "scan_fwd_kernelItLi8ELb0ELb1E"]}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
@pytest.mark.parametrize("src", sorted(WANTED))
def test_snapshot_instantiations_spill_nothing(src):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, src + ".s")
        subprocess.check_call(["hipcc"] + FLAGS + ["-o", out, os.path.join(ROOT, "rwkv_lm_ext_amd", "csrc", src)])
        asm = open(out).read()
    spills, scratch = kernel_meta(asm, "vgpr_spill_count"), kernel_meta(asm, "private_segment_fixed_size")
    for w in WANTED[src]:
        hit = [n for n in spills if w in n]
        assert len(hit) == 1, (w, hit)
        assert spills[hit[0]] == 0, (hit[0], spills[hit[0]])
        assert scratch[hit[0]] == 0, (hit[0], scratch[hit[0]])
