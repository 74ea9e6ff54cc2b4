"""ISA guard of the packed reversal-map and pair instantiations of the chunked kernels (general token addressing on packed rows), no GPU
needed: hipcc cross-compiles gfx950.  None of them spills a vector register or reserves scratch memory, and -- by the walk of
tests/test_isa_cpu.py over every function of both listings, imported and run here, not copied -- no instantiation touches scratch
memory inside a loop."""
import os
import shutil
import subprocess
import tempfile

import pytest

import test_isa_cpu
from test_varlen_isa_cpu import FLAGS, ROOT, kernel_meta

# forward: (raw bf16 decay | fp32 ew) x (full | state pass) under a map, the pair with both decay kinds; backward: both decay kinds each
WANTED = {"wkv6_chunk.hip": ["chunk_fwd_varlen_rev_kernelILb1ELb0E", "chunk_fwd_varlen_rev_kernelILb0ELb0E",
                             "chunk_fwd_varlen_rev_kernelILb1ELb1E", "chunk_fwd_varlen_rev_kernelILb0ELb1E",
                             "chunk_fwd_varlen_pair_kernelILb1E", "chunk_fwd_varlen_pair_kernelILb0E"],
          "wkv6_chunk_bwd12k.hip": ["chunk_bwd12k_varlen_rev_kernelILb1E", "chunk_bwd12k_varlen_rev_kernelILb0E",
                                    "chunk_bwd12k_varlen_pair_kernelILb1E", "chunk_bwd12k_varlen_pair_kernelILb0E"]}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_packed_map_and_pair_instantiations_spill_nothing_and_keep_scratch_out_of_loops():
    with tempfile.TemporaryDirectory() as tmp:
        for src, wanted in WANTED.items():
            out = os.path.join(tmp, src + ".s")
            subprocess.check_call(["hipcc"] + FLAGS + ["-o", out, os.path.join(ROOT, "rwkv_lm_ext_amd", "csrc", src)])
            asm = open(out).read()
            spills, scratch = kernel_meta(asm, "vgpr_spill_count"), kernel_meta(asm, "private_segment_fixed_size")
            for w in wanted:
                hit = [n for n in spills if w in n]
                assert len(hit) == 1, (w, hit)
                assert spills[hit[0]] == 0, (hit[0], spills[hit[0]])
                assert scratch[hit[0]] == 0, (hit[0], scratch[hit[0]])
    test_isa_cpu.test_no_scratch_access_inside_any_loop_and_no_spill_in_the_benched_kernels()
