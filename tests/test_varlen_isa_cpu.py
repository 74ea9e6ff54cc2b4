"""ISA guard of the packed variable-length instantiations of the chunked kernels (chunk_fwd_varlen_kernel, chunk_bwd12k_varlen_kernel),
no GPU needed: hipcc cross-compiles gfx950.  They spill no vector register, and -- by the walk of tests/test_isa_cpu.py over every
function of both listings, which is imported and run here, not copied -- no instantiation touches scratch memory inside a loop."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import test_isa_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-strict-aliasing", "-w", "-S", "--cuda-device-only"]
# forward: (raw bf16 decay | fp32 ew) x (full | state pass); backward: both decay kinds
WANTED = {"wkv6_chunk.hip": ["chunk_fwd_varlen_kernelILb1ELb0E", "chunk_fwd_varlen_kernelILb0ELb0E",
                             "chunk_fwd_varlen_kernelILb1ELb1E", "chunk_fwd_varlen_kernelILb0ELb1E"],
          "wkv6_chunk_bwd12k.hip": ["chunk_bwd12k_varlen_kernelILb1E", "chunk_bwd12k_varlen_kernelILb0E"]}


def kernel_meta(asm, key):
    names = re.findall(r"^\s+\.name:\s+(\S+)", asm, re.M)
    vals = [int(x) for x in re.findall(r"^\s+\." + key + r":\s+(\d+)", asm, re.M)]
    assert len(names) == len(vals) and names
    return dict(zip(names, vals))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_packed_instantiations_spill_nothing_and_keep_scratch_out_of_loops():
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
    # every function of both listings, the packed ones included: no scratch instruction inside a loop (and the benched dense
    # instantiations still spill nothing)
    test_isa_cpu.test_no_scratch_access_inside_any_loop_and_no_spill_in_the_benched_kernels()
