"""ISA guard of the instantiations the packed, serving and LoRA features added, no GPU needed: hipcc cross-compiles gfx950.  From the kernel
metadata alone: every kernel of the table below spills no vector register and has no private segment.  Where a feature added instantiations
of the chunked kernels' stage loops, the walk of tests/test_isa_cpu.py over every function of both chunked listings runs as well -- imported,
not copied: no instantiation touches scratch memory inside a loop.

And two tests of the helper all ISA guards read their listings through (tools/isa_listing.py)."""
import os
import shutil
import sys

import pytest

import test_isa_cpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_listing                                                  # noqa: E402

# feature -> source -> substrings of the mangled kernel names, each of which must name exactly one kernel
SPILL_FREE = {
    # packed variable-length batches.  forward: (raw bf16 decay | fp32 ew) x (full | state pass); backward: both decay kinds
    "varlen": {"wkv6_chunk.hip": ["chunk_fwd_varlen_kernelILb1ELb0E", "chunk_fwd_varlen_kernelILb0ELb0E",
                                  "chunk_fwd_varlen_kernelILb1ELb1E", "chunk_fwd_varlen_kernelILb0ELb1E"],
               "wkv6_chunk_bwd12k.hip": ["chunk_bwd12k_varlen_kernelILb1E", "chunk_bwd12k_varlen_kernelILb0E"]},
    # packed rows under a reversal map, and the packed pair (general token addressing on packed rows).  forward: (raw bf16 decay | fp32 ew) x
    # (full | state pass) under a map, the pair with both decay kinds; backward: both decay kinds each
    "varlen_rev": {"wkv6_chunk.hip": ["chunk_fwd_varlen_rev_kernelILb1ELb0E", "chunk_fwd_varlen_rev_kernelILb0ELb0E",
                                      "chunk_fwd_varlen_rev_kernelILb1ELb1E", "chunk_fwd_varlen_rev_kernelILb0ELb1E",
                                      "chunk_fwd_varlen_pair_kernelILb1E", "chunk_fwd_varlen_pair_kernelILb0E"],
                   "wkv6_chunk_bwd12k.hip": ["chunk_bwd12k_varlen_rev_kernelILb1E", "chunk_bwd12k_varlen_rev_kernelILb0E",
                                             "chunk_bwd12k_varlen_pair_kernelILb1E", "chunk_bwd12k_varlen_pair_kernelILb0E"]},
    # packed stateful inference: scan_fwd_kernel<float | _Float16 | unsigned short (raw bf16), 8 waves, SLOTS = true>
    "rwkv6_varlen": {"wkv6_chunk.hip": ["chunk_fwd_varlen_slots_kernel"],
                     "wkv6_scan.hip": ["scan_fwd_kernelIfLi8ELb1E", "scan_fwd_kernelIDF16_Li8ELb1E", "scan_fwd_kernelItLi8ELb1E"]},
    # ... with state snapshots: scan_fwd_kernel<float | _Float16 | unsigned short (raw bf16), 8 waves, false, SNAP = true>
    "rwkv6_snap": {"wkv6_chunk.hip": ["chunk_fwd_varlen_snap_kernel"],
                   "wkv6_scan.hip": ["scan_fwd_kernelIfLi8ELb0ELb1E", "scan_fwd_kernelIDF16_Li8ELb0ELb1E", "scan_fwd_kernelItLi8ELb0ELb1E"]},
    # ... with the long sequences cut over T: the state pass per item, the forward per item (the mangled name: the kernel's own name, then E
    # and the argument types)
    "rwkv6_split": {"wkv6_chunk.hip": ["chunk_fwd_varlen_seg_state_kernelE", "chunk_fwd_varlen_seg_kernelE"]},
    # the token-shift slot pool: ddlerp_fwd_slots_kernel<NS, HAS_M> for (NS = 1, no m), (NS = 5, m), (NS = 1, m), (NS = 2, no m) -- the pairs of
    # dispatch_slot_lerp -- and shift_keep_kernel
    "packed_shift": {"wkv6_mix.hip": ["ddlerp_fwd_slots_kernelILi1ELb0E", "ddlerp_fwd_slots_kernelILi5ELb1E", "ddlerp_fwd_slots_kernelILi1ELb1E",
                                      "ddlerp_fwd_slots_kernelILi2ELb0E", "shift_keep_kernel"]},
    # per-sequence LoRA adapters: lora_shrink_kernel<R> and lora_expand_kernel<R>, R = 8, 16, 32, 64
    "lora_packed": {"wkv6_lora.hip": [f"lora_{kind}_kernelILi{r}EE" for kind in ("shrink", "expand") for r in (8, 16, 32, 64)]},
}
SCRATCH_WALK_TOO = ("varlen", "varlen_rev")

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


@needs_hipcc
@pytest.mark.parametrize("feature", sorted(SPILL_FREE))
def test_instantiations_spill_nothing_and_have_no_private_segment(feature):
    for src, wanted in SPILL_FREE[feature].items():
        asm = isa_listing.listing(src)
        spills, scratch = isa_listing.kernel_meta(asm, "vgpr_spill_count"), isa_listing.kernel_meta(asm, "private_segment_fixed_size")
        for w in wanted:
            hit = [n for n in spills if w in n]
            assert len(hit) == 1, (w, hit)
            assert spills[hit[0]] == 0, (hit[0], spills[hit[0]])
            assert scratch[hit[0]] == 0, (hit[0], scratch[hit[0]])
    if feature in SCRATCH_WALK_TOO:
        # every function of both chunked listings, the packed ones included: no scratch instruction inside a loop (and the benched dense
        # instantiations still spill nothing)
        test_isa_cpu.test_no_scratch_access_inside_any_loop_and_no_spill_in_the_benched_kernels()


@needs_hipcc
def test_a_source_is_compiled_once_per_process():
    first = isa_listing.listing("wkv6_lora.hip")
    assert isa_listing.listing("wkv6_lora.hip") is first
    assert [os.path.basename(p) for p in isa_listing.COMPILED].count("wkv6_lora.hip") == 1


def test_the_listing_flags_are_the_builds():
    from rwkv_lm_ext_amd import _build
    flags = isa_listing.flags()
    kept = [f for f in _build.HIPCC_FLAGS if not f.startswith("-W")]
    assert kept and flags[:len(kept)] == kept                       # the build's, in its order, and nothing between them
    assert sorted(flags[len(kept):]) == sorted(["-w", "-S", "--cuda-device-only"])
