"""What the operator layer refuses before it touches the library, on CPU tensors: one row per distinct `raise` of wkv6_op and mix_op that
can be reached without a GPU, with the exception type and the FULL message.  `_lib.load` is patched to raise, so a refusal that moved
behind the library load fails here as well.  (The refusals that need a GPU tensor are in tests/test_op_calls_gpu.py.)

    python tests/test_op_refusals_cpu.py      # prints EXPECTED for the tree it is run in
"""
import os
import sys


T, C, H, N = 8, 128, 2, 64


def rows():
    import torch
    from rwkv_lm_ext_amd import mix_op, wkv6_op as op
    bf, f16, f32, i32 = torch.bfloat16, torch.float16, torch.float32, torch.int32
    z = lambda *shape, dtype=bf: torch.zeros(shape, dtype=dtype)
    r, u, p, cu = z(2, T, C), z(H, N), z(T, C), torch.tensor([0, 3, 8], dtype=i32)
    i2, i3 = torch.zeros(2, dtype=i32), torch.zeros(3, dtype=i32)
    out = []

    def row(name, call, *args, **kw):
        out.append((name, lambda: call(*args, **kw)))

    # ---- _check_tensors, as far as a CPU tensor gets
    row("check_tensors type", op.wkv6_cuda.forward, 2, T, C, H, [1.0], r, r, r.float(), u, r)
    row("check_tensors cpu", op.forward_ex, r, r, r, r, u, H)
    row("check_tensors cpu first of several", op.wkv6state_cuda.backward, 2, T, C, H, r, r.float(), r, r, u, z(H, N, N), *[r] * 5, z(2, C), None)
    row("gn cpu", op.forward_gn_ex, r, r, r, r, u, H, r, z(C), z(C), 1e-5)
    row("rwkv6.forward_fp32 cpu", op.rwkv6.forward_fp32, 2, T, C, H, z(2, H, N, N, dtype=f32), r, r, r, r, u, r)

    # ---- rwkv6.forward_varlen_*: every check in front of the device
    ok = dict(state_pool=z(4, H, N, N, dtype=f32), state_slot=i2, r=p, k=p, v=p, w=p.float(), u=u, y=p, cu_seqlens=cu)
    order = ("state_pool", "state_slot", "r", "k", "v", "w", "u", "y", "cu_seqlens")

    def varlen(fn=op.rwkv6.forward_varlen_bf16, total_T=T, max_seqlen=8, **over):
        a = dict(ok, **{n: over.pop(n) for n in order if n in over})
        return fn(total_T, C, H, *(a[n] for n in order), max_seqlen, **over)

    snap = dict(state_slot_out=i2, snap_every=64, cu_snap=i3, snap_slot=torch.zeros(5, dtype=i32))
    row("varlen type", varlen, k=None)
    row("varlen dtype", varlen, k=p.half())
    row("varlen dtype fp16", varlen, fn=op.rwkv6.forward_varlen_fp16)
    row("varlen dtype w", varlen, w=p)
    row("varlen dtype state_pool", varlen, state_pool=ok["state_pool"].double())
    row("varlen type before algo", varlen, y=3, algo="fast")
    row("varlen algo", varlen, algo="fast")
    row("varlen total_T", varlen, total_T=0)
    row("varlen max_seqlen", varlen, max_seqlen=0)
    row("varlen state_pool shape", varlen, state_pool=z(4, H, N, 32, dtype=f32))
    row("varlen state_pool empty", varlen, state_pool=z(0, H, N, N, dtype=f32))
    row("varlen cu_seqlens dtype", varlen, cu_seqlens=cu.long())
    row("varlen cu_seqlens short", varlen, cu_seqlens=cu[:1])
    row("varlen cu_seqlens 2-d", varlen, cu_seqlens=cu.view(1, 3))
    row("varlen cu_seqlens strided", varlen, cu_seqlens=torch.zeros(6, dtype=i32)[::2])
    row("varlen cu_seqlens list", varlen, cu_seqlens=[0, 3, 8])
    row("varlen pool too small", varlen, state_slot=None, state_pool=z(1, H, N, N, dtype=f32))
    row("varlen state_slot shape", varlen, state_slot=i3)
    row("varlen state_slot dtype", varlen, state_slot=i2.long())
    row("varlen state_slot list", varlen, state_slot=[0, 1])
    row("varlen ws dtype", varlen, ws=torch.zeros(64, dtype=i32))
    row("varlen ws strided", varlen, ws=torch.zeros(64, dtype=torch.uint8)[::2])
    row("varlen seg_len odd", varlen, seg_len=32)
    row("varlen seg_len bool", varlen, seg_len=True)
    row("varlen seg_len float", varlen, seg_len=64.0)
    row("varlen seg_len scan", varlen, seg_len=64, algo="scan")
    row("varlen seg_len fp16", varlen, fn=op.rwkv6.forward_varlen_fp16, seg_len=64)
    row("varlen seg_len fp32", varlen, fn=op.rwkv6.forward_varlen_fp32, seg_len=0)
    row("varlen snap_every", varlen, **dict(snap, snap_every=96))
    row("varlen snap_every str", varlen, **dict(snap, snap_every="64"))
    row("varlen state_slot_out", varlen, **dict(snap, state_slot_out=i3))
    row("varlen cu_snap without snap_every", varlen, **dict(snap, snap_every=0))
    row("varlen cu_snap none", varlen, **dict(snap, cu_snap=None))
    row("varlen cu_snap shape", varlen, **dict(snap, cu_snap=i2))
    row("varlen snap_slot 2-d", varlen, **dict(snap, snap_slot=torch.zeros(2, 2, dtype=i32)))
    row("varlen snap_slot dtype", varlen, **dict(snap, snap_slot=torch.zeros(5)))
    row("varlen cpu", varlen)
    row("varlen cpu snap", varlen, **snap)
    row("varlen cpu seg_len", varlen, seg_len=64)
    a = tuple(ok[n] for n in order[2:])
    row("varlen_snap snap_every", op.rwkv6.forward_varlen_snap_bf16, T, C, H, ok["state_pool"], None, None, *a, 8, -64, None, None)
    row("varlen_snap dtype", op.rwkv6.forward_varlen_snap_fp16, T, C, H, ok["state_pool"], None, None, *a, 8, 0, None, None)
    row("varlen_snap cpu", op.rwkv6.forward_varlen_snap_bf16, T, C, H, ok["state_pool"], None, None, *a, 8, 0, None, None)
    row("varlen_snap no ws", op.rwkv6.forward_varlen_snap_bf16, T, C, H, ok["state_pool"], None, None, *a, 8, 0, None, None, ws=None)
    row("varlen_split seg_len", op.rwkv6.forward_varlen_split_bf16, T, C, H, ok["state_pool"], None, None, *a, 8, 0, None, None, 100)
    row("varlen_split cpu", op.rwkv6.forward_varlen_split_bf16, T, C, H, ok["state_pool"], None, None, *a, 8, 0, None, None, 0)

    # ---- unsupported I/O dtype: all six
    h, hp = r.half(), p.half()
    row("forward_ex dtype", op.forward_ex, h, h, h, h, u.half(), H)
    row("wkv5_forward_ex dtype", op.wkv5_forward_ex, h, h, h, u.half(), u.half(), H)
    row("forward_rev_ex dtype", op.forward_rev_ex, h, h, h, h, u.half(), H, i2, 0)
    row("backward_rev_ex dtype", op.backward_rev_ex, h, h, h, h, u.half(), h, H, i2, 0)
    row("forward_varlen_ex dtype", op.forward_varlen_ex, hp, hp, hp, hp, u.half(), H, cu, 5)
    row("backward_varlen_rev_ex dtype", op.backward_varlen_rev_ex, hp, hp, hp, hp, u.half(), hp, H, cu, 5, None, 0)

    # ---- packed: the preamble of _varlen_common and of the pair wrappers
    row("forward_varlen_ex 3-d", op.forward_varlen_ex, r, r, r, r, u, H, cu, 5)
    row("backward_varlen_ex 3-d before dtype", op.backward_varlen_ex, h, h, h, h, u, h, H, cu, 5)
    row("forward_varlen_ex cu_seqlens", op.forward_varlen_ex, p, p, p, p, u, H, cu.long(), 5)
    row("forward_varlen_ex cu_seqlens before max_seqlen", op.forward_varlen_ex, p, p, p, p, u, H, cu[:1], 0)
    row("forward_varlen_rev_ex max_seqlen", op.forward_varlen_rev_ex, p, p, p, p, u, H, cu, 0, None, 0)
    row("backward_varlen_ex cpu", op.backward_varlen_ex, p, p, p, p, u, p, H, cu, 5, ckpt_valid=True)
    q = lambda t, **kw: [dict(r=t, k=t, v=t, w=t, **kw), dict(r=t, k=t, v=t, w=t, **kw)]
    for name, fn, kw in (("forward_varlen_pair_ex", op.forward_varlen_pair_ex, {}), ("backward_varlen_pair_ex", op.backward_varlen_pair_ex, {"gy": p})):
        row(name + " 3-d", fn, H, u, q(r), cu, 5)
        row(name + " cu_seqlens", fn, H, u, q(p, **kw), [0, 3, 8], 5)
        row(name + " max_seqlen", fn, H, u, q(p, **kw), cu, 0)
        row(name + " cpu", fn, H, u, q(p, **kw), cu, 5)
    row("forward_pair_ex cpu", op.forward_pair_ex, H, u, q(r))
    row("backward_pair_ex cpu", op.backward_pair_ex, H, u, q(r, gy=r))

    # ---- wkv6_bi: mask or lens
    row("bi_forward_ex neither", op.bi_forward_ex, None, r, r, r, r, u, H)
    row("bi_forward_ex both", op.bi_forward_ex, torch.zeros(2, T, dtype=i32), r, r, r, r, u, H, lens=i2)
    row("bi_backward_ex neither", op.bi_backward_ex, None, r, r, r, r, u, r, H)
    row("bi_backward_ex mask type", op.bi_backward_ex, [[1] * T] * 2, r, r, r, r, u, r, H)
    row("bi_forward_ex lens cpu", op.bi_forward_ex, None, r, r, r, r, u, H, lens=i2)

    # ---- mix_op: the autograd ops
    row("ddlerp cpu", mix_op.ddlerp, r, z(5, C))
    row("ddlerp fp32", mix_op.ddlerp, r.float(), z(5, C))
    row("ddlerp varlen cpu", mix_op.ddlerp, p, z(5, C), cu_seqlens=cu)
    row("ddlerp varlen rev cpu", mix_op.ddlerp, p, z(5, C), cu_seqlens=cu, rev_n=i2)
    row("group_norm_gate cpu", mix_op.group_norm_gate, p, p, z(C), z(C), H, 1e-5)
    row("sqrelu type", mix_op.sqrelu, None)
    row("sigmoid_mul cpu", mix_op.sigmoid_mul, p, p)

    # ---- mix_op.ddlerp_slots
    x, pool = z(1, T, C), z(4, C)
    row("slots x dtype", mix_op.ddlerp_slots, x.float(), z(1, C), None, pool, None, cu)
    row("slots x 1-d", mix_op.ddlerp_slots, z(C), z(1, C), None, pool, None, cu)
    row("slots x batch", mix_op.ddlerp_slots, z(2, T, C), z(1, C), None, pool, None, cu)
    row("slots pool width", mix_op.ddlerp_slots, x, z(1, C), None, z(4, C + 64), None, cu)
    row("slots pool strided", mix_op.ddlerp_slots, x, z(1, C), None, z(4, 2 * C)[:, ::2], None, cu)
    row("slots cu_seqlens", mix_op.ddlerp_slots, x, z(1, C), None, pool, None, cu.long())
    row("slots cu_seqlens short", mix_op.ddlerp_slots, x, z(1, C), None, pool, None, cu[:1])
    row("slots maa dtype", mix_op.ddlerp_slots, x, z(1, C).float(), None, pool, None, cu)
    row("slots maa width", mix_op.ddlerp_slots, x, z(1, C + 1), None, pool, None, cu)
    row("slots m shape", mix_op.ddlerp_slots, x, z(5, C), z(5, T, C), pool, None, cu)
    row("slots NS 5 no m", mix_op.ddlerp_slots, x, z(5, C), None, pool, None, cu)
    row("slots NS 2 m", mix_op.ddlerp_slots, x, z(2, C), z(2, 1, T, C), pool, None, cu)
    row("slots pool too small", mix_op.ddlerp_slots, x, z(1, C), None, z(1, C), None, cu)
    row("slots grad", mix_op.ddlerp_slots, x.clone().requires_grad_(True), z(1, C), None, pool, None, cu)
    row("slots slots shape", mix_op.ddlerp_slots, x, z(1, C), None, pool, i3, cu)
    row("slots slots dtype", mix_op.ddlerp_slots, x, z(1, C), None, pool, i2.long(), cu)
    row("slots cpu", mix_op.ddlerp_slots, x, z(1, C), None, pool, i2, cu)

    # ---- mix_op.shift_keep
    row("keep x", mix_op.shift_keep, x.half(), cu, 5, pool, None)
    row("keep pool", mix_op.shift_keep, x, cu, 5, pool.float(), None)
    row("keep cu_seqlens", mix_op.shift_keep, x, cu.view(3, 1), 5, pool, None)
    row("keep max_seqlen 0", mix_op.shift_keep, x, cu, 0, pool, None)
    row("keep max_seqlen bool", mix_op.shift_keep, x, cu, True, pool, None)
    row("keep pool too small", mix_op.shift_keep, x, cu, 5, z(1, C), None)
    row("keep snap_every", mix_op.shift_keep, x, cu, 5, pool, None, (-1, None, None))
    row("keep snap_every float", mix_op.shift_keep, x, cu, 5, pool, None, (64.0, i3, i2))
    row("keep cu_snap", mix_op.shift_keep, x, cu, 5, pool, None, (64, i2, i2))
    row("keep cu_snap none", mix_op.shift_keep, x, cu, 5, pool, None, (64, None, i2))
    row("keep snap_slots 2-d", mix_op.shift_keep, x, cu, 5, pool, None, (64, i3, torch.zeros(2, 2, dtype=i32)))
    row("keep snap_slots before slot_out", mix_op.shift_keep, x, cu, 5, pool, i3, (64, i3, None))
    row("keep slot_out", mix_op.shift_keep, x, cu, 5, pool, i3)
    row("keep slot_out dtype", mix_op.shift_keep, x, cu, 5, pool, i2.float())
    row("keep grad", mix_op.shift_keep, x, cu, 5, pool.clone().requires_grad_(True), None)
    row("keep cpu", mix_op.shift_keep, x, cu, 5, pool, i2, (64, i3, i2))
    row("keep cpu snap_every 0 ignores the arrays", mix_op.shift_keep, x, cu, 5, pool, None, (0, "no", "arrays"))

    # ---- mix_op.lora_packed
    K, R = 64, 8
    lx, ly, A, Bp, sc = z(1, T, K), z(1, T, K), z(2, R, K), z(2, K, R), z(2, dtype=f32)
    row("lora x", mix_op.lora_packed, lx.float(), ly, A, Bp, sc, i2, cu)
    row("lora x batch", mix_op.lora_packed, z(2, T, K), ly, A, Bp, sc, i2, cu)
    row("lora y", mix_op.lora_packed, lx, z(1, T + 1, K), A, Bp, sc, i2, cu)
    row("lora y 2-d", mix_op.lora_packed, lx, z(T, K), A, Bp, sc, i2, cu)
    row("lora A_pool", mix_op.lora_packed, lx, ly, z(2, R, K + 64), Bp, sc, i2, cu)
    row("lora B_pool", mix_op.lora_packed, lx, ly, A, z(2, R, K), sc, i2, cu)
    row("lora scale", mix_op.lora_packed, lx, ly, A, Bp, sc.to(bf), i2, cu)
    row("lora R", mix_op.lora_packed, lx, ly, z(2, 4, K), z(2, K, 4), sc, i2, cu)
    row("lora K", mix_op.lora_packed, z(1, T, 32), ly, z(2, R, 32), Bp, sc, i2, cu)
    row("lora no adapters", mix_op.lora_packed, lx, ly, z(0, R, K), z(0, K, R), z(0, dtype=f32), i2, cu)
    row("lora cu_seqlens", mix_op.lora_packed, lx, ly, A, Bp, sc, i2, cu.float())
    row("lora adapter shape", mix_op.lora_packed, lx, ly, A, Bp, sc, i3, cu)
    row("lora adapter list", mix_op.lora_packed, lx, ly, A, Bp, sc, [0, 1], cu)
    row("lora grad", mix_op.lora_packed, lx, ly, A.clone().requires_grad_(True), Bp, sc, i2, cu)
    row("lora cpu", mix_op.lora_packed, lx, ly, A, Bp, sc, i2, cu)
    return out


_GPU = " must be on the GPU (the WKV6 operator has no CPU path)"
_CU_R = "cu_seqlens must be a contiguous int32 [n_seq + 1] tensor on the device of r"
_CU_X = "cu_seqlens must be a contiguous int32 [n_seq + 1] tensor on the device of x"
_SLOT = "state_slot must be a contiguous int32 [n_seq] tensor on the device of r, or None"
_WS = "ws must be a new_rwkv6_varlen_workspace() buffer on the device of r"
_MIX = " must be a bf16 GPU tensor (the fused time-mix ops have no CPU path)"
_POOL = "shift_pool must be a contiguous bf16 tensor [n_slots, C = 128] (it is used in place, never copied)"
_NS = "ddlerp_slots: supported are (NS = 1, m or not), (NS = 5, m), (NS = 2, no m)"
_SLOTS_GPU = "x must be on the GPU (the slot-pool kernels have no CPU path)"
_LORA_SIZES = "lora_packed: total_T and n_adapters must be >= 1, K and N multiples of 64 in [64, 16384]"
EXPECTED = {
    'check_tensors type': ('TypeError', 'r must be a tensor'),
    'check_tensors cpu': ('RuntimeError', 'r' + _GPU),
    'check_tensors cpu first of several': ('RuntimeError', 'r' + _GPU),
    'gn cpu': ('RuntimeError', 'r' + _GPU),
    'rwkv6.forward_fp32 cpu': ('RuntimeError', 'state' + _GPU),
    'varlen type': ('TypeError', 'k must be a tensor'),
    'varlen dtype': ('RuntimeError', 'k must be torch.bfloat16, got torch.float16'),
    'varlen dtype fp16': ('RuntimeError', 'r must be torch.float16, got torch.bfloat16'),
    'varlen dtype w': ('RuntimeError', 'w must be torch.float32, got torch.bfloat16'),
    'varlen dtype state_pool': ('RuntimeError', 'state_pool must be torch.float32, got torch.float64'),
    'varlen type before algo': ('TypeError', 'y must be a tensor'),
    'varlen algo': ('RuntimeError', "unknown algo 'fast'"),
    'varlen total_T': ('RuntimeError', 'total_T and max_seqlen must be >= 1'),
    'varlen max_seqlen': ('RuntimeError', 'total_T and max_seqlen must be >= 1'),
    'varlen state_pool shape': ('RuntimeError', 'state_pool has shape (4, 2, 64, 32), expected (n_slots, 2, 64, 64)'),
    'varlen state_pool empty': ('RuntimeError', 'state_pool has shape (0, 2, 64, 64), expected (n_slots, 2, 64, 64)'),
    'varlen cu_seqlens dtype': ('RuntimeError', _CU_R),
    'varlen cu_seqlens short': ('RuntimeError', _CU_R),
    'varlen cu_seqlens 2-d': ('RuntimeError', _CU_R),
    'varlen cu_seqlens strided': ('RuntimeError', _CU_R),
    'varlen cu_seqlens list': ('RuntimeError', _CU_R),
    'varlen pool too small': ('RuntimeError', 'state_slot=None names slot s for sequence s: the pool has 1 slots for 2 sequences'),
    'varlen state_slot shape': ('RuntimeError', _SLOT),
    'varlen state_slot dtype': ('RuntimeError', _SLOT),
    'varlen state_slot list': ('RuntimeError', _SLOT),
    'varlen ws dtype': ('RuntimeError', _WS),
    'varlen ws strided': ('RuntimeError', _WS),
    'varlen seg_len odd': ('RuntimeError', 'seg_len must be 0 or a multiple of 64, got 32'),
    'varlen seg_len bool': ('RuntimeError', 'seg_len must be 0 or a multiple of 64, got True'),
    'varlen seg_len float': ('RuntimeError', 'seg_len must be 0 or a multiple of 64, got 64.0'),
    'varlen seg_len scan': ('RuntimeError', "seg_len > 0 cuts sequences on the chunked route only: not with algo='scan'"),
    'varlen seg_len fp16': ('TypeError', "_Rwkv6.forward_varlen_fp16() got an unexpected keyword argument 'seg_len'"),
    'varlen seg_len fp32': ('TypeError', "_Rwkv6.forward_varlen_fp32() got an unexpected keyword argument 'seg_len'"),
    'varlen snap_every': ('RuntimeError', 'snap_every must be 0 or a multiple of 64, got 96'),
    'varlen snap_every str': ('RuntimeError', "snap_every must be 0 or a multiple of 64, got '64'"),
    'varlen state_slot_out': ('RuntimeError', 'state_slot_out must be a contiguous int32 [n_seq] tensor on the device of r'),
    'varlen cu_snap without snap_every': ('RuntimeError', 'cu_snap and snap_slot belong to snap_every > 0'),
    'varlen cu_snap none': ('RuntimeError', 'cu_snap must be a contiguous int32 [n_seq + 1] tensor on the device of r'),
    'varlen cu_snap shape': ('RuntimeError', 'cu_snap must be a contiguous int32 [n_seq + 1] tensor on the device of r'),
    'varlen snap_slot 2-d': ('RuntimeError', 'snap_slot must be a contiguous int32 [n_snap] tensor on the device of r'),
    'varlen snap_slot dtype': ('RuntimeError', 'snap_slot must be a contiguous int32 [n_snap] tensor on the device of r'),
    'varlen cpu': ('RuntimeError', 'state_pool' + _GPU),
    'varlen cpu snap': ('RuntimeError', 'state_pool' + _GPU),
    'varlen cpu seg_len': ('RuntimeError', 'state_pool' + _GPU),
    'varlen_snap snap_every': ('RuntimeError', 'snap_every must be 0 or a multiple of 64, got -64'),
    'varlen_snap dtype': ('RuntimeError', 'r must be torch.float16, got torch.bfloat16'),
    'varlen_snap cpu': ('RuntimeError', 'state_pool' + _GPU),
    'varlen_snap no ws': ('TypeError', "_Rwkv6.forward_varlen_snap_bf16() got an unexpected keyword argument 'ws'"),
    'varlen_split seg_len': ('RuntimeError', 'seg_len must be 0 or a multiple of 64, got 100'),
    'varlen_split cpu': ('RuntimeError', 'state_pool' + _GPU),
    'forward_ex dtype': ('RuntimeError', 'unsupported I/O dtype torch.float16'),
    'wkv5_forward_ex dtype': ('RuntimeError', 'unsupported I/O dtype torch.float16'),
    'forward_rev_ex dtype': ('RuntimeError', 'unsupported I/O dtype torch.float16'),
    'backward_rev_ex dtype': ('RuntimeError', 'unsupported I/O dtype torch.float16'),
    'forward_varlen_ex dtype': ('RuntimeError', 'unsupported I/O dtype torch.float16'),
    'backward_varlen_rev_ex dtype': ('RuntimeError', 'unsupported I/O dtype torch.float16'),
    'forward_varlen_ex 3-d': ('RuntimeError', 'packed tensors are [total_T, C]'),
    'backward_varlen_ex 3-d before dtype': ('RuntimeError', 'packed tensors are [total_T, C]'),
    'forward_varlen_ex cu_seqlens': ('RuntimeError', _CU_R),
    'forward_varlen_ex cu_seqlens before max_seqlen': ('RuntimeError', _CU_R),
    'forward_varlen_rev_ex max_seqlen': ('RuntimeError', 'max_seqlen must be >= 1'),
    'backward_varlen_ex cpu': ('RuntimeError', 'r' + _GPU),
    'forward_varlen_pair_ex 3-d': ('RuntimeError', 'packed tensors are [total_T, C]'),
    'forward_varlen_pair_ex cu_seqlens': ('RuntimeError', _CU_R),
    'forward_varlen_pair_ex max_seqlen': ('RuntimeError', 'max_seqlen must be >= 1'),
    'forward_varlen_pair_ex cpu': ('RuntimeError', 'r' + _GPU),
    'backward_varlen_pair_ex 3-d': ('RuntimeError', 'packed tensors are [total_T, C]'),
    'backward_varlen_pair_ex cu_seqlens': ('RuntimeError', _CU_R),
    'backward_varlen_pair_ex max_seqlen': ('RuntimeError', 'max_seqlen must be >= 1'),
    'backward_varlen_pair_ex cpu': ('RuntimeError', 'r' + _GPU),
    'forward_pair_ex cpu': ('RuntimeError', 'r' + _GPU),
    'backward_pair_ex cpu': ('RuntimeError', 'r' + _GPU),
    'bi_forward_ex neither': ('RuntimeError', 'pass either mask or lens'),
    'bi_forward_ex both': ('RuntimeError', 'pass either mask or lens'),
    'bi_backward_ex neither': ('RuntimeError', 'pass either mask or lens'),
    'bi_backward_ex mask type': ('TypeError', 'mask must be a tensor'),
    'bi_forward_ex lens cpu': ('RuntimeError', 'lens' + _GPU),
    'ddlerp cpu': ('RuntimeError', 'x' + _MIX),
    'ddlerp fp32': ('RuntimeError', 'x' + _MIX),
    'ddlerp varlen cpu': ('RuntimeError', 'x' + _MIX),
    'ddlerp varlen rev cpu': ('RuntimeError', 'x' + _MIX),
    'group_norm_gate cpu': ('RuntimeError', 'y' + _MIX),
    'sqrelu type': ('RuntimeError', 'x' + _MIX),
    'sigmoid_mul cpu': ('RuntimeError', 'r' + _MIX),
    'slots x dtype': ('RuntimeError', 'x must be a bf16 tensor [1, total_T, C] (or [total_T, C])'),
    'slots x 1-d': ('RuntimeError', 'x must be a bf16 tensor [1, total_T, C] (or [total_T, C])'),
    'slots x batch': ('RuntimeError', 'a packed batch is [1, total_T, C] (or [total_T, C])'),
    'slots pool width': ('RuntimeError', _POOL),
    'slots pool strided': ('RuntimeError', _POOL),
    'slots cu_seqlens': ('RuntimeError', _CU_X),
    'slots cu_seqlens short': ('RuntimeError', _CU_X),
    'slots maa dtype': ('RuntimeError', 'maa must be a bf16 tensor [NS, C]'),
    'slots maa width': ('RuntimeError', 'maa must be a bf16 tensor [NS, C]'),
    'slots m shape': ('RuntimeError', 'm must be a bf16 tensor [5, 1, 8, 128] or None'),
    'slots NS 5 no m': ('RuntimeError', _NS),
    'slots NS 2 m': ('RuntimeError', _NS),
    'slots pool too small': ('RuntimeError', 'slots = None means slot = sequence index: the pool must hold n_seq slots'),
    'slots grad': ('RuntimeError', 'ddlerp_slots has no backward: call it under torch.no_grad() (training uses ddlerp with shifted0)'),
    'slots slots shape': ('RuntimeError', 'slots must be a contiguous int32 [2] tensor on the device of x'),
    'slots slots dtype': ('RuntimeError', 'slots must be a contiguous int32 [2] tensor on the device of x'),
    'slots cpu': ('RuntimeError', _SLOTS_GPU),
    'keep x': ('RuntimeError', 'x must be a bf16 tensor [1, total_T, C] (or [total_T, C])'),
    'keep pool': ('RuntimeError', _POOL),
    'keep cu_seqlens': ('RuntimeError', _CU_X),
    'keep max_seqlen 0': ('RuntimeError', 'max_seqlen must be an int >= 1'),
    'keep max_seqlen bool': ('RuntimeError', 'max_seqlen must be an int >= 1'),
    'keep pool too small': ('RuntimeError', 'slot_out = None means slot = sequence index: the pool must hold n_seq slots'),
    'keep snap_every': ('RuntimeError', 'snap_every must be an int >= 0'),
    'keep snap_every float': ('RuntimeError', 'snap_every must be an int >= 0'),
    'keep cu_snap': ('RuntimeError', 'cu_snap must be a contiguous int32 [3] tensor on the device of x'),
    'keep cu_snap none': ('RuntimeError', 'cu_snap must be a contiguous int32 [3] tensor on the device of x'),
    'keep snap_slots 2-d': ('RuntimeError', 'snap_slots must be a contiguous int32 1-d tensor on the device of x'),
    'keep snap_slots before slot_out': ('RuntimeError', 'snap_slots must be a contiguous int32 1-d tensor on the device of x'),
    'keep slot_out': ('RuntimeError', 'slot_out must be a contiguous int32 [2] tensor on the device of x'),
    'keep slot_out dtype': ('RuntimeError', 'slot_out must be a contiguous int32 [2] tensor on the device of x'),
    'keep grad': ('RuntimeError', 'shift_keep writes the pool in place and has no backward'),
    'keep cpu': ('RuntimeError', _SLOTS_GPU),
    'keep cpu snap_every 0 ignores the arrays': ('RuntimeError', _SLOTS_GPU),
    'lora x': ('RuntimeError', 'x must be a contiguous bf16 tensor [1, total_T, K] (or [total_T, K])'),
    'lora x batch': ('RuntimeError', 'x must be a contiguous bf16 tensor [1, total_T, K] (or [total_T, K])'),
    'lora y': ('RuntimeError', "y must be a contiguous bf16 tensor [1, 8, 'N'] (it is updated in place, never copied)"),
    'lora y 2-d': ('RuntimeError', "y must be a contiguous bf16 tensor [1, 8, 'N'] (it is updated in place, never copied)"),
    'lora A_pool': ('RuntimeError', 'A_pool must be a contiguous bf16 tensor [n_adapters, R, K = 64]'),
    'lora B_pool': ('RuntimeError', 'B_pool must be a contiguous bf16 tensor [n_adapters = 2, N = 64, R = 8]'),
    'lora scale': ('RuntimeError', 'scale must be a contiguous fp32 tensor [n_adapters = 2]'),
    'lora R': ('RuntimeError', 'lora_packed: R must be one of (8, 16, 32, 64) (zero-pad a lower rank), got 4'),
    'lora K': ('RuntimeError', _LORA_SIZES),
    'lora no adapters': ('RuntimeError', _LORA_SIZES),
    'lora cu_seqlens': ('RuntimeError', _CU_X),
    'lora adapter shape': ('RuntimeError', 'adapter must be a contiguous int32 [2] tensor on the device of x'),
    'lora adapter list': ('RuntimeError', 'adapter must be a contiguous int32 [2] tensor on the device of x'),
    'lora grad': ('RuntimeError', "lora_packed has no backward: call it under torch.no_grad() (adapters.MultiLoraLinear's eager path has autograd)"),
    'lora cpu': ('RuntimeError', 'x must be on the GPU (lora_packed has no CPU path)'),
}


def observed():
    import torch
    got = {}
    for name, call in rows():
        assert name not in got, name
        try:
            with torch.enable_grad():
                call()
            got[name] = (None, "no exception")
        except Exception as e:                                  # noqa: BLE001  (the table says which type it has to be)
            got[name] = (type(e).__name__, str(e))
    return got


def test_refusals_keep_their_type_message_and_place_before_the_library(monkeypatch):
    from rwkv_lm_ext_amd import _lib

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", no_library)
    got = observed()
    assert list(got) == list(EXPECTED)
    for name, want in EXPECTED.items():
        assert got[name] == want, f"{name}: {got[name]}, expected {want}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from rwkv_lm_ext_amd import _lib

    def _no_library():
        raise AssertionError("the library was called")

    _lib.load = _no_library
    print("EXPECTED = {")
    for _name, _want in observed().items():
        print(f"    {_name!r}: {_want!r},")
    print("}")
