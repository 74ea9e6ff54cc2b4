"""Carried-state ("infctx") containers and block forward for long sequences processed in chunks.

Mirrors src/infctx_module.py:1-50 (TimeMixState, ChannelMixState, BlockState, BlockStateList; wkv states
[L, B, H, N, N] in bf16, value-major like the kernels, shift states [L, 2, B, C]) and the *_infctx module forwards of
src/model.py:738-812: token shift starts from the previous chunk's last token, the WKV starts from the carried
state and hands the final state on (RUN_CUDA_RWKV6_STATE of the 'infctx' flavour, src/model.py:130-132).
"""
import torch


from dataclasses import dataclass


@dataclass
class TimeMixState:
    """What a time-mix layer carries to the next chunk: the last token (for the token shift) and the WKV state [B, H, N, N]."""
    shift_state: torch.Tensor
    wkv_state: torch.Tensor


@dataclass
class ChannelMixState:
    """What a channel-mix layer carries: the last token of the chunk."""
    shift_state: torch.Tensor


@dataclass
class BlockState:
    time_mix_state: TimeMixState
    channel_mix_state: ChannelMixState


_TMIX, _CMIX = 0, 1          # slot of each sub-layer in shift_states[layer]


class BlockStateList:
    """All layers' carried state in two tensors: `wkv_states` [L, B, H, N, N] (always bf16: the kernels' state dtype) and
    `shift_states` [L, 2, B, C] (activation dtype).  Indexing with a layer number gives views, assignment copies into them.
    Same constructor, factories, attribute names and indexing protocol as the reference's container (src/infctx_module.py:20-50),
    because training scripts build and index it directly."""

    def __init__(self, shift_states, wkv_states):
        self.shift_states, self.wkv_states = shift_states, wkv_states

    @classmethod
    def _allocate(cls, alloc, n_layer, B, C, H, device, dtype):
        head = C // H
        return cls(alloc((n_layer, 2, B, C), device=device, dtype=dtype),
                   alloc((n_layer, B, H, head, head), device=device, dtype=torch.bfloat16))

    @staticmethod
    def empty(N, B, C, H, device, dtype):
        return BlockStateList._allocate(torch.empty, N, B, C, H, device, dtype)

    @staticmethod
    def create(N, B, C, H, device, dtype):
        return BlockStateList._allocate(torch.zeros, N, B, C, H, device, dtype)

    def __len__(self):
        return self.wkv_states.shape[0]

    def __getitem__(self, layer):
        shift = self.shift_states[layer]
        return BlockState(TimeMixState(shift[_TMIX], self.wkv_states[layer]), ChannelMixState(shift[_CMIX]))

    def __setitem__(self, layer, state):
        tm, cm = state.time_mix_state, state.channel_mix_state
        self.wkv_states[layer].copy_(tm.wkv_state)
        self.shift_states[layer, _TMIX].copy_(tm.shift_state)
        self.shift_states[layer, _CMIX].copy_(cm.shift_state)


def _default_wkv_state(B, T, C, H, r, k, v, w, u, s):
    from .wkv import RUN_CUDA_RWKV6_INFCTX
    bf = torch.bfloat16
    y, s = RUN_CUDA_RWKV6_INFCTX(B, T, C, H, *(t.to(bf).contiguous() for t in (r, k, v, w, u)), s)
    return y.to(r.dtype), s


def tmix_forward_infctx(tm, x, last_state, wkv_state=None):
    """RWKV_Tmix_x060_infctx.forward (src/model.py:773-782) for a callers.Tmix_x060 `tm`."""
    B, T, C = x.size()
    shifted = torch.cat((last_state.shift_state.unsqueeze(1), x[:, :-1]), dim=1)
    r, k, v, g, w = tm.jit_func(x, shifted=shifted)
    s = last_state.wkv_state.clone().contiguous()
    y, s = (wkv_state or _default_wkv_state)(B, T, C, tm.n_head, r, k, v, w, tm.time_faaaa, s)
    return tm.jit_func_2(y, g), TimeMixState(x[:, -1], s)


def cmix_forward_infctx(cm, x, last_state):
    """RWKV_CMix_x060_infctx.forward (src/model.py:803-812) for a callers.CMix_x060 `cm`."""
    xx = torch.cat((last_state.shift_state.unsqueeze(1), x[:, :-1]), dim=1) - x
    k = torch.relu(cm.key(x + xx * cm.time_maa_k)) ** 2
    return torch.sigmoid(cm.receptance(x + xx * cm.time_maa_r)) * cm.value(k), ChannelMixState(x[:, -1])


# ---- a serving loop's packed batch: sequences of any lengths back to back in x [1,total_T,C], the carried state of sequence s in slot
# slots[s] (int32 [n_seq] on the device of x) of caller-owned pools -- shift_pool [n_slots,C] (the last token of the sequence's previous
# call, one pool per sub-layer) and wkv_pool fp32 [n_slots,H,N,N].  A slot outside the pool means no state: zero in, nothing kept.
# cu_seqlens and slots are never read on the host.
def _carried_tokens(shift_pool, slots):
    """[n_seq,C]: shift_pool[slots[s]], zero where the slot lies outside the pool."""
    n = shift_pool.shape[0]
    s = slots.long()
    ok = (s >= 0) & (s < n)
    return shift_pool[s.clamp(0, n - 1)].masked_fill(~ok.unsqueeze(1), 0).contiguous()


def _keep_last_tokens(shift_pool, slots, x, cu_seqlens, max_seqlen=None):
    """shift_pool[slots[s]] = the last token of sequence s; empty sequences and slots outside the pool leave the pool alone (their rows go
    to a dummy slot behind it)."""
    n, T = shift_pool.shape[0], x.shape[0]
    cu, s = cu_seqlens.long().clamp(0, T), slots.long()
    length = cu[1:] - cu[:-1]
    if max_seqlen is not None:
        length = length.clamp(max=int(max_seqlen))
    alive = (length > 0) & (s >= 0) & (s < n)
    rows = x[(cu[:-1] + length - 1).clamp(0, T - 1)].to(shift_pool.dtype)
    dest = torch.where(alive, s, torch.full_like(s, n))
    shift_pool.copy_(torch.cat((shift_pool, shift_pool.new_zeros(1, shift_pool.shape[1]))).index_copy_(0, dest, rows)[:n])


def _keep_snap_tokens(shift_pool, snap, x, cu_seqlens, max_seqlen=None):
    """shift_pool[snap_slots[cu_snap[s] + j]] = token (j + 1) * snap_every - 1 of sequence s for every snapshot j the operator keeps
    (include/wkv6_amd.h: rwkv6_forward_varlen_snap_*, the same clamps); everything else goes to the dummy slot behind the pool."""
    snap_every, cu_snap, snap_slots = snap
    n, T, n_snap = shift_pool.shape[0], x.shape[0], snap_slots.numel()
    most = (T if max_seqlen is None else min(T, int(max_seqlen))) // int(snap_every)     # snapshots of the longest sequence there can be
    if most < 1 or n_snap < 1:
        return
    cu, cs = cu_seqlens.long().clamp(0, T), cu_snap.long().clamp(0, n_snap)
    length = cu[1:] - cu[:-1]
    if max_seqlen is not None:
        length = length.clamp(max=int(max_seqlen))
    count = torch.minimum(length.clamp(min=0) // int(snap_every), (cs[1:] - cs[:-1]).clamp(min=0))
    j = torch.arange(most, device=x.device).unsqueeze(0)                                 # [1, most] against [n_seq, 1]
    s = snap_slots.long()[(cs[:-1].unsqueeze(1) + j).clamp(0, n_snap - 1)]
    alive = (j < count.unsqueeze(1)) & (s >= 0) & (s < n)
    rows = x[(cu[:-1].unsqueeze(1) + (j + 1) * int(snap_every) - 1).clamp(0, T - 1).reshape(-1)].to(shift_pool.dtype)
    dest = torch.where(alive, s, torch.full_like(s, n)).reshape(-1)
    shift_pool.copy_(torch.cat((shift_pool, shift_pool.new_zeros(1, shift_pool.shape[1]))).index_copy_(0, dest, rows)[:n])


def _pool_kernels(mod, x, shift_pool, pool_kernels, ints):
    """Whether the HIP slot-pool kernels (mix_op.ddlerp_slots, mix_op.shift_keep) serve this call.  pool_kernels None: when the module's
    fused path applies, the pool is contiguous bf16 on x's device and no gradient is required; False: never (the eager code, which also
    serves fp16 / fp32 and autograd); True: they must, or this raises.  `ints`: the call's int arrays; the kernels take them as contiguous
    int32 on x's device, the eager code casts whatever it gets, so anything else stays with it (under True, mix_op refuses it)."""
    if pool_kernels is False:
        return False
    if pool_kernels is None and not all(t is None or (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_contiguous()
                                                      and t.device == x.device) for t in ints):
        return False
    why = None
    if not (x.is_cuda and x.dtype == torch.bfloat16 and mod._use_fused(x)):
        why = "the module's fused (HIP) path does not apply to x"
    elif not (shift_pool.dtype == torch.bfloat16 and shift_pool.dim() == 2 and shift_pool.is_contiguous() and shift_pool.device == x.device):
        why = "the shift pool must be a contiguous bf16 [n_slots,C] tensor on the device of x"
    elif torch.is_grad_enabled() and (x.requires_grad or shift_pool.requires_grad or any(p.requires_grad for p in mod.parameters())):
        why = "a gradient is required (the slot-pool kernels are forward only: call under torch.no_grad())"
    if why is not None and pool_kernels:
        raise RuntimeError("pool_kernels=True: " + why)
    return why is None


def tmix_forward_packed(tm, x, cu_seqlens, max_seqlen, shift_pool, wkv_pool, slots, out_slots=None, snap=None, seg_len=0, pool_kernels=None):
    """tmix_forward_infctx for every sequence of a packed batch x [1,total_T,C] in one pass (a callers.Tmix_x060 `tm`): the token shift
    starts from shift_pool[slots[s]], the operator (wkv.RUN_RWKV_6_VARLEN) from wkv_pool[slots[s]]; both pools are updated in place.
    out_slots (int32 [n_seq]): what the sequences leave goes to these slots of both pools instead, slots keeps its contents.
    snap = (snap_every, cu_snap, snap_slots): the state after every snap_every tokens is kept as well -- the WKV state and the token in
    front of the next one land in the same slot number snap_slots[cu_snap[s] + j] of their pools.
    seg_len (0: off): handed to the operator, which cuts sequences longer than that over T; the token shift has no recurrence to cut.
    pool_kernels (None: where they apply, see _pool_kernels): the shift pool is read inside the lerp kernels and written by one launch
    that touches only the rows that change, instead of the eager gather / scatter over the whole pool; the results are bit-identical."""
    from .wkv import RUN_RWKV_6_VARLEN
    B, T, C = x.size()
    assert B == 1, "a packed batch is [1,total_T,C]"
    kernels = _pool_kernels(tm, x, shift_pool, pool_kernels, (cu_seqlens, slots, out_slots) + (tuple(snap[1:]) if snap is not None else ()))
    if kernels:
        r, k, v, g, w = tm.jit_func(x, cu_seqlens=cu_seqlens, shift_pool=shift_pool, slots=slots)
    else:
        r, k, v, g, w = tm.jit_func(x, cu_seqlens=cu_seqlens, shifted0=_carried_tokens(shift_pool, slots).to(x.dtype))
    u = tm.time_faaaa.to(r.dtype).contiguous()
    snap_every, cu_snap, snap_slots = snap if snap is not None else (0, None, None)
    y, _ = RUN_RWKV_6_VARLEN(T, C, tm.n_head, wkv_pool, slots, *(t.contiguous() for t in (r, k, v, w.to(r.dtype))), u, cu_seqlens, max_seqlen,
                             state_slot_out=out_slots, snap_every=snap_every, cu_snap=cu_snap, snap_slot=snap_slots, seg_len=seg_len)
    out = tm.jit_func_2(y, g)
    if kernels:         # behind the lerps in stream order: with out_slots None they read the rows this writes
        from . import mix_op
        mix_op.shift_keep(x, cu_seqlens, int(max_seqlen), shift_pool, slots if out_slots is None else out_slots, snap)
        return out
    _keep_last_tokens(shift_pool, slots if out_slots is None else out_slots, x[0], cu_seqlens, max_seqlen)
    if snap is not None and snap_every > 0:
        _keep_snap_tokens(shift_pool, snap, x[0], cu_seqlens, max_seqlen)
    return out


def cmix_forward_packed(cm, x, cu_seqlens, shift_pool, slots, out_slots=None, snap=None, pool_kernels=None):
    """cmix_forward_infctx for every sequence of a packed batch x [1,total_T,C] (a callers.CMix_x060 `cm`); shift_pool is this sub-layer's.
    out_slots, snap and pool_kernels as in tmix_forward_packed."""
    from .callers import _packed_prev
    B, T, C = x.size()
    assert B == 1, "a packed batch is [1,total_T,C]"
    if _pool_kernels(cm, x, shift_pool, pool_kernels, (cu_seqlens, slots, out_slots) + (tuple(snap[1:]) if snap is not None else ())):
        from . import mix_op
        xk, xr = mix_op.ddlerp_slots(x, torch.cat([cm.time_maa_k, cm.time_maa_r], 0).view(2, -1), None, shift_pool, slots, cu_seqlens)
        out = mix_op.sigmoid_mul(cm.receptance(xr), cm.value(mix_op.sqrelu(cm.key(xk))))
        mix_op.shift_keep(x, cu_seqlens, T, shift_pool, slots if out_slots is None else out_slots, snap)      # no max_seqlen here: total_T
        return out
    carried = _carried_tokens(shift_pool, slots).to(x.dtype)
    if cm._use_fused(x):
        from . import mix_op
        xk, xr = mix_op.ddlerp(x, torch.cat([cm.time_maa_k, cm.time_maa_r], 0).view(2, -1), shifted0=carried, cu_seqlens=cu_seqlens)
        out = mix_op.sigmoid_mul(cm.receptance(xr), cm.value(mix_op.sqrelu(cm.key(xk))))
    else:
        xx = _packed_prev(x, cu_seqlens, carried) - x
        k = torch.relu(cm.key(x + xx * cm.time_maa_k)) ** 2
        out = torch.sigmoid(cm.receptance(x + xx * cm.time_maa_r)) * cm.value(k)
    _keep_last_tokens(shift_pool, slots if out_slots is None else out_slots, x[0], cu_seqlens)
    if snap is not None and snap[0] > 0:
        _keep_snap_tokens(shift_pool, snap, x[0], cu_seqlens)
    return out


# ---- the block-level serving step on a packed stateful batch
@dataclass
class PackedPools:
    """Every layer's carried state of a serving loop, slot p of every pool belonging to one sequence: shift_att / shift_ffn [L,n_slots,C]
    (the token in front of the sequence's next one, per sub-layer, activation dtype) and wkv fp32 [L,n_slots,H,64,64]."""
    shift_att: torch.Tensor
    shift_ffn: torch.Tensor
    wkv: torch.Tensor

    @staticmethod
    def create(n_layer, n_slots, C, H, device, dtype):
        head = C // H
        return PackedPools(torch.zeros((n_layer, n_slots, C), device=device, dtype=dtype),
                           torch.zeros((n_layer, n_slots, C), device=device, dtype=dtype),
                           torch.zeros((n_layer, n_slots, H, head, head), device=device, dtype=torch.float32))


def block_forward_packed(block, x, cu_seqlens, max_seqlen, pools, layer, slots, out_slots=None, snap=None, seg_len=0, pool_kernels=None):
    """One RWKV-6 block (anything shaped like train_dp.Block: ln0 where there is one, ln1, att, ln2, ffn) on a packed stateful batch
    x [1,total_T,C]: x + att(ln1 x), then + ffn(ln2 .), the sub-layers through tmix_forward_packed / cmix_forward_packed on slice
    `layer` of the pools.  Nothing here reads a device array on the host."""
    if getattr(block, "ln0", None) is not None:
        x = block.ln0(x)
    x = x + tmix_forward_packed(block.att, block.ln1(x), cu_seqlens, max_seqlen, pools.shift_att[layer], pools.wkv[layer], slots,
                                out_slots=out_slots, snap=snap, seg_len=seg_len, pool_kernels=pool_kernels)
    return x + cmix_forward_packed(block.ffn, block.ln2(x), cu_seqlens, pools.shift_ffn[layer], slots, out_slots=out_slots, snap=snap,
                                   pool_kernels=pool_kernels)


def step_packed(blocks, x, cu_seqlens, max_seqlen, pools, slots, out_slots=None, snap=None, seg_len=0, pool_kernels=None):
    """block_forward_packed over a stack of blocks, block i on layer i of the pools.

    Per-sequence LoRA adapters need nothing here: under adapters.inject_adapters the blocks' linears are MultiLoraLinear modules, and
    adapters.set_adapters(blocks, cu_seqlens, adapter) binds the batch on them before the call -- this function, block_forward_packed and
    the sub-layer functions reach the linears through the modules.  The two tensors are bound by reference, so a captured step is
    re-routed by refilling them in place."""
    for layer, block in enumerate(blocks):
        x = block_forward_packed(block, x, cu_seqlens, max_seqlen, pools, layer, slots, out_slots=out_slots, snap=snap, seg_len=seg_len,
                                 pool_kernels=pool_kernels)
    return x


def last_token_rows(x, cu_seqlens, max_seqlen):
    """[n_seq,C]: the last served token of every sequence of the packed bf16 batch x [1,total_T,C] (token min(len_s, max_seqlen) - 1), zeros
    for an empty one -- the rows the head needs.  One mix_op.shift_keep launch into a zeroed buffer with identity slots."""
    from . import mix_op
    rows = torch.zeros((cu_seqlens.numel() - 1, x.shape[-1]), device=x.device, dtype=x.dtype)
    mix_op.shift_keep(x, cu_seqlens, int(max_seqlen), rows, None)
    return rows
