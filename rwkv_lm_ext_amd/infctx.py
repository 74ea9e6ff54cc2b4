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


# ---- the last step of the serving loop: logits rows to token ids on the device.  The sequence's decaying token-occurrence counts are a
# fourth state under the slot number of its WKV state and shift tokens, in a pool of its own so that PackedPools stays what it is.
@dataclass
class SamplingPool:
    """occ fp32 [n_slots,ld]: row p holds the occurrence counts of the sequence in slot p over the first `vocab` columns; the others are
    padding (ld: a multiple of 8, the row stride of the padded head's logits) and are never touched."""
    occ: torch.Tensor
    vocab: int

    @staticmethod
    def create(n_slots, vocab, device, ld=None):
        ld = (vocab + 7) // 8 * 8 if ld is None else int(ld)
        if ld < vocab or ld % 8:
            raise ValueError(f"ld must be a multiple of 8 and at least vocab = {vocab}, got {ld}")
        return SamplingPool(torch.zeros((n_slots, ld), device=device, dtype=torch.float32), int(vocab))


def sampling_params(n_seq, device, temperature=1.0, top_p=1.0, top_k=0, alpha_presence=0.0, alpha_frequency=0.0, alpha_decay=1.0,
                    repetition_penalty=1.0):
    """params fp32 [n_seq,8] with every sequence on the given settings (the columns in the order of the arguments, then 0); a serving loop
    then writes the rows of the sequences that differ."""
    row = (temperature, top_p, top_k, alpha_presence, alpha_frequency, alpha_decay, repetition_penalty, 0.0)
    return torch.tensor(row, dtype=torch.float32, device=device).repeat(n_seq, 1)


def _first_true(mask, none):
    """[rows]: the first column at which mask [rows,V] holds, `none` where it never does."""
    V = mask.shape[1]
    cols = torch.arange(V, device=mask.device).expand_as(mask)
    first = torch.where(mask, cols, torch.full_like(cols, V)).amin(1)
    return torch.where(first < V, first, none)


def _sample_eager(logits, occ, slots, params, u, out_slots):
    """The operation of include/wkv6_amd.h (rwkv6_sample_slots_*) restated with torch ops, on any device: fp32 z, one stable sort for the
    order, fp64 sums.  Reads nothing on the host."""
    n_seq, V = logits.shape
    n_slots, dev = occ.shape[0], logits.device
    x = logits.float()
    src = torch.arange(n_seq, device=dev) if slots is None else slots.long()
    dst = src if out_slots is None else out_slots.long()
    src_ok, dst_ok = (src >= 0) & (src < n_slots), (dst >= 0) & (dst < n_slots)
    o = occ[src.clamp(0, n_slots - 1)].masked_fill(~src_ok.unsqueeze(1), 0.0)
    temp, top_p, top_k, ap, af, decay, pen = (params[:, i:i + 1] for i in range(7))
    inf = float("inf")
    poisoned = ~(x < inf).all(1) | ~(x > -inf).any(1) | ~((params >= 0) & (params < inf)).all(1)
    z = torch.where(o > 0, x - (ap + o * af), x)
    z = torch.where(z == 0, torch.zeros_like(z), z)
    z = torch.where(z == z, z, torch.full_like(z, -inf))
    # 2.-4.: the order, the nucleus threshold with its ties, the first top_k of the order
    zs, order = torch.sort(z, dim=1, descending=True, stable=True)
    cum = torch.softmax(zs.double(), 1).cumsum(1)
    reach = cum >= top_p.double()
    c = _first_true(reach, torch.full((n_seq,), V - 1, device=dev))
    cut = torch.where((top_p < 1) & reach.any(1, keepdim=True), zs.gather(1, c.unsqueeze(1)), torch.full_like(top_p, -inf))
    kept_sorted = zs >= cut
    k_on = (top_k >= 1) & (top_k < V)
    kept_sorted &= ~k_on | (torch.arange(V, device=dev).unsqueeze(0) < top_k.floor())
    kept = torch.zeros_like(kept_sorted).scatter_(1, order, kept_sorted)
    # 5.-7.
    z2 = torch.where(z < 0, z * pen, z / pen)
    z2 = torch.where(z2 == 0, torch.zeros_like(z2), z2)
    z2 = torch.where((o > 0) & (pen != 1), torch.where(z2 == z2, z2, torch.full_like(z2, -inf)), z)
    greedy = temp == 0
    none = torch.full((n_seq,), -1, device=dev)
    tok_greedy = _first_true(z2 == z2.amax(1, keepdim=True), none)
    top = z2.masked_fill(~kept, -inf).amax(1, keepdim=True)
    w = torch.where(kept, torch.exp(((z2 - top) / torch.where(greedy, torch.ones_like(temp), temp)).double()), torch.zeros_like(cum))
    cdf = w.cumsum(1)
    W = cdf[:, -1:]
    last_kept = V - 1 - _first_true(kept.flip(1), torch.full((n_seq,), V, device=dev))
    tok_drawn = _first_true(cdf > u.double().clamp_min(0).unsqueeze(1) * W, last_kept)
    token = torch.where(greedy.squeeze(1), tok_greedy, tok_drawn)
    poisoned = poisoned | (token < 0)
    at = token.clamp(0, V - 1).unsqueeze(1)
    logprob = torch.where(greedy, torch.zeros_like(W), torch.log(w.gather(1, at) / W)).squeeze(1).float()
    # 8.: rows of poisoned sequences and of slots outside the pool go to a dummy row behind the pool
    new = (o * decay).scatter_add_(1, at, torch.ones_like(at, dtype=torch.float32))
    dest = torch.where(dst_ok & ~poisoned, dst, torch.full_like(dst, n_slots))
    occ.copy_(torch.cat((occ, occ.new_zeros(1, V))).index_copy_(0, dest, new)[:n_slots])
    nan = torch.full_like(logprob, float("nan"))
    return torch.where(poisoned, none, token).int(), torch.where(poisoned, nan, logprob)


def _sample_kernel(logits, occ, slots, params, u, out_slots, kernels):
    """Whether mix_op.sample_slots serves this call (kernels as pool_kernels of _pool_kernels: None where it applies, False never, True it
    must -- then mix_op says what is wrong)."""
    if kernels is False:
        return False
    if kernels:
        return True
    def ints(t):
        return t is None or (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_contiguous() and t.device == logits.device)
    def floats(t, shape):
        return t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous() and t.device == logits.device
    n_seq, V = logits.shape
    ld = logits.stride(0)
    return (logits.is_cuda and logits.dtype in (torch.bfloat16, torch.float16, torch.float32) and logits.stride(1) == 1 and ld >= V
            and ld % 8 == 0 and V <= 65536 and occ.device == logits.device and occ.stride(1) == 1 and occ.stride(0) == ld
            and logits.data_ptr() % 16 == 0 and occ.data_ptr() % 16 == 0 and ints(slots) and ints(out_slots) and floats(params, (n_seq, 8))
            and floats(u, (n_seq,)) and (slots is not None or occ.shape[0] >= n_seq)
            and not (torch.is_grad_enabled() and any(t.requires_grad for t in (logits, occ, params, u))))


def sample_packed(logits, pool, slots, params, u, out_slots=None, kernels=None):
    """(tokens int32 [n_seq], logprob fp32 [n_seq]): one token per row of logits [n_seq, >= pool.vocab] (the columns past the vocabulary are
    a padded head's and are ignored), sequence s with params[s] (fp32 [n_seq,8]: see sampling_params) and the uniform draw u[s]; its
    occurrence counts are read from pool.occ[slots[s]] (slots None: row s; a slot outside the pool: zero) and written, decayed and with the
    token counted, to pool.occ[out_slots[s]] (None: in place).  A poisoned row (NaN or +inf logits, no finite logit, a negative or
    non-finite parameter) gives -1 and NaN and keeps its counts.  include/wkv6_amd.h states the operation.
    kernels None: one mix_op.sample_slots launch where it applies (GPU tensors, the row stride of logits a multiple of 8 and equal to the
    pool's), else the eager restatement, which also serves the CPU; False: always the eager code; True: the kernel, or this raises."""
    if not (isinstance(logits, torch.Tensor) and logits.dim() == 2 and logits.shape[1] >= pool.vocab):
        raise RuntimeError(f"logits must be [n_seq, >= vocab = {pool.vocab}]")
    lg, occ = logits[:, :pool.vocab], pool.occ[:, :pool.vocab]
    if _sample_kernel(lg, occ, slots, params, u, out_slots, kernels):
        from . import mix_op
        return mix_op.sample_slots(lg, occ, slots, params, u, out_slots=out_slots, want_logprob=True)
    with torch.no_grad():
        return _sample_eager(lg, occ, slots, params, u, out_slots)


def decode_step_packed(emb, blocks, ln_out, head, tokens, pools, sampling_pool, slots, params, u, cu_seqlens, pool_kernels=None, kernels=None):
    """One decode step of every sequence of a serving batch, token ids in and token ids out: emb(tokens) -> step_packed (one token per
    sequence: cu_seqlens is arange(n_seq + 1), int32 on the device) -> ln_out -> head -> sample_packed.  tokens int32 [n_seq]; returns the
    new tokens int32 [n_seq] (-1 for a poisoned row; such an id is embedded as token 0 if it is fed back).  All four states of sequence s
    live under slots[s], in place.  pool_kernels as in step_packed, kernels as in sample_packed.  Nothing is read on the host, so the step
    can be captured in a graph and replayed with tokens and u refilled in place."""
    x = emb(tokens.clamp_min(0)).unsqueeze(0)
    x = step_packed(blocks, x, cu_seqlens, 1, pools, slots, pool_kernels=pool_kernels)
    return sample_packed(head(ln_out(x[0])), sampling_pool, slots, params, u, kernels=kernels)[0]
