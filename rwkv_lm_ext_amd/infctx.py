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


# ---- the other decoding mode: beam search.  A beam that forks is several children reading one parent slot and each writing a slot of its
# own, which out_slots of step_packed already provides; what is new is the selection (include/wkv6_amd.h: rwkv6_beam_candidates_*) and the
# small bookkeeping behind it on [n_groups, K] tensors.  Everything is device-side and fixed-shape, so a step can be captured and replayed.
def _best_first(s, k):
    """(values [N,k], indices [N,k]) of the k first entries of every row of s [N,M] in the order (s descending, index ascending) -- a topk
    whose ties, at the boundary included, fall to the lower index; M < k is padded with -inf / M.  No NaN in s."""
    N, M = s.shape
    if M < k:
        s = torch.cat((s, s.new_full((N, k - M), float("-inf"))), 1)
    kth = s.topk(k, dim=1).values[:, -1:]
    above, equal = s > kth, s == kth
    chosen = above | (equal & (equal.cumsum(1) <= k - above.sum(1, keepdim=True)))                     # exactly k a row
    cols = torch.arange(s.shape[1], device=s.device)
    idx = torch.where(chosen, s.shape[1] - cols, torch.zeros_like(cols)).topk(k, dim=1).indices        # ... by ascending index
    v, order = s.gather(1, idx).sort(dim=1, descending=True, stable=True)
    return v, idx.gather(1, order)


def _beam_candidates_eager(logits, cum, cu_rows, K, occ, slots, penalty):
    """The operation of include/wkv6_amd.h (rwkv6_beam_candidates_*) restated with torch ops, on any device: fp64 log_softmax and scores,
    the K best of every row and then of every group's rows (the same K as a topk on the flattened group: the group's best lie in the union
    of its rows' best), ties by row and token.  Reads nothing on the host."""
    n_rows, V = logits.shape
    dev, inf = logits.device, float("inf")
    G = cu_rows.numel() - 1
    cu = cu_rows.long().clamp(0, n_rows)
    r = torch.arange(n_rows, device=dev)
    g = torch.bucketize(r, cu[:G], right=True) - 1                          # the last group that starts at or in front of the row
    gc = g.clamp_min(0)
    in_group = (g >= 0) & (r < cu[gc + 1]) & (r - cu[gc] < 64)
    x, c = logits.float(), cum.float()
    p = torch.ones(n_rows, device=dev) if penalty is None else penalty.float()[gc]
    live = in_group & (c > -inf) & (c < inf) & (p >= 0) & (p < inf) & (x < inf).all(1) & (x > -inf).any(1)
    lp = torch.log_softmax(x.double(), 1)
    if occ is not None:
        n_slots = occ.shape[0]
        src = r if slots is None else slots.long()
        o = occ[src.clamp(0, n_slots - 1)].masked_fill(~((src >= 0) & (src < n_slots)).unsqueeze(1), 0.0)
        pd = p.double().unsqueeze(1)
        pen = torch.where(lp < 0, lp * pd, lp / pd)
        lp = torch.where((o > 0) & (pd != 1), torch.where(pen == pen, pen, torch.zeros_like(pen)), lp)
    s = c.double().unsqueeze(1) + lp
    s = torch.where(live.unsqueeze(1) & (x > -inf) & (s > -inf), s, torch.full_like(s, -inf))
    row_s, row_tok = _best_first(s, K)                                                                # [n_rows, K]
    R = min(64, n_rows)
    rows = cu[:G].unsqueeze(1) + torch.arange(R, device=dev)                                           # [G, R]
    mine = (rows < cu[1:].unsqueeze(1)).unsqueeze(2)
    rows = rows.clamp(max=n_rows - 1)
    flat = torch.where(mine, row_s[rows], torch.full_like(row_s[rows], -inf)).reshape(G, R * K)
    score, at = _best_first(flat, K)
    at = at.clamp(max=R * K - 1)
    none = score == -inf
    parent = rows.gather(1, at // K).masked_fill(none, -1)
    token = row_tok[rows].reshape(G, R * K).gather(1, at).masked_fill(none, -1)
    return parent.int(), token.int(), score.float()


def _beam_kernel(logits, cum, cu_rows, occ, slots, penalty, kernels):
    """Whether mix_op.beam_candidates serves this call (kernels as in _sample_kernel: None where it applies, False never, True it must --
    then mix_op says what is wrong).  Where it applies it is taken: profiles/beam_time.txt has the kernels ahead of the eager code at
    every size measured."""
    if kernels is False:
        return False
    if kernels:
        return True
    def ints(t):
        return t is None or (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_contiguous() and t.device == logits.device)
    def floats(t, shape):
        return (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous()
                and t.device == logits.device)
    n_rows, V = logits.shape
    ld = logits.stride(0)
    G = cu_rows.numel() - 1 if isinstance(cu_rows, torch.Tensor) else 0
    return (logits.is_cuda and logits.dtype in (torch.bfloat16, torch.float16, torch.float32) and logits.stride(1) == 1 and ld >= V
            and ld % 8 == 0 and V <= 65536 and logits.data_ptr() % 16 == 0 and floats(cum, (n_rows,)) and ints(cu_rows) and cu_rows is not None
            and cu_rows.dim() == 1 and G >= 1 and ints(slots)
            and (occ is None or (occ.device == logits.device and occ.dtype == torch.float32 and occ.stride(1) == 1 and occ.stride(0) == ld
                                 and occ.data_ptr() % 16 == 0 and floats(penalty, (G,)) and (slots is not None or occ.shape[0] >= n_rows)))
            and not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (logits, cum, occ, penalty))))


def beam_candidates(logits, cum, cu_rows, K, pool=None, slots=None, penalty=None, vocab=None, kernels=None):
    """(parent int32, token int32, score fp32), each [n_groups, K]: for every group g of rows cu_rows[g] .. cu_rows[g+1] - 1 (int32 on the
    device, at most the first 64 rows of a group) of logits [n_rows, >= vocab] the K (1..64) best continuations (row, token) by cum[row] +
    log_softmax(logits[row, :vocab])[token], best first, equal scores by row and then token; missing entries are -1, -1, -inf.  A row with
    cum == -inf is dead: it is not read and gives nothing.  A poisoned row (NaN or +inf logits, no finite logit, NaN or +inf cum, a
    negative or non-finite penalty) gives nothing either.  pool (a SamplingPool; vocab is then the pool's) with penalty fp32 [n_groups]:
    the repetition penalty, on the log-probabilities of the tokens that pool.occ[slots[row]] (slots None: row) counts.
    include/wkv6_amd.h states the operation.
    kernels None: the HIP kernels (mix_op.beam_candidates) where they apply (GPU tensors, the row stride of logits a multiple of 8 and
    equal to the pool's), else the eager restatement, which also serves the CPU; False: always the eager code; True: the kernels, or this
    raises."""
    V = pool.vocab if pool is not None else (int(vocab) if vocab is not None else (logits.shape[1] if isinstance(logits, torch.Tensor) else 0))
    if not (isinstance(logits, torch.Tensor) and logits.dim() == 2 and logits.shape[1] >= V >= 1 and logits.shape[0] >= 1):
        raise RuntimeError(f"logits must be [n_rows, >= vocab = {V}]")
    if not (isinstance(K, int) and 1 <= K <= 64):
        raise RuntimeError(f"K must be an int in [1, 64], got {K!r}")
    if (pool is None) != (penalty is None) or (slots is not None and pool is None):
        raise RuntimeError("pool and penalty go together (both None: no penalty), and slots needs them")
    lg, occ = logits[:, :V], None if pool is None else pool.occ[:, :V]
    if _beam_kernel(lg, cum, cu_rows, occ, slots, penalty, kernels):
        from . import mix_op
        return mix_op.beam_candidates(lg, cum, cu_rows, K, occ_pool=occ, slots=slots, penalty=penalty)
    with torch.no_grad():
        return _beam_candidates_eager(lg, cum, cu_rows, K, occ, slots, penalty)


@dataclass
class BeamSearch:
    """The state of a beam search over n_groups requests with W beams each, of fixed shape: n_rows = n_groups * W rows always, row
    g * W + j the j-th beam of request g, a dead row carrying cum = -inf.  Everything is a device tensor updated in place, so a captured
    beam_step_packed replays: `step` counts on the device and selects the half of the slots in use.

    tokens int32 [n_rows]: the token every row feeds next;  cum fp32 [n_rows]: its cumulative log-probability;
    slots_in / slots_out int32 [n_rows]: where a row's carried state is read and where it is left.  Request g owns the 2 W slots
      slot_base + 2 W g .. + 2 W - 1 of every pool, in two halves: step t leaves row j's state in half t % 2, slot j, and the children read
      it from there at step t + 1, whichever of them and however many.  At step 0 every slots_in entry names the request's prompt slot,
      which is only ever read;
    slots_occ int32 [n_rows]: the row's occurrence counts in a SamplingPool (the prompt slot at step 0, then the row's slots_out);
    hist_parent / hist_token int32 [max_new_tokens, n_rows]: row r of step t + 1 continues row hist_parent[t, r] of step t with hist_token[t, r];
    hyp_score fp32 / hyp_step, hyp_row int32 [n_groups, W]: the finished hypotheses, best first (-inf: none): cum / len^length_penalty
      with len = hyp_step + 1 (the eos counted, as the reference does), the step at which the eos was chosen and the row that chose it;
    done bool [n_groups]."""
    n_groups: int
    W: int
    K: int
    max_new_tokens: int
    length_penalty: float
    slot_base: int
    eos_ids: torch.Tensor
    penalty: torch.Tensor
    step: torch.Tensor
    tokens: torch.Tensor
    cum: torch.Tensor
    cu_rows: torch.Tensor
    cu_tokens: torch.Tensor
    slots_in: torch.Tensor
    slots_out: torch.Tensor
    slots_occ: torch.Tensor
    hist_parent: torch.Tensor
    hist_token: torch.Tensor
    hyp_score: torch.Tensor
    hyp_step: torch.Tensor
    hyp_row: torch.Tensor
    done: torch.Tensor

    @property
    def n_rows(self):
        return self.n_groups * self.W

    @staticmethod
    def create(n_groups, W, max_new_tokens, eos_ids, length_penalty, repetition_penalty, tokens, prompt_slots, slot_base, device, K=None):
        """tokens int [n_groups]: the token every request feeds first (the last one of its prompt);  prompt_slots int [n_groups]: the slot
        the rest of the prompt was prefilled into, outside slot_base .. slot_base + 2 W n_groups - 1;  K (None: (1 + len(eos_ids)) * W, the
        reference's reserve_beam_size, which is also the least allowed): candidates taken per request and step, at most 64."""
        eos = [int(e) for e in eos_ids]
        K = (1 + len(eos)) * W if K is None else int(K)
        if n_groups < 1 or W < 1 or max_new_tokens < 1:
            raise ValueError("n_groups, W and max_new_tokens must be at least 1")
        if not (1 + len(eos)) * W <= K <= 64:
            raise ValueError(f"K must be in [(1 + len(eos_ids)) * W, 64] = [{(1 + len(eos)) * W}, 64] so that W continuations always remain, got {K}")
        n_rows = n_groups * W
        i32 = dict(dtype=torch.int32, device=device)
        first = torch.arange(n_rows, device=device) % W == 0
        neg = torch.full((n_rows,), float("-inf"), device=device)
        prompt = torch.as_tensor(prompt_slots, **i32).reshape(n_groups)
        return BeamSearch(
            n_groups=n_groups, W=W, K=K, max_new_tokens=int(max_new_tokens), length_penalty=float(length_penalty), slot_base=int(slot_base),
            eos_ids=torch.tensor(eos, dtype=torch.int32, device=device), penalty=torch.full((n_groups,), float(repetition_penalty), device=device),
            step=torch.zeros((), dtype=torch.int64, device=device),
            tokens=torch.as_tensor(tokens, **i32).reshape(n_groups).repeat_interleave(W).contiguous(),
            cum=torch.where(first, torch.zeros_like(neg), neg),
            cu_rows=torch.arange(0, n_rows + 1, W, **i32), cu_tokens=torch.arange(n_rows + 1, **i32),
            slots_in=prompt.repeat_interleave(W).contiguous(), slots_out=_beam_half(n_groups, W, slot_base, 0, device),
            slots_occ=prompt.repeat_interleave(W).contiguous(),
            hist_parent=torch.zeros((max_new_tokens, n_rows), **i32), hist_token=torch.full((max_new_tokens, n_rows), -1, **i32),
            hyp_score=torch.full((n_groups, W), float("-inf"), device=device), hyp_step=torch.zeros((n_groups, W), **i32),
            hyp_row=torch.zeros((n_groups, W), **i32), done=torch.zeros(n_groups, dtype=torch.bool, device=device))


def _beam_half(n_groups, W, slot_base, half, device):
    """int32 [n_groups * W]: row g * W + j -> slot_base + 2 W g + W half + j; half: 0, 1 or a device tensor of one element"""
    r = torch.arange(n_groups * W, device=device)
    return (slot_base + 2 * W * (r // W) + W * half + r % W).int()


def beam_advance(state, parent, token, score, sampling_pool=None):
    """One step of the bookkeeping, in place on `state`, from the candidates (parent, token, score), each [n_groups, K] best first, of
    beam_candidates on the step's logits.  Of a request's candidates, those that end in an eos id and rank among the first W go to its
    hypothesis table with cum / len^length_penalty (the worst entry leaves a full table; an equal newcomer does not displace it); the first
    W others become the next rows: token, cum, the parent's slots_out as slots_in, the other half as slots_out.  A request is done when its
    table is full and its worst entry is at least (best cum of the step) / len^length_penalty (BeamHypothesis.is_done of the reference with
    early_stopping=False); its rows, and the rows that found no continuation, are dead: cum = -inf.  With a SamplingPool a child's
    occurrence row is its parent's with the child's token counted, in the child's slots_out of the next step.  Nothing is read on the host."""
    G, W, K = state.n_groups, state.W, state.K
    if not all(isinstance(t, torch.Tensor) and tuple(t.shape) == (G, K) for t in (parent, token, score)):
        raise RuntimeError(f"parent, token and score must be [n_groups = {G}, K = {K}]")
    dev, inf = score.device, float("inf")
    with torch.no_grad():
        parent, token, score = parent.long(), token.long(), score.float()
        t = state.step.clamp(max=state.max_new_tokens - 1)
        length = (t + 1).float() ** state.length_penalty
        valid = parent >= 0
        eos = valid & (token.unsqueeze(2) == state.eos_ids.long().view(1, 1, -1)).any(2)
        # ---- the first W continuations, in candidate order
        cont = valid & ~eos
        nth = cont.cumsum(1)
        dest = torch.where(cont & (nth <= W), nth - 1, torch.full_like(nth, W))
        at = torch.full((G, W + 1), K, dtype=torch.long, device=dev).scatter_(1, dest, torch.arange(K, device=dev).expand(G, K))[:, :W]
        have = at < K
        at = at.clamp(max=K - 1)
        # ---- the hypothesis table: the old entries in front, so that a stable sort keeps them ahead of equal newcomers
        n_new = min(W, K)
        new_score = torch.where(eos[:, :n_new], score[:, :n_new] / length, torch.full_like(score[:, :n_new], -inf))
        both = torch.cat((state.hyp_score, new_score), 1)
        hyp_score, order = both.sort(dim=1, descending=True, stable=True)
        hyp_score, order = hyp_score[:, :W], order[:, :W]
        hyp_step = torch.cat((state.hyp_step, t.int().expand(G, n_new)), 1).gather(1, order)
        hyp_row = torch.cat((state.hyp_row, parent[:, :n_new].int()), 1).gather(1, order)
        best = score[:, 0]                                                      # -inf where the request has no candidate at all
        done = state.done | ((hyp_score[:, W - 1] > -inf) & (hyp_score[:, W - 1] >= best / length))
        # ---- the next rows
        alive = (have & ~done.unsqueeze(1)).reshape(-1)
        first_row = (torch.arange(G, device=dev) * W).unsqueeze(1)
        new_parent = torch.where(have, parent.gather(1, at), first_row.expand(G, W)).reshape(-1)
        new_token = torch.where(have, token.gather(1, at), torch.zeros_like(at)).reshape(-1)
        new_cum = torch.where(alive, score.gather(1, at).reshape(-1), torch.full((G * W,), -inf, device=dev))
        slots_in = state.slots_out[new_parent]
        slots_out = _beam_half(G, W, state.slot_base, (state.step + 1) % 2, dev)
        if sampling_pool is not None:
            occ = sampling_pool.occ
            rows = occ[state.slots_occ[new_parent].long()]
            rows.scatter_add_(1, new_token.unsqueeze(1), alive.float().unsqueeze(1))
            occ.index_copy_(0, slots_out.long(), rows)
        state.hist_parent.index_copy_(0, t.view(1), new_parent.int().unsqueeze(0))
        state.hist_token.index_copy_(0, t.view(1), torch.where(alive, new_token, torch.full_like(new_token, -1)).int().unsqueeze(0))
        state.hyp_score.copy_(hyp_score); state.hyp_step.copy_(hyp_step); state.hyp_row.copy_(hyp_row); state.done.copy_(done)
        state.tokens.copy_(new_token); state.cum.copy_(new_cum)
        state.slots_in.copy_(slots_in); state.slots_out.copy_(slots_out); state.slots_occ.copy_(slots_out)
        state.step.add_(1)
    return state


def beam_step_packed(emb, blocks, ln_out, head, state, pools, sampling_pool=None, pool_kernels=None, kernels=None):
    """One step of a beam search on every request of a serving batch: emb(tokens) -> step_packed (one token per row, slots = slots_in,
    out_slots = slots_out: the fork) -> ln_out -> head -> beam_candidates -> beam_advance.  Returns the step's candidates (parent, token,
    score).  sampling_pool: the repetition penalty of state.penalty on the tokens a beam has counted there (the prompt's counts in the
    prompt slot, if the caller put them there).  pool_kernels as in step_packed, kernels as in beam_candidates.  Nothing is read on the
    host, so the step can be captured in a graph and replayed; `state` carries everything from one replay to the next."""
    x = emb(state.tokens.clamp_min(0)).unsqueeze(0)
    x = step_packed(blocks, x, state.cu_tokens, 1, pools, state.slots_in, out_slots=state.slots_out, pool_kernels=pool_kernels)
    logits = head(ln_out(x[0]))
    penalised = sampling_pool is not None
    out = beam_candidates(logits, state.cum, state.cu_rows, state.K, pool=sampling_pool, slots=state.slots_occ if penalised else None,
                          penalty=state.penalty if penalised else None, kernels=kernels)
    beam_advance(state, *out, sampling_pool=sampling_pool)
    return out


def beam_finalize(state, n_return):
    """(sequences int32 [n_groups, n_return, max_new_tokens] padded with -1, lengths int32 [n_groups, n_return], scores fp32 [n_groups,
    n_return]), best first: of every request the n_return best of its finished hypotheses and its open beams together, as the reference
    pools them -- an open beam with cum / len^length_penalty, len the steps taken.  A hypothesis' sequence does not hold its eos, as in
    the reference.  Missing entries have score -inf and length 0.  The parent pointers are walked on the device."""
    G, W, T = state.n_groups, state.W, state.max_new_tokens
    dev, inf = state.cum.device, float("inf")
    with torch.no_grad():
        steps = state.step.clamp(max=T)
        open_score = state.cum.view(G, W) / steps.clamp_min(1).float() ** state.length_penalty
        score = torch.cat((state.hyp_score, open_score), 1)                                  # finished first: they win equal scores
        length = torch.cat((state.hyp_step.long(), steps.expand(G, W)), 1)
        row = torch.cat((state.hyp_row.long(), torch.arange(G * W, device=dev).view(G, W)), 1)
        score, order = score.sort(dim=1, descending=True, stable=True)
        n = min(n_return, 2 * W)
        score, order = score[:, :n], order[:, :n]
        missing = score == -inf
        length = length.gather(1, order).masked_fill(missing, 0)
        row = row.gather(1, order)
        seq = torch.full((G, n, T), -1, dtype=torch.int32, device=dev)
        for pos in range(T - 1, -1, -1):
            on = pos < length
            seq[:, :, pos] = torch.where(on, state.hist_token[pos][row], torch.full_like(row, -1).int())
            row = torch.where(on, state.hist_parent[pos][row].long(), row)
        if n < n_return:
            pad = n_return - n
            seq = torch.cat((seq, seq.new_full((G, pad, T), -1)), 1)
            length = torch.cat((length, length.new_zeros((G, pad))), 1)
            score = torch.cat((score, score.new_full((G, pad), -inf)), 1)
        return seq, length.int(), score
