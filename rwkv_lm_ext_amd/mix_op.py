"""Fused elementwise neighbours of the WKV6 operator in the RWKV-6 blocks, served by librwkv6_amd.so
(csrc/wkv6_mix.hip): the token-shift / data-dependent-lerp chain in front of the time-mix projections (src/model.py:435-448,
SURVEY.md row n4), the per-head GroupNorm + gate behind the operator (src/model.py:462-468, row n1), and the elementwise glue of
the channel-mix FFN (token shift + two lerps, squared ReLU, sigmoid gate: src/model.py:636-644); further down the packed serving and
training pieces, the last of them the LM-head cross-entropy with L2Wrap (ce_rows, ce_rows_grad_: csrc/wkv6_ce.hip).

bf16 GPU tensors only; like the operator itself there is no CPU path.  Each op is a torch.autograd.Function whose
forward and backward are one HIP kernel each; parameter gradients come back as fp32 partial rows summed here."""
import torch

from . import _lib
from ._args import _AT_LEAST_2, _call, _ints, _ptr, _ptrs          # same pointer / stream / checking conventions as the operator

_CU_SEQLENS = "cu_seqlens must be a contiguous int32 [n_seq + 1] tensor on the device of x"

_NPARTS = 1024


def _require(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.bfloat16):
        raise RuntimeError(f"{name} must be a bf16 GPU tensor (the fused time-mix ops have no CPU path)")
    return t.contiguous()


class _DDLerp(torch.autograd.Function):
    """out[s] = x + (shift(x) - x) * (maa[s] + m[s]);  x [B,T,C], maa [NS,C], m [NS,B,T,C] or None -> out [NS,B,T,C].
    rev_n (int32 [B] or None): the shift runs over the stream whose first rev_n[b] tokens are reversed."""

    @staticmethod
    def forward(ctx, x, maa, m, shifted0, rev_n):
        x, maa = _require(x, "x"), _require(maa, "maa")
        m = None if m is None else _require(m, "m")
        shifted0 = None if shifted0 is None else _require(shifted0, "shifted0")
        B, T, C = x.shape
        if rev_n is not None:
            _ints(rev_n, (B,), x.device, "rev_n must be a contiguous int32 [B] tensor on the device of x")
        NS = maa.shape[0]
        out = torch.empty((NS, B, T, C), device=x.device, dtype=x.dtype)
        _call("wkv6_ddlerp_rev_forward", "ddlerp forward", x.device, B, T, C, NS, *_ptrs(x, shifted0, m, maa, rev_n, out))
        ctx.save_for_backward(x, maa, m, shifted0, rev_n)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, maa, m, shifted0, rev_n = ctx.saved_tensors
        dout = _require(dout, "dout")
        B, T, C = x.shape
        NS = maa.shape[0]
        nparts = min(_NPARTS, B * T)
        dx = torch.empty_like(x)
        dm = None if m is None else torch.empty_like(m)
        part = torch.empty((nparts, NS, C), device=x.device, dtype=torch.float32)
        _call("wkv6_ddlerp_rev_backward", "ddlerp backward", x.device, B, T, C, NS, *_ptrs(x, shifted0, m, maa, rev_n, dout, dx, dm, part), nparts)
        dshift = None
        if shifted0 is not None and ctx.needs_input_grad[3]:
            # The token in front of the row (the infctx carry: the previous chunk's last token, src/model.py:1134-1190 passes the
            # shift states through torch_checkpoint without detaching them) enters only the stream's first token t0:
            # d shifted0[b] = sum_s dout[s,b,t0] (maa_s + m[s,b,t0]),  t0 = rev_n[b] - 1 where a reversed span starts the stream, else 0.
            if rev_n is None:
                d0 = dout[:, :, 0].float()
                m0 = None if m is None else m[:, :, 0].float()
            else:
                t0 = (rev_n.clamp(0, T).long() - 1).clamp_min(0).view(1, B, 1, 1).expand(NS, B, 1, C)
                d0 = dout.gather(2, t0)[:, :, 0].float()
                m0 = None if m is None else m.gather(2, t0)[:, :, 0].float()
            wgt = maa.float().view(NS, 1, C) + (0.0 if m0 is None else m0)
            dshift = (d0 * wgt).sum(0).to(shifted0.dtype)
        return dx, part.sum(0).to(maa.dtype), dm, dshift, None


class _DDLerpVarlen(torch.autograd.Function):
    """_DDLerp on a packed variable-length batch: x [1,total_T,C] (or [total_T,C]), m [NS,*x.shape] or None, cu_seqlens int32
    [n_seq + 1]; the token in front of sequence s is shifted0[s] ([n_seq,C], None: zero), never the last token of sequence s - 1.
    rev_n (int32 [n_seq], clamped to the sequence's length on the device, or None): the shift of sequence s is taken over the stream
    "its first rev_n[s] tokens reversed, the rest in place".  Without rev_n the plain entry points are called, not the rev ones with a
    null map."""

    @staticmethod
    def forward(ctx, x, maa, m, shifted0, cu_seqlens, rev_n):
        x, maa = _require(x, "x"), _require(maa, "maa")
        m = None if m is None else _require(m, "m")
        shifted0 = None if shifted0 is None else _require(shifted0, "shifted0")
        n_seq = _ints(cu_seqlens, _AT_LEAST_2, x.device, _CU_SEQLENS).numel() - 1
        C = x.shape[-1]
        total = x.numel() // C
        if x.dim() == 3 and x.shape[0] != 1:
            raise RuntimeError("a packed batch is [1, total_T, C] (or [total_T, C])")
        if shifted0 is not None and tuple(shifted0.shape) != (n_seq, C):
            raise RuntimeError(f"shifted0 must be [n_seq, C] = {(n_seq, C)}")
        if rev_n is not None:
            _ints(rev_n, (n_seq,), x.device, "rev_n must be a contiguous int32 [n_seq] tensor on the device of x")
        NS = maa.shape[0]
        out = torch.empty((NS,) + tuple(x.shape), device=x.device, dtype=x.dtype)
        if rev_n is None:
            _call("wkv6_ddlerp_varlen_forward", "ddlerp varlen forward", x.device, total, n_seq, C, NS, *_ptrs(cu_seqlens, x, shifted0, m, maa, out))
        else:
            _call("wkv6_ddlerp_varlen_rev_forward", "ddlerp varlen rev forward", x.device, total, n_seq, C, NS,
                  *_ptrs(cu_seqlens, x, shifted0, m, maa, rev_n, out))
        ctx.save_for_backward(x, maa, m, shifted0, cu_seqlens, rev_n)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, maa, m, shifted0, cu, rev_n = ctx.saved_tensors
        dout = _require(dout, "dout")
        C = x.shape[-1]
        total = x.numel() // C
        n_seq = cu.numel() - 1
        NS = maa.shape[0]
        nparts = min(_NPARTS, total)
        dx = torch.empty_like(x)
        dm = None if m is None else torch.empty_like(m)
        part = torch.empty((nparts, NS, C), device=x.device, dtype=torch.float32)
        if rev_n is None:
            _call("wkv6_ddlerp_varlen_backward", "ddlerp varlen backward", x.device, total, n_seq, C, NS,
                  *_ptrs(cu, x, shifted0, m, maa, dout, dx, dm, part), nparts)
        else:
            _call("wkv6_ddlerp_varlen_rev_backward", "ddlerp varlen rev backward", x.device, total, n_seq, C, NS,
                  *_ptrs(cu, x, shifted0, m, maa, rev_n, dout, dx, dm, part), nparts)
        dshift = None
        if shifted0 is not None and ctx.needs_input_grad[3]:
            # shifted0[s] enters only the stream's first token of a non-empty sequence s: cu[s] + rev_n[s] - 1 where a reversed span opens
            # the stream, else cu[s] (device index arithmetic only: nobody reads cu_seqlens or rev_n on the host).  The two forms agree on
            # every cu_seqlens the kernels accept and clamp a malformed one differently, so each keeps its own.
            if rev_n is None:
                first = cu[:-1].long().clamp(0, total - 1)
                alive = cu[1:] > cu[:-1]
            else:
                start = cu[:-1].long().clamp(0, total)
                length = (cu[1:].long().clamp(0, total) - start).clamp_min(0)
                nrev = torch.minimum(rev_n.long().clamp_min(0), length)
                first = (start + (nrev - 1).clamp_min(0)).clamp(0, total - 1)
                alive = length > 0
            d0 = dout.reshape(NS, total, C)[:, first].float()
            wgt = maa.float().view(NS, 1, C) + (0.0 if m is None else m.reshape(NS, total, C)[:, first].float())
            dshift = ((d0 * wgt) * alive.view(1, n_seq, 1).float()).sum(0).to(shifted0.dtype)
        return dx, part.sum(0).to(maa.dtype), dm, dshift, None, None


def ddlerp(x, maa, m=None, shifted0=None, rev_n=None, cu_seqlens=None):
    """maa: [NS,C] (or anything reshapeable to it, e.g. five [1,1,C] parameters stacked).  cu_seqlens (int32 [n_seq + 1]): x is a packed
    variable-length batch [1,total_T,C] and the shift does not cross a sequence boundary (shifted0 is then [n_seq,C]); rev_n is then
    int32 [n_seq]: the reversed span of every sequence's stream."""
    if cu_seqlens is not None:
        return _DDLerpVarlen.apply(x, maa.reshape(-1, x.shape[-1]), m, shifted0, cu_seqlens, rev_n)
    return _DDLerp.apply(x, maa.reshape(-1, x.shape[-1]), m, shifted0, rev_n)


# ---- the token-shift state of a serving loop as a device-side slot pool (include/wkv6_amd.h: wkv6_ddlerp_slots_forward, wkv6_shift_keep);
# inference only: no autograd.  Shapes and types are judged first, the device last (there is no CPU path).
def _check_ints(t, shape, name):
    """shape None: any 1-d length.  The device is judged by the caller, behind every shape."""
    _ints(t, shape, None, f"{name} must be a contiguous int32 {'1-d' if shape is None else list(shape)} tensor on the device of x")


def _check_packed(x, shift_pool, cu_seqlens):
    """(total_T, C, n_seq, n_slots) of a packed bf16 batch x [1,total_T,C] (or [total_T,C]) and a bf16 slot pool [n_slots,C]."""
    if not (isinstance(x, torch.Tensor) and x.dtype == torch.bfloat16 and x.dim() in (2, 3)):
        raise RuntimeError("x must be a bf16 tensor [1, total_T, C] (or [total_T, C])")
    if x.dim() == 3 and x.shape[0] != 1:
        raise RuntimeError("a packed batch is [1, total_T, C] (or [total_T, C])")
    C = x.shape[-1]
    if not (isinstance(shift_pool, torch.Tensor) and shift_pool.dtype == torch.bfloat16 and shift_pool.dim() == 2
            and shift_pool.shape[1] == C and shift_pool.is_contiguous()):
        raise RuntimeError(f"shift_pool must be a contiguous bf16 tensor [n_slots, C = {C}] (it is used in place, never copied)")
    return x.numel() // C, C, _ints(cu_seqlens, _AT_LEAST_2, None, _CU_SEQLENS).numel() - 1, shift_pool.shape[0]


def _check_gpu(x, shift_pool, cu_seqlens):
    if not x.is_cuda:
        raise RuntimeError("x must be on the GPU (the slot-pool kernels have no CPU path)")
    if shift_pool.device != x.device or cu_seqlens.device != x.device:
        raise RuntimeError("shift_pool and cu_seqlens must be on the device of x")


def ddlerp_slots(x, maa, m, shift_pool, slots, cu_seqlens):
    """ddlerp(x, maa, m, shifted0, cu_seqlens=cu_seqlens) with shifted0[s] = shift_pool[slots[s]] taken inside the kernel (zero where the
    slot lies outside the pool): no gather, the pool [n_slots,C] is only read.  slots: int32 [n_seq] or None (slot = sequence index,
    n_slots >= n_seq).  Inference only: raises when a gradient is required."""
    total, C, n_seq, n_slots = _check_packed(x, shift_pool, cu_seqlens)
    if not isinstance(maa, torch.Tensor) or maa.dtype != torch.bfloat16 or maa.numel() % C:
        raise RuntimeError("maa must be a bf16 tensor [NS, C]")
    maa = maa.reshape(-1, C).contiguous()
    NS = maa.shape[0]
    if m is not None and not (isinstance(m, torch.Tensor) and m.dtype == torch.bfloat16 and tuple(m.shape) == (NS,) + tuple(x.shape)):
        raise RuntimeError(f"m must be a bf16 tensor {[NS] + list(x.shape)} or None")
    if (NS, m is not None) not in ((1, False), (1, True), (5, True), (2, False)):
        raise RuntimeError("ddlerp_slots: supported are (NS = 1, m or not), (NS = 5, m), (NS = 2, no m)")
    if slots is None and n_slots < n_seq:
        raise RuntimeError("slots = None means slot = sequence index: the pool must hold n_seq slots")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, maa, m, shift_pool)):
        raise RuntimeError("ddlerp_slots has no backward: call it under torch.no_grad() (training uses ddlerp with shifted0)")
    if slots is not None:
        _check_ints(slots, (n_seq,), "slots")
    _check_gpu(x, shift_pool, cu_seqlens)
    if any(t is not None and t.device != x.device for t in (maa, m, slots)):
        raise RuntimeError("maa, m and slots must be on the device of x")
    x, m = x.contiguous(), None if m is None else m.contiguous()
    out = torch.empty((NS,) + tuple(x.shape), device=x.device, dtype=x.dtype)
    _call("wkv6_ddlerp_slots_forward", "ddlerp slots forward", x.device, total, n_seq, C, NS, *_ptrs(cu_seqlens, x, shift_pool), n_slots,
          *_ptrs(slots, m, maa, out))
    return out


def shift_keep(x, cu_seqlens, max_seqlen, shift_pool, slot_out, snap=None):
    """shift_pool[slot_out[s]] = the last served token of sequence s (token min(len_s, max_seqlen) - 1; empty sequences and slots outside
    the pool write nothing), and with snap = (snap_every, cu_snap, snap_slots) also shift_pool[snap_slots[cu_snap[s] + j]] = token
    (j + 1) * snap_every - 1 for every snapshot j the operator keeps.  One launch that writes only those rows of the pool, in place.
    slot_out: int32 [n_seq] or None (slot = sequence index)."""
    total, C, n_seq, n_slots = _check_packed(x, shift_pool, cu_seqlens)
    if isinstance(max_seqlen, bool) or not isinstance(max_seqlen, int) or max_seqlen < 1:
        raise RuntimeError("max_seqlen must be an int >= 1")
    if slot_out is None and n_slots < n_seq:
        raise RuntimeError("slot_out = None means slot = sequence index: the pool must hold n_seq slots")
    snap_every, cu_snap, snap_slots = (0, None, None) if snap is None else snap
    if isinstance(snap_every, bool) or not isinstance(snap_every, int) or snap_every < 0:
        raise RuntimeError("snap_every must be an int >= 0")
    if snap_every > 0:
        _check_ints(cu_snap, (n_seq + 1,), "cu_snap")
        _check_ints(snap_slots, None, "snap_slots")
    else:
        cu_snap = snap_slots = None
    if slot_out is not None:
        _check_ints(slot_out, (n_seq,), "slot_out")
    if shift_pool.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("shift_keep writes the pool in place and has no backward")
    _check_gpu(x, shift_pool, cu_seqlens)
    for t, name in ((slot_out, "slot_out"), (cu_snap, "cu_snap"), (snap_slots, "snap_slots")):
        if t is not None and t.device != x.device:
            raise RuntimeError(f"{name} must be a contiguous int32 tensor on the device of x")
    x, n_snap = x.contiguous(), 0 if snap_slots is None else snap_slots.numel()
    _call("wkv6_shift_keep", "shift keep", x.device, total, n_seq, min(max_seqlen, 0x7fffffff), C, *_ptrs(cu_seqlens, x, shift_pool), n_slots,
          _ptr(slot_out), snap_every, _ptr(cu_snap), _ptr(snap_slots), n_snap)


# ---- per-sequence LoRA adapters on a packed batch (include/wkv6_amd.h: wkv6_lora_packed_bf16); inference only: no autograd.  Shapes and
# types are judged first, the device last (there is no CPU path here: adapters.MultiLoraLinear has the eager one).
LORA_RANKS = (8, 16, 32, 64)


def lora_packed(x, y, A_pool, B_pool, scale, adapter, cu_seqlens):
    """y[t] += scale[a] * (bf16(x[t] A_pool[a]^T)) B_pool[a]^T for every row t of a sequence whose a = adapter[s] lies in the pool, in place
    on y (which holds the base GEMM's x W^T); every other row keeps its bits.  x bf16 [.., total_T, K] and y bf16 [.., total_T, N] (leading
    dimensions of size 1 only, as a packed batch has), A_pool bf16 [n_adapters, R, K], B_pool bf16 [n_adapters, N, R], scale fp32
    [n_adapters], adapter int32 [n_seq], cu_seqlens int32 [n_seq + 1]; R in LORA_RANKS.  Returns y.  The workspace is a torch tensor, so a
    graph capture owns it.  Raises when a gradient is required."""
    bf = torch.bfloat16
    if not (isinstance(x, torch.Tensor) and x.dtype == bf and x.dim() in (2, 3) and (x.dim() == 2 or x.shape[0] == 1) and x.is_contiguous()):
        raise RuntimeError("x must be a contiguous bf16 tensor [1, total_T, K] (or [total_T, K])")
    K, total = x.shape[-1], x.shape[-2]
    if not (isinstance(y, torch.Tensor) and y.dtype == bf and y.dim() == x.dim() and tuple(y.shape[:-1]) == tuple(x.shape[:-1])
            and y.is_contiguous()):
        raise RuntimeError(f"y must be a contiguous bf16 tensor {list(x.shape[:-1]) + ['N']} (it is updated in place, never copied)")
    N = y.shape[-1]
    if not (isinstance(A_pool, torch.Tensor) and A_pool.dtype == bf and A_pool.dim() == 3 and A_pool.shape[2] == K and A_pool.is_contiguous()):
        raise RuntimeError(f"A_pool must be a contiguous bf16 tensor [n_adapters, R, K = {K}]")
    n_adapters, R = A_pool.shape[0], A_pool.shape[1]
    if not (isinstance(B_pool, torch.Tensor) and B_pool.dtype == bf and tuple(B_pool.shape) == (n_adapters, N, R) and B_pool.is_contiguous()):
        raise RuntimeError(f"B_pool must be a contiguous bf16 tensor [n_adapters = {n_adapters}, N = {N}, R = {R}]")
    if not (isinstance(scale, torch.Tensor) and scale.dtype == torch.float32 and tuple(scale.shape) == (n_adapters,) and scale.is_contiguous()):
        raise RuntimeError(f"scale must be a contiguous fp32 tensor [n_adapters = {n_adapters}]")
    if R not in LORA_RANKS:
        raise RuntimeError(f"lora_packed: R must be one of {LORA_RANKS} (zero-pad a lower rank), got {R}")
    if total < 1 or n_adapters < 1 or K % 64 or N % 64 or not (64 <= K <= 16384 and 64 <= N <= 16384):
        raise RuntimeError("lora_packed: total_T and n_adapters must be >= 1, K and N multiples of 64 in [64, 16384]")
    n_seq = _ints(cu_seqlens, _AT_LEAST_2, None, _CU_SEQLENS).numel() - 1
    _check_ints(adapter, (n_seq,), "adapter")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, y, A_pool, B_pool, scale)):
        raise RuntimeError("lora_packed has no backward: call it under torch.no_grad() (adapters.MultiLoraLinear's eager path has autograd)")
    if not x.is_cuda:
        raise RuntimeError("x must be on the GPU (lora_packed has no CPU path)")
    if any(t.device != x.device for t in (y, A_pool, B_pool, scale, adapter, cu_seqlens)):
        raise RuntimeError("y, A_pool, B_pool, scale, adapter and cu_seqlens must be on the device of x")
    nbytes = _lib.load().wkv6_lora_packed_workspace_bytes(total, R)
    work = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    _call("wkv6_lora_packed_bf16", "lora packed", x.device, total, n_seq, K, N, R, n_adapters,
          *_ptrs(cu_seqlens, adapter, x, A_pool, B_pool, scale, y, work), nbytes)
    return y


# ---- the two low-rank pairs in front of the time-mix projections (include/wkv6_amd.h: wkv6_tmix_lerp_lowrank_bf16,
# wkv6_decay_lowrank_bf16); inference only: no autograd.  Shapes and types are judged first, the device last (there is no CPU path here:
# callers.Tmix_x060.jit_func has the eager one).
LOWRANK_D = (32, 64)           # TIME_MIX_EXTRA_DIM the kernels have
LOWRANK_DD = (64, 128)         # TIME_DECAY_EXTRA_DIM


def _bf16_shape(t, shape):
    return isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16 and tuple(t.shape) == tuple(shape) and t.is_contiguous()


def _lowrank_work(dev, rows, d_total):
    nbytes = _lib.load().wkv6_lowrank_workspace_bytes(rows, d_total)
    return torch.empty(nbytes, device=dev, dtype=torch.uint8), nbytes


def tmix_inputs(x, maa_x, W1t, W2t, maa5, cu_seqlens=None, shifted0=None, shift_pool=None, slots=None):
    """The five inputs xw, xk, xv, xr, xg of an RWKV-6 time-mix layer, bf16 [5, *x.shape], in two launches:
    x + (xp - x) * (maa5[s] + tanh((x + (xp - x) * maa_x) @ W1) [s] @ W2[s]), xp the token in front; the operation and its rounding points
    are stated in include/wkv6_amd.h.  x bf16 [B, T, C] (dense; shifted0 [B, C] or None: the token in front of every batch row), or with
    cu_seqlens (int32 [n_seq + 1]) a packed batch [1, total_T, C] (or [total_T, C]) with either shifted0 [n_seq, C] or shift_pool bf16
    [n_slots, C] and slots (int32 [n_seq], None: the sequence index), as ddlerp_slots takes them.  maa_x bf16 [C] (any shape of C elements),
    maa5 bf16 [5, C], W1t bf16 [5 D, C] and W2t bf16 [5, C, D]: time_maa_w1 and time_maa_w2 in nn.Linear layout; D in LOWRANK_D.  The workspace
    is a torch tensor, so a graph capture owns it.  Raises when a gradient is required."""
    bf = torch.bfloat16
    if not (isinstance(x, torch.Tensor) and x.dtype == bf and x.dim() in (2, 3) and x.is_contiguous()):
        raise RuntimeError("x must be a contiguous bf16 tensor [B, T, C] (packed: [1, total_T, C] or [total_T, C])")
    C = x.shape[-1]
    total = x.numel() // max(C, 1)
    if cu_seqlens is None:
        if x.dim() != 3:
            raise RuntimeError("x must be a contiguous bf16 tensor [B, T, C] (packed: [1, total_T, C] or [total_T, C])")
        n_seq = x.shape[0]
    else:
        if x.dim() == 3 and x.shape[0] != 1:
            raise RuntimeError("a packed batch is [1, total_T, C] (or [total_T, C])")
        n_seq = _ints(cu_seqlens, _AT_LEAST_2, None, _CU_SEQLENS).numel() - 1
    if not (isinstance(maa_x, torch.Tensor) and maa_x.dtype == bf and maa_x.numel() == C and maa_x.is_contiguous()):
        raise RuntimeError(f"maa_x must be a contiguous bf16 tensor of C = {C} elements")
    if not (isinstance(W1t, torch.Tensor) and W1t.dtype == bf and W1t.dim() == 2 and W1t.shape[1] == C and W1t.shape[0] % 5 == 0
            and W1t.is_contiguous()):
        raise RuntimeError(f"W1t must be a contiguous bf16 tensor [5 D, C = {C}] (time_maa_w1 transposed)")
    D = W1t.shape[0] // 5
    if not _bf16_shape(W2t, (5, C, D)):
        raise RuntimeError(f"W2t must be a contiguous bf16 tensor [5, C = {C}, D = {D}] (time_maa_w2 with its last two dimensions transposed)")
    if not _bf16_shape(maa5, (5, C)):
        raise RuntimeError(f"maa5 must be a contiguous bf16 tensor [5, C = {C}]")
    if D not in LOWRANK_D:
        raise RuntimeError(f"tmix_inputs: D must be one of {LOWRANK_D}, got {D}")
    if total < 1 or n_seq < 1 or C % 64 or not 64 <= C <= 4096:
        raise RuntimeError("tmix_inputs: x must hold at least one row, C a multiple of 64 in [64, 4096]")
    if shifted0 is not None and shift_pool is not None:
        raise RuntimeError("shifted0 and shift_pool exclude each other")
    if shift_pool is not None and cu_seqlens is None:
        raise RuntimeError("shift_pool / slots belong to a packed batch (cu_seqlens)")
    if slots is not None and shift_pool is None:
        raise RuntimeError("slots name rows of shift_pool")
    front = shifted0 if shift_pool is None else shift_pool
    if shifted0 is not None and not _bf16_shape(shifted0, (n_seq, C)):
        raise RuntimeError(f"shifted0 must be a contiguous bf16 tensor [n_seq, C] = {[n_seq, C]}")
    if shift_pool is not None:
        if not (isinstance(shift_pool, torch.Tensor) and shift_pool.dtype == bf and shift_pool.dim() == 2 and shift_pool.shape[0] >= 1
                and shift_pool.shape[1] == C and shift_pool.is_contiguous()):
            raise RuntimeError(f"shift_pool must be a contiguous bf16 tensor [n_slots, C = {C}] (it is used in place, never copied)")
        if slots is None and shift_pool.shape[0] < n_seq:
            raise RuntimeError("slots = None means slot = sequence index: the pool must hold n_seq slots")
        if slots is not None:
            _check_ints(slots, (n_seq,), "slots")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, maa_x, W1t, W2t, maa5, front)):
        raise RuntimeError("tmix_inputs has no backward: call it under torch.no_grad() (training uses ddlerp and the torch matmuls)")
    if not x.is_cuda:
        raise RuntimeError("x must be on the GPU (tmix_inputs has no CPU path)")
    if any(t is not None and t.device != x.device for t in (maa_x, W1t, W2t, maa5, cu_seqlens, front, slots)):
        raise RuntimeError("maa_x, W1t, W2t, maa5, cu_seqlens, shifted0, shift_pool and slots must be on the device of x")
    out = torch.empty((5,) + tuple(x.shape), device=x.device, dtype=bf)
    work, nbytes = _lowrank_work(x.device, total, 5 * D)
    _call("wkv6_tmix_lerp_lowrank_bf16", "tmix lerp lowrank", x.device, total, n_seq, C, D, *_ptrs(cu_seqlens, x, front),
          0 if front is None else front.shape[0], *_ptrs(slots, maa_x, W1t, W2t, maa5, out, work), nbytes)
    return out


def decay_lowrank(xw, D1t, D2t, time_decay):
    """w = time_decay + tanh(xw @ D1) @ D2 in two launches, bf16 [*xw.shape[:-1], N]; the operation and its rounding points are stated in
    include/wkv6_amd.h.  xw bf16 [.., C], D1t bf16 [Dd, C] and D2t bf16 [N, Dd]: time_decay_w1 and time_decay_w2 in nn.Linear layout, Dd in
    LOWRANK_DD; time_decay bf16 of N elements.  The workspace is a torch tensor, so a graph capture owns it.  Raises when a gradient is
    required."""
    bf = torch.bfloat16
    if not (isinstance(xw, torch.Tensor) and xw.dtype == bf and xw.dim() >= 2 and xw.is_contiguous()):
        raise RuntimeError("xw must be a contiguous bf16 tensor [.., rows, C]")
    C = xw.shape[-1]
    rows = xw.numel() // max(C, 1)
    if not (isinstance(D1t, torch.Tensor) and D1t.dtype == bf and D1t.dim() == 2 and D1t.shape[1] == C and D1t.is_contiguous()):
        raise RuntimeError(f"D1t must be a contiguous bf16 tensor [Dd, C = {C}] (time_decay_w1 transposed)")
    Dd = D1t.shape[0]
    if not (isinstance(D2t, torch.Tensor) and D2t.dtype == bf and D2t.dim() == 2 and D2t.shape[1] == Dd and D2t.is_contiguous()):
        raise RuntimeError(f"D2t must be a contiguous bf16 tensor [N, Dd = {Dd}] (time_decay_w2 transposed)")
    N = D2t.shape[0]
    if not (isinstance(time_decay, torch.Tensor) and time_decay.dtype == bf and time_decay.numel() == N and time_decay.is_contiguous()):
        raise RuntimeError(f"time_decay must be a contiguous bf16 tensor of N = {N} elements")
    if Dd not in LOWRANK_DD:
        raise RuntimeError(f"decay_lowrank: Dd must be one of {LOWRANK_DD}, got {Dd}")
    if rows < 1 or C % 64 or N % 64 or not (64 <= C <= 4096 and 64 <= N <= 4096):
        raise RuntimeError("decay_lowrank: xw must hold at least one row, C and N multiples of 64 in [64, 4096]")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (xw, D1t, D2t, time_decay)):
        raise RuntimeError("decay_lowrank has no backward: call it under torch.no_grad() (training uses the torch matmuls)")
    if not xw.is_cuda:
        raise RuntimeError("xw must be on the GPU (decay_lowrank has no CPU path)")
    if any(t.device != xw.device for t in (D1t, D2t, time_decay)):
        raise RuntimeError("D1t, D2t and time_decay must be on the device of xw")
    w = torch.empty(tuple(xw.shape[:-1]) + (N,), device=xw.device, dtype=bf)
    work, nbytes = _lowrank_work(xw.device, rows, Dd)
    _call("wkv6_decay_lowrank_bf16", "decay lowrank", xw.device, rows, C, Dd, N, *_ptrs(xw, D1t, D2t, time_decay, w, work), nbytes)
    return w


# ---- device-side token sampling with a penalty slot pool (include/wkv6_amd.h: rwkv6_sample_slots_*); inference only: no autograd.  Shapes
# and types are judged first, the device last (there is no CPU path here: infctx.sample_packed has the eager one).
SAMPLE_MAX_VOCAB = 65536
_SAMPLE_ENTRY = {torch.bfloat16: "rwkv6_sample_slots_bf16", torch.float16: "rwkv6_sample_slots_fp16", torch.float32: "rwkv6_sample_slots_fp32"}


def _rows_in_storage(t, ld):
    """Whether every row of the 2-d view t may be read up to the next multiple of 8 columns (the kernel's 16-byte accesses)."""
    last = t.storage_offset() + (t.shape[0] - 1) * ld + (t.shape[1] + 7) // 8 * 8
    return last * t.element_size() <= t.untyped_storage().nbytes()


def sample_slots(logits, occ_pool, slots, params, u, out_slots=None, want_logprob=False):
    """One token per row of logits [n_seq, V] (bf16, fp16 or fp32; a view of the first V columns of a contiguous [n_seq, ld] tensor, ld % 8
    == 0, is taken as it is), every sequence with its own params[s] = (temperature, top_p, top_k, alpha_presence, alpha_frequency,
    alpha_decay, repetition_penalty, 0) and uniform draw u[s]; the operation is stated in include/wkv6_amd.h.  occ_pool fp32 [n_slots, ld]
    (or a view of the first V columns of one) holds the sequences' decaying occurrence counts: row slots[s] is read (slots None: row s), row
    out_slots[s] (None: the same row) is written, in place.  Returns tokens int32 [n_seq], with want_logprob (tokens, logprob fp32 [n_seq]);
    a poisoned row gives -1 and NaN.  Nothing is read on the host.  Raises when a gradient is required."""
    if not (isinstance(logits, torch.Tensor) and logits.dtype in _SAMPLE_ENTRY and logits.dim() == 2 and logits.shape[0] >= 1
            and logits.shape[1] >= 1 and logits.stride(1) == 1):
        raise RuntimeError("logits must be a bf16, fp16 or fp32 tensor [n_seq, V] with unit stride along V")
    n_seq, V = logits.shape
    ld = logits.stride(0)
    if ld < V or ld % 8 or not _rows_in_storage(logits, ld):
        raise RuntimeError(f"logits rows must lie ld elements apart in memory, ld a multiple of 8 and >= V = {V}: pass the first V columns "
                           f"of a padded [n_seq, ld] tensor (INTEGRATION.md), got a row stride of {ld}")
    if V > SAMPLE_MAX_VOCAB:
        raise RuntimeError(f"sample_slots: V must be at most {SAMPLE_MAX_VOCAB}, got {V}")
    if not (isinstance(occ_pool, torch.Tensor) and occ_pool.dtype == torch.float32 and occ_pool.dim() == 2 and occ_pool.shape[0] >= 1
            and occ_pool.shape[1] == V and occ_pool.stride(1) == 1 and occ_pool.stride(0) == ld and _rows_in_storage(occ_pool, ld)):
        raise RuntimeError(f"occ_pool must be an fp32 tensor [n_slots, V = {V}] whose rows lie ld = {ld} elements apart, as the rows of "
                           "logits do (it is used in place, never copied)")
    n_slots = occ_pool.shape[0]
    if not (isinstance(params, torch.Tensor) and params.dtype == torch.float32 and tuple(params.shape) == (n_seq, 8) and params.is_contiguous()):
        raise RuntimeError(f"params must be a contiguous fp32 tensor [n_seq = {n_seq}, 8]")
    if not (isinstance(u, torch.Tensor) and u.dtype == torch.float32 and tuple(u.shape) == (n_seq,) and u.is_contiguous()):
        raise RuntimeError(f"u must be a contiguous fp32 tensor [n_seq = {n_seq}]")
    if slots is None and n_slots < n_seq:
        raise RuntimeError("slots = None means slot = sequence index: the pool must hold n_seq slots")
    if slots is not None:
        _check_ints(slots, (n_seq,), "slots")
    if out_slots is not None:
        _check_ints(out_slots, (n_seq,), "out_slots")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (logits, occ_pool, params, u)):
        raise RuntimeError("sample_slots has no backward: call it under torch.no_grad()")
    if not logits.is_cuda:
        raise RuntimeError("logits must be on the GPU (sample_slots has no CPU path: infctx.sample_packed has the eager one)")
    if any(t is not None and t.device != logits.device for t in (occ_pool, params, u, slots, out_slots)):
        raise RuntimeError("occ_pool, params, u, slots and out_slots must be on the device of logits")
    if logits.data_ptr() % 16 or occ_pool.data_ptr() % 16:
        raise RuntimeError("logits and occ_pool must be 16-byte aligned")
    tokens = torch.empty(n_seq, device=logits.device, dtype=torch.int32)
    logprob = torch.empty(n_seq, device=logits.device, dtype=torch.float32) if want_logprob else None
    _call(_SAMPLE_ENTRY[logits.dtype], "sample slots", logits.device, n_seq, V, ld, *_ptrs(logits, occ_pool), n_slots,
          *_ptrs(slots, out_slots, params, u, tokens, logprob))
    return (tokens, logprob) if want_logprob else tokens


# ---- beam-search candidates on rows of logits (include/wkv6_amd.h: rwkv6_beam_candidates_*); inference only: no autograd.  Shapes and types
# are judged first, the device last (there is no CPU path here: infctx.beam_candidates has the eager one).
BEAM_MAX_K = 64
_BEAM_ENTRY = {torch.bfloat16: "rwkv6_beam_candidates_bf16", torch.float16: "rwkv6_beam_candidates_fp16",
               torch.float32: "rwkv6_beam_candidates_fp32"}


def beam_candidates(logits, cum, cu_rows, K, occ_pool=None, slots=None, penalty=None):
    """(parent int32, token int32, score fp32), each [n_groups, K]: for every group g of rows cu_rows[g] .. cu_rows[g+1] - 1 of logits
    [n_rows, V] (bf16, fp16 or fp32; a view of the first V columns of a contiguous [n_rows, ld] tensor, ld % 8 == 0, is taken as it is) the
    K best (row, token) by cum[row] + log_softmax(logits[row])[token], best first, ties by row and then token; missing entries are -1, -1,
    -inf.  A row with cum == -inf is dead and is not read.  occ_pool fp32 [n_slots, V] (rows ld apart, as the sampler's) with penalty fp32
    [n_groups] applies the repetition penalty to the log-probabilities of the tokens that row slots[r] (slots None: row r) counts.  The
    operation is stated in include/wkv6_amd.h.  Nothing is read on the host.  Raises when a gradient is required."""
    if not (isinstance(logits, torch.Tensor) and logits.dtype in _BEAM_ENTRY and logits.dim() == 2 and logits.shape[0] >= 1
            and logits.shape[1] >= 1 and logits.stride(1) == 1):
        raise RuntimeError("logits must be a bf16, fp16 or fp32 tensor [n_rows, V] with unit stride along V")
    n_rows, V = logits.shape
    ld = logits.stride(0)
    if ld < V or ld % 8 or not _rows_in_storage(logits, ld):
        raise RuntimeError(f"logits rows must lie ld elements apart in memory, ld a multiple of 8 and >= V = {V}: pass the first V columns "
                           f"of a padded [n_rows, ld] tensor (INTEGRATION.md), got a row stride of {ld}")
    if V > SAMPLE_MAX_VOCAB:
        raise RuntimeError(f"beam_candidates: V must be at most {SAMPLE_MAX_VOCAB}, got {V}")
    if not (isinstance(K, int) and 1 <= K <= BEAM_MAX_K):
        raise RuntimeError(f"K must be an int in [1, {BEAM_MAX_K}], got {K!r}")
    if not (isinstance(cum, torch.Tensor) and cum.dtype == torch.float32 and tuple(cum.shape) == (n_rows,) and cum.is_contiguous()):
        raise RuntimeError(f"cum must be a contiguous fp32 tensor [n_rows = {n_rows}]")
    _ints(cu_rows, _AT_LEAST_2, None, "cu_rows must be a contiguous int32 tensor [n_groups + 1]")
    n_groups = cu_rows.numel() - 1
    if (occ_pool is None) != (penalty is None) or (slots is not None and occ_pool is None):
        raise RuntimeError("occ_pool and penalty go together (both None: no penalty), and slots needs them")
    n_slots = 0
    if occ_pool is not None:
        if not (isinstance(occ_pool, torch.Tensor) and occ_pool.dtype == torch.float32 and occ_pool.dim() == 2 and occ_pool.shape[0] >= 1
                and occ_pool.shape[1] == V and occ_pool.stride(1) == 1 and occ_pool.stride(0) == ld and _rows_in_storage(occ_pool, ld)):
            raise RuntimeError(f"occ_pool must be an fp32 tensor [n_slots, V = {V}] whose rows lie ld = {ld} elements apart, as the rows of "
                               "logits do (it is used in place, never copied)")
        n_slots = occ_pool.shape[0]
        if not (isinstance(penalty, torch.Tensor) and penalty.dtype == torch.float32 and tuple(penalty.shape) == (n_groups,)
                and penalty.is_contiguous()):
            raise RuntimeError(f"penalty must be a contiguous fp32 tensor [n_groups = {n_groups}]")
        if slots is None and n_slots < n_rows:
            raise RuntimeError("slots = None means slot = row index: the pool must hold n_rows slots")
        if slots is not None:
            _check_ints(slots, (n_rows,), "slots")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (logits, cum, occ_pool, penalty)):
        raise RuntimeError("beam_candidates has no backward: call it under torch.no_grad()")
    if not logits.is_cuda:
        raise RuntimeError("logits must be on the GPU (beam_candidates has no CPU path: infctx.beam_candidates has the eager one)")
    if any(t is not None and t.device != logits.device for t in (cum, cu_rows, occ_pool, slots, penalty)):
        raise RuntimeError("cum, cu_rows, occ_pool, slots and penalty must be on the device of logits")
    if logits.data_ptr() % 16 or (occ_pool is not None and occ_pool.data_ptr() % 16):
        raise RuntimeError("logits and occ_pool must be 16-byte aligned")
    dev = logits.device
    parent, token = (torch.empty((n_groups, K), device=dev, dtype=torch.int32) for _ in range(2))
    score = torch.empty((n_groups, K), device=dev, dtype=torch.float32)
    ws_bytes = _lib.load().rwkv6_beam_candidates_workspace_bytes(n_rows, K)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    _call(_BEAM_ENTRY[logits.dtype], "beam candidates", dev, n_rows, V, ld, *_ptrs(logits, cum), n_groups, _ptr(cu_rows), K, _ptr(occ_pool),
          n_slots, *_ptrs(slots, penalty, parent, token, score, ws), ws_bytes)
    return parent, token, score


# ---- sentence pooling on a packed batch (include/wkv6_amd.h: wkv6_pool_packed_*); bf16, GPU, with a backward.  Shapes and types are judged
# first, the device last (there is no CPU path here: callers.pooling_packed has the eager one).
class _PoolPacked(torch.autograd.Function):
    """out [n_seq,C] of x [total_T,C] (checked by pool_packed); gx is written whole by the backward kernel, the +0 rows included."""

    @staticmethod
    def forward(ctx, x, cu_seqlens, actual_len, kind):
        C = x.shape[-1]
        total, n_seq = x.numel() // C, cu_seqlens.numel() - 1
        out = torch.empty((n_seq, C), device=x.device, dtype=x.dtype)
        _call("wkv6_pool_packed_forward", "pool packed forward", x.device, total, n_seq, C, kind, *_ptrs(cu_seqlens, actual_len, x, out))
        ctx.save_for_backward(cu_seqlens, actual_len)
        ctx.kind, ctx.shape = kind, x.shape
        return out

    @staticmethod
    def backward(ctx, gout):
        cu_seqlens, actual_len = ctx.saved_tensors
        gout = _require(gout, "gout")
        C = ctx.shape[-1]
        gx = torch.empty(ctx.shape, device=gout.device, dtype=gout.dtype)
        _call("wkv6_pool_packed_backward", "pool packed backward", gout.device, gx.numel() // C, cu_seqlens.numel() - 1, C, ctx.kind,
              *_ptrs(cu_seqlens, actual_len, gout, gx))
        return gx, None, None, None


def pool_packed(x, cu_seqlens, actual_len=None, kind="weightedmean"):
    """One vector per sequence of the packed bf16 batch x [1,total_T,C] (or [total_T,C], C a multiple of 8) -> bf16 [n_seq,C]: kind
    "weightedmean", "lasttoken" or "avg" of RwkvForSequenceEmbedding.pooling at a_s = clamp(actual_len[s], 0, len_s - 1) (actual_len int32
    [n_seq]: the position of the sequence's first emb_id token; None: its last token); the operation, its clamping rule and the rows the
    backward writes as +0 are stated in include/wkv6_amd.h.  Nothing is read on the host."""
    if not (isinstance(x, torch.Tensor) and x.dtype == torch.bfloat16 and x.dim() in (2, 3)):
        raise RuntimeError("x must be a bf16 tensor [1, total_T, C] (or [total_T, C])")
    if x.dim() == 3 and x.shape[0] != 1:
        raise RuntimeError("a packed batch is [1, total_T, C] (or [total_T, C])")
    C = x.shape[-1]
    if C < 8 or C % 8 or x.numel() < C:
        raise RuntimeError(f"pool_packed: C must be a multiple of 8 and total_T >= 1, got x {list(x.shape)}")
    if kind not in _lib.POOL_KINDS:
        raise RuntimeError(f"pool_packed: kind must be one of {sorted(_lib.POOL_KINDS)}, got {kind!r}")
    n_seq = _ints(cu_seqlens, _AT_LEAST_2, None, _CU_SEQLENS).numel() - 1
    if actual_len is not None:
        _check_ints(actual_len, (n_seq,), "actual_len")
    if not x.is_cuda:
        raise RuntimeError("x must be on the GPU (pool_packed has no CPU path: callers.pooling_packed has the eager one)")
    if cu_seqlens.device != x.device or (actual_len is not None and actual_len.device != x.device):
        raise RuntimeError("cu_seqlens and actual_len must be on the device of x")
    return _PoolPacked.apply(x.contiguous(), cu_seqlens, actual_len, _lib.POOL_KINDS[kind])


# ---- LM-head cross-entropy with L2Wrap on rows of logits (include/wkv6_amd.h: wkv6_ce_rows_*); bf16, fp16 or fp32 on the GPU, with a
# backward.  Shapes and types are judged first, the device last (there is no CPU path here: callers.lm_loss has the eager one).
_CE_ENTRY = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}


def _ce_ld(logits):
    """The row stride the kernels take logits [n_rows, V] with (one row: V rounded up to 8), or None where the layout does not serve them:
    rows ld elements apart, ld a multiple of 8 and >= V, every row readable up to the next multiple of 8 columns."""
    n_rows, V = logits.shape
    ld = logits.stride(0) if n_rows > 1 else (V + 7) // 8 * 8
    return ld if ld >= V and ld % 8 == 0 and _rows_in_storage(logits, ld) else None


def _check_ce(logits, targets, scales):
    """(n_rows, V, ld) of logits [n_rows, V] (a view of the first V columns of a contiguous [n_rows, ld] tensor is taken as it is), int64
    targets [n_rows] and the fp32 [n_rows] arrays of `scales` (name -> tensor or None)."""
    if not (isinstance(logits, torch.Tensor) and logits.dtype in _CE_ENTRY and logits.dim() == 2 and logits.shape[0] >= 1
            and logits.shape[1] >= 1 and logits.stride(1) == 1):
        raise RuntimeError("logits must be a bf16, fp16 or fp32 tensor [n_rows, V] with unit stride along V")
    n_rows, V = logits.shape
    ld = _ce_ld(logits)
    if ld is None:
        raise RuntimeError(f"logits rows must lie ld elements apart in memory, ld a multiple of 8 and >= V = {V}: pass the first V columns "
                           f"of a padded [n_rows, ld] tensor (INTEGRATION.md), got a row stride of {logits.stride(0)}")
    if not (isinstance(targets, torch.Tensor) and targets.dtype == torch.int64 and tuple(targets.shape) == (n_rows,) and targets.is_contiguous()):
        raise RuntimeError(f"targets must be a contiguous int64 tensor [n_rows = {n_rows}]")
    for name, t in scales.items():
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and tuple(t.shape) == (n_rows,) and t.is_contiguous()):
            raise RuntimeError(f"{name} must be a contiguous fp32 tensor [n_rows = {n_rows}]")
    if not logits.is_cuda:
        raise RuntimeError("logits must be on the GPU (ce_rows has no CPU path: callers.lm_loss has the eager one)")
    if any(t is not None and t.device != logits.device for t in (targets, *scales.values())):
        raise RuntimeError("targets and the scales must be on the device of logits")
    if logits.data_ptr() % 16:
        raise RuntimeError("logits must be 16-byte aligned")
    return n_rows, V, ld


def _ce_stats(logits):
    n, dev = logits.shape[0], logits.device
    f = torch.empty((3, n), device=dev, dtype=torch.float32)
    return f[0], f[1], f[2], torch.empty(n, device=dev, dtype=torch.int32)


class _CeRows(torch.autograd.Function):
    """loss_row of checked logits; the backward is one kernel with ce_scale = the incoming gradient.  As in the reference's L2Wrap the L2
    term is not multiplied by it."""

    @staticmethod
    def forward(ctx, logits, targets, l2_scale, dims):
        n_rows, V, ld = dims
        loss, lse, zmax, imax = _ce_stats(logits)
        _call("wkv6_ce_rows_forward_" + _CE_ENTRY[logits.dtype], "ce rows forward", logits.device, n_rows, V, ld,
              *_ptrs(logits, targets, loss, lse, zmax, imax, None, None, None), 0)
        ctx.save_for_backward(logits, targets, lse, zmax, imax, l2_scale)
        ctx.dims = dims
        return loss

    @staticmethod
    def backward(ctx, gloss):
        logits, targets, lse, zmax, imax, l2_scale = ctx.saved_tensors
        n_rows, V, ld = ctx.dims
        if l2_scale is None:
            l2_scale = torch.zeros(n_rows, device=logits.device, dtype=torch.float32)
        ce_scale = gloss.float().contiguous()
        ld_g = (V + 7) // 8 * 8
        g = torch.empty((n_rows, ld_g), device=logits.device, dtype=logits.dtype)
        _call("wkv6_ce_rows_backward_" + _CE_ENTRY[logits.dtype], "ce rows backward", logits.device, n_rows, V, ld,
              *_ptrs(logits, targets, lse, zmax, imax, ce_scale, l2_scale, g), ld_g)
        return g[:, :V], None, None, None


def ce_rows(logits, targets, l2_scale=None):
    """loss_row fp32 [n_rows] = logsumexp(logits[r]) - logits[r, targets[r]] (+0 where targets[r] == -100) of logits [n_rows, V] (bf16, fp16
    or fp32; rows ld elements apart, ld % 8 == 0) and int64 targets; the operation is stated in include/wkv6_amd.h.  Differentiable in
    logits: the gradient is gloss_row[r] * (softmax - onehot) plus, with l2_scale (fp32 [n_rows]), the L2Wrap term l2_scale[r] * max at
    the row's argmax, which is NOT multiplied by the incoming gradient (src/model.py:960-974).  Nothing is read on the host."""
    dims = _check_ce(logits, targets, {"l2_scale": l2_scale})
    return _CeRows.apply(logits, targets, l2_scale, dims)


def ce_rows_grad_(logits, targets, ce_scale, l2_scale):
    """The fused mode: one launch that OVERWRITES logits with the gradient ce_scale[r] * (softmax - onehot) + l2_scale[r] * max at the
    argmax and returns loss_row fp32 [n_rows]; for a caller that knows its scales before it has any loss (callers.head_loss).  No
    autograd: raises when a gradient is required."""
    dims = _check_ce(logits, targets, {"ce_scale": ce_scale, "l2_scale": l2_scale})
    if ce_scale is None or l2_scale is None:
        raise RuntimeError("ce_rows_grad_ needs ce_scale and l2_scale (fp32 [n_rows])")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (logits, ce_scale, l2_scale)):
        raise RuntimeError("ce_rows_grad_ overwrites logits and has no backward: call it under torch.no_grad() (ce_rows has autograd)")
    n_rows, V, ld = dims
    loss, lse, zmax, imax = _ce_stats(logits)
    _call("wkv6_ce_rows_forward_" + _CE_ENTRY[logits.dtype], "ce rows fused", logits.device, n_rows, V, ld,
          *_ptrs(logits, targets, loss, lse, zmax, imax, ce_scale, l2_scale, logits), ld)
    return loss


def gn_gate_forward(y, g, gamma, beta, H, eps):
    """(out, stats): out = GroupNorm_H(y) * g on [rows, C]; stats fp32 [rows, H, 2] = mean, rstd (for gn_gate_backward)."""
    y, g, gamma, beta = _require(y, "y"), _require(g, "g"), _require(gamma, "gamma"), _require(beta, "beta")
    C = y.shape[-1]
    rows = y.numel() // C
    out = torch.empty_like(y)
    stats = torch.empty((rows, H, 2), device=y.device, dtype=torch.float32)
    _call("wkv6_gn_gate_forward", "gn_gate forward", y.device, rows, C, H, *_ptrs(y, g, gamma, beta), float(eps), _ptr(out), _ptr(stats))
    return out, stats


def gn_gate_backward(y, g, gamma, beta, stats, dout, H):
    """(dy, dg, dgamma, dbeta) of gn_gate_forward; the parameter gradients are summed from fp32 per-workgroup partial rows."""
    dout = _require(dout, "dout")
    C = y.shape[-1]
    rows = y.numel() // C
    nparts = min(_NPARTS, rows)
    dy, dg = torch.empty_like(y), torch.empty_like(g)
    pg = torch.empty((nparts, C), device=y.device, dtype=torch.float32)
    pb = torch.empty((nparts, C), device=y.device, dtype=torch.float32)
    _call("wkv6_gn_gate_backward", "gn_gate backward", y.device, rows, C, H, *_ptrs(y, g, gamma, beta, stats, dout, dy, dg, pg, pb), nparts)
    return dy, dg, pg.sum(0).to(gamma.dtype), pb.sum(0).to(beta.dtype)


class _GroupNormGate(torch.autograd.Function):
    """out = GroupNorm_H(y) * g  on [rows, C] with C = 64 H."""

    @staticmethod
    def forward(ctx, y, g, gamma, beta, H, eps):
        out, stats = gn_gate_forward(y, g, gamma, beta, H, eps)
        ctx.save_for_backward(_require(y, "y"), _require(g, "g"), gamma, beta, stats)
        ctx.H = H
        return out

    @staticmethod
    def backward(ctx, dout):
        y, g, gamma, beta, stats = ctx.saved_tensors
        return gn_gate_backward(y, g, gamma, beta, stats, dout, ctx.H) + (None, None)


def group_norm_gate(y, g, gamma, beta, n_head, eps):
    return _GroupNormGate.apply(y, g, gamma, beta, n_head, eps)


class _SqRelu(torch.autograd.Function):
    """relu(x)^2 (src/model.py:640-641) in one pass; one rounding where the eager form rounds relu and the square separately (relu is
    exact, so the results are identical)."""

    @staticmethod
    def forward(ctx, x):
        x = _require(x, "x")
        out = torch.empty_like(x)
        _call("wkv6_sqrelu_forward", "sqrelu forward", x.device, x.numel(), _ptr(x), _ptr(out))
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        dout = _require(dout, "dout")
        dx = torch.empty_like(x)
        _call("wkv6_sqrelu_backward", "sqrelu backward", x.device, x.numel(), _ptr(x), _ptr(dout), _ptr(dx))
        return dx


class _SigMul(torch.autograd.Function):
    """sigmoid(r) * kv (src/model.py:643-644) in one pass, rounded once."""

    @staticmethod
    def forward(ctx, r, kv):
        r, kv = _require(r, "r"), _require(kv, "kv")
        if r.shape != kv.shape:
            raise RuntimeError("sigmoid_mul: r and kv must have the same shape")
        out = torch.empty_like(r)
        _call("wkv6_sigmul_forward", "sigmul forward", r.device, r.numel(), _ptr(r), _ptr(kv), _ptr(out))
        ctx.save_for_backward(r, kv)
        return out

    @staticmethod
    def backward(ctx, dout):
        r, kv = ctx.saved_tensors
        dout = _require(dout, "dout")
        dr, dkv = torch.empty_like(r), torch.empty_like(kv)
        _call("wkv6_sigmul_backward", "sigmul backward", r.device, r.numel(), *_ptrs(r, kv, dout, dr, dkv))
        return dr, dkv


def sqrelu(x):
    return _SqRelu.apply(x)


def sigmoid_mul(r, kv):
    return _SigMul.apply(r, kv)


def fusable(*tensors):
    """The HIP elementwise path applies: bf16 GPU tensors whose element count is a multiple of 8."""
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.bfloat16 and t.numel() % 8 == 0 for t in tensors)
