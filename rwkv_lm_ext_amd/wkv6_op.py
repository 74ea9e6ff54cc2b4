"""Operator layer: the torch-extension surface of cuda/wkv6_op.cpp, cuda/wkv6_bi_op.cpp,
cuda/wkv6state_op.cpp, cuda/wkv6infctx_op.cpp and cuda/wkv5_op.cpp, served by librwkv6_amd.so.

The reference obtains four module objects from ``torch.utils.cpp_extension.load`` (src/model.py:80-81,
134-135, 188-189; cuda/wkv6_bi.py:7) and calls ``module.forward(...)`` / ``module.backward(...)`` on
them with caller-allocated outputs.  The four objects below keep those names, positional signatures,
in-place output convention and dtypes:

    wkv6_cuda.forward (B,T,C,H, r,k,v, ew[f32], u, y)                              cuda/wkv6_op.cpp:8-10
    wkv6_cuda.backward(B,T,C,H, r,k,v, ew[f32], u, gy, gr,gk,gv,gw, gu[B,C])       cuda/wkv6_op.cpp:11-13
    wkv6_bi_cuda.forward / backward: same with `mask` (int32 [B,T]) after H        cuda/wkv6_bi_op.cpp:8-13
    wkv6state_cuda / wkv6infctx_cuda.forward(B,T,C,H, r,k,v, w[bf16 raw], u, s, y) cuda/wkv6state_op.cpp:8-10
                                   .backward(..., s, gy, gr,gk,gv,gw, gu, gs)      cuda/wkv6state_op.cpp:11-13
    wkv5.forward (B,T,C,H, r,k,v, eew[f32 H,N], u, y)                              cuda/wkv5_op.cpp:8-10
    wkv5.backward(B,T,C,H, r,k,v, eew, ew[f32 H,N], u, gy, gr,gk,gv, gw[B,C], gu[B,C])   cuda/wkv5_op.cpp:11-13

They are also registered as ``torch.ops.wkv6.forward`` etc. (the reference's TORCH_LIBRARY blocks,
cuda/wkv6_op.cpp:19-22).  Unlike the reference shims (which check nothing) every call validates
device, dtype, contiguity and shape and launches on the current stream of the tensors' device.

Every wrapper is made of the pieces of _args.py (whose docstring states what must not change): `_named` builds the table that
`_check_tensors` judges, `_ints` judges an int32 array, `_flags` builds the flag word and `_call` is the one way into the library.
"""
import contextlib
import ctypes

import torch

from . import _lib
from ._args import (_AT_LEAST_2, HEAD_SIZE, _call, _flags, _ints, _io_of, _named, _on_device, _ptr, _ptrs, _s0_entry, _stream_ptr,   # noqa: F401
                    _workspace_or_ckpt)

_SUFFIX = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}      # of the rwkv6_* symbols
_CU_SEQLENS = "cu_seqlens must be a contiguous int32 [n_seq + 1] tensor on the device of r"


def _check_tensors(B, T, C, H, named, dtype=torch.bfloat16):
    dev = None
    for name, (t, shape, dt) in named.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be on the GPU (the WKV6 operator has no CPU path)")
        dev = dev or t.device
        if t.device != dev:
            raise RuntimeError(f"{name} is on {t.device}, expected {dev}")
        if t.dtype != (dt or dtype):
            raise RuntimeError(f"{name} must be {dt or dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise RuntimeError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if C != H * HEAD_SIZE:
        raise RuntimeError(f"C ({C}) must equal H*{HEAD_SIZE} ({H * HEAD_SIZE})")   # reference: assert(H*_N_ == C)
    _lib.load()
    _lib.selftest_once(dev.index, _on_device)
    return dev


class _Wkv6:
    """Stand-in for the module object of `load(name="wkv6", ...)` (src/model.py:188-189)."""

    @staticmethod
    def forward(B, T, C, H, r, k, v, w, u, y):
        dev = _check_tensors(B, T, C, H, _named((B, T, C), None, r, k, v, w, u, wdt=torch.float32, y=y))
        _call("wkv6_cuda_forward", "wkv6 forward", dev, B, T, C, H, *_ptrs(r, k, v, w, u, y))

    @staticmethod
    def backward(B, T, C, H, r, k, v, w, u, gy, gr, gk, gv, gw, gu):
        named = _named((B, T, C), None, r, k, v, w, u, wdt=torch.float32, gy=gy, gr=gr, gk=gk, gv=gv, gw=gw)
        named["gu"] = (gu, (B, C), None)
        dev = _check_tensors(B, T, C, H, named)
        ws = new_checkpoint(B, T, C, H, dev)
        _call("wkv6_backward_ex", "wkv6 backward", dev, B, T, C, H, *_ptrs(r, k, v, w, u, None, gy, gr, gk, gv, gw, gu, None, ws),
              ws.numel(), _lib.W_EW_F32)


class _Wkv6Bi:
    """Stand-in for `load(name="wkv6_bi", ...)` (cuda/wkv6_bi.py:7)."""

    @staticmethod
    def forward(B, T, C, H, mask, r, k, v, w, u, y):
        named = {"mask": (mask, (B, T), torch.int32), **_named((B, T, C), None, r, k, v, w, u, wdt=torch.float32, y=y)}
        dev = _check_tensors(B, T, C, H, named)
        ws = bi_new_workspace(B, T, C, H, dev)
        _call("wkv6bi_forward_ex", "wkv6_bi forward", dev, B, T, C, H, *_ptrs(mask, None, r, k, v, w, u, y, ws), ws.numel(), _lib.W_EW_F32)

    @staticmethod
    def backward(B, T, C, H, mask, r, k, v, w, u, gy, gr, gk, gv, gw, gu):
        named = {"mask": (mask, (B, T), torch.int32),
                 **_named((B, T, C), None, r, k, v, w, u, wdt=torch.float32, gy=gy, gr=gr, gk=gk, gv=gv, gw=gw), "gu": (gu, (B, C), None)}
        dev = _check_tensors(B, T, C, H, named)
        ws = bi_new_workspace(B, T, C, H, dev)
        _call("wkv6bi_backward_ex", "wkv6_bi backward", dev, B, T, C, H, *_ptrs(mask, None, r, k, v, w, u, gy, gr, gk, gv, gw, gu, ws),
              ws.numel(), _lib.W_EW_F32)


class _Wkv6State:
    """Stand-in for `load(name="wkv6state", ...)` (src/model.py:134-135); s: bf16 [H,N,N]."""
    _per_batch = False
    _name = "wkv6state"

    @classmethod
    def _s(cls, s, B, H):
        return {"s": (s, (B, H, HEAD_SIZE, HEAD_SIZE) if cls._per_batch else (H, HEAD_SIZE, HEAD_SIZE), None)}

    @classmethod
    def forward(cls, B, T, C, H, r, k, v, w, u, s, y):
        dev = _check_tensors(B, T, C, H, _named((B, T, C), None, r, k, v, w, u, then=cls._s(s, B, H), y=y))
        _call(cls._name + "_cuda_forward", cls._name + " forward", dev, B, T, C, H, *_ptrs(r, k, v, w, u, s, y))

    @classmethod
    def backward(cls, B, T, C, H, r, k, v, w, u, s, gy, gr, gk, gv, gw, gu, gs):
        named = _named((B, T, C), None, r, k, v, w, u, then=cls._s(s, B, H), gy=gy, gr=gr, gk=gk, gv=gv, gw=gw)
        named["gu"], named["gs"] = (gu, (B, C), None), (gs, (B, H, HEAD_SIZE, HEAD_SIZE), None)
        dev = _check_tensors(B, T, C, H, named)
        ws = new_checkpoint(B, T, C, H, dev)
        _call("wkv6_backward_ex", cls._name + " backward", dev, B, T, C, H, *_ptrs(r, k, v, w, u, s, gy, gr, gk, gv, gw, gu, gs, ws),
              ws.numel(), _lib.W_RAW | (_lib.S0_PER_BATCH if cls._per_batch else 0))


class _Wkv6Infctx(_Wkv6State):
    """Stand-in for `load(name="wkv6infctx", ...)` (src/model.py:80-81); s: bf16 [B,H,N,N], the forward
    overwrites it with the final state (cuda/wkv6infctx_cuda.cu:65-67)."""
    _per_batch = True
    _name = "wkv6infctx"


class _Rwkv6:
    """Stand-in for `load(name="rwkv6", ...)` (src/model_run.py:46-47): stateful forward-only kernel for inference.
    forward_bf16 / forward_fp32 (B,T,C,H, state[f32], r,k,v, eew[f32 decay], u, y); state updated in place."""

    @staticmethod
    def _forward(B, T, C, H, state, r, k, v, w, u, y, io):
        sshape = None if state.numel() == B * H * HEAD_SIZE * HEAD_SIZE else (-1,)
        named = {"state": (state, sshape, torch.float32), **_named((B, T, C), io, r, k, v, w, u, wdt=torch.float32, y=y)}
        dev = _check_tensors(B, T, C, H, named, dtype=io)
        _call("rwkv6_cuda_forward_" + _SUFFIX[io], "rwkv6 forward", dev, B, T, C, H, *_ptrs(state, r, k, v, w, u, y))

    @staticmethod
    def forward_bf16(B, T, C, H, state, r, k, v, w, u, y):
        _Rwkv6._forward(B, T, C, H, state, r, k, v, w, u, y, torch.bfloat16)

    @staticmethod
    def forward_fp32(B, T, C, H, state, r, k, v, w, u, y):
        _Rwkv6._forward(B, T, C, H, state, r, k, v, w, u, y, torch.float32)

    @staticmethod
    def forward_fp16(B, T, C, H, state, r, k, v, w, u, y):
        """cuda/rwkv6_op.cpp:16-19: r, k, v, u, y in fp16; the kernel widens the inputs to fp32 (exact), computes and carries the
        state in fp32 and rounds y to fp16 once (cuda/rwkv6.cu:8-71)."""
        _Rwkv6._forward(B, T, C, H, state, r, k, v, w, u, y, torch.float16)

    # ---- packed batches with a state-slot pool (include/wkv6_amd.h: rwkv6_forward_varlen_*) ----
    @staticmethod
    def _call_varlen(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, algo, ws, io,
                     state_slot_out=None, snap_every=0, cu_snap=None, snap_slot=None, force_snap=False, seg_len=0, force_split=False):
        """Every sequence of the packed [total_T,C] tensors (rows cu_seqlens[s] .. cu_seqlens[s+1]-1) from the state in slot state_slot[s]
        (None: slot s) of state_pool fp32 [n_slots,H,N,N], which is updated in place; y is written, rows outside every sequence as +0.
        w is the fp32 decay.  algo="scan" forces the exact scan kernel; ws: a new_rwkv6_varlen_workspace() buffer (graph capture).
        state_slot_out (int32 [n_seq]): the slot that takes the final state of sequence s instead of its source slot.  snap_every (a
        multiple of 64) with cu_snap (int32 [n_seq + 1]) and snap_slot (int32 [n_snap]): the state after the first (j + 1) * snap_every
        tokens of sequence s goes to slot snap_slot[cu_snap[s] + j] as well (include/wkv6_amd.h: rwkv6_forward_varlen_snap_*).  With all
        four at their defaults the plain entry point is called (force_snap: the snap entry point all the same).
        seg_len (0, or a multiple of 64; bf16 on the chunked route only): every sequence longer than seg_len tokens is cut at multiples of
        seg_len and served by one workgroup per (segment, head) (include/wkv6_amd.h: rwkv6_forward_varlen_split_bf16); ws is then a
        new_rwkv6_varlen_split_workspace() buffer.  seg_len > 0 or force_split: the split entry point."""
        named = {"state_pool": (state_pool, None, torch.float32),
                 **_named((total_T, C), io, r, k, v, w, u, wdt=torch.float32, ushape=(H, HEAD_SIZE), y=y)}
        for name, (t, _, dt) in named.items():      # (types first: what is wrong with a tensor is reported whatever device it is on)
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name} must be a tensor")
            if t.dtype != dt:
                raise RuntimeError(f"{name} must be {dt}, got {t.dtype}")
        if algo not in (None, "scan"):
            raise RuntimeError(f"unknown algo {algo!r}")
        if int(total_T) < 1 or int(max_seqlen) < 1:
            raise RuntimeError("total_T and max_seqlen must be >= 1")
        per_slot = H * HEAD_SIZE * HEAD_SIZE
        if state_pool.dim() != 4 or tuple(state_pool.shape[1:]) != (H, HEAD_SIZE, HEAD_SIZE) or state_pool.shape[0] < 1:
            raise RuntimeError(f"state_pool has shape {tuple(state_pool.shape)}, expected (n_slots, {H}, {HEAD_SIZE}, {HEAD_SIZE})")
        n_slots = state_pool.numel() // per_slot
        n_seq = _ints(cu_seqlens, _AT_LEAST_2, r.device, _CU_SEQLENS).numel() - 1
        if state_slot is None:
            if n_slots < n_seq:
                raise RuntimeError(f"state_slot=None names slot s for sequence s: the pool has {n_slots} slots for {n_seq} sequences")
        else:
            _ints(state_slot, (n_seq,), r.device, "state_slot must be a contiguous int32 [n_seq] tensor on the device of r, or None")
        if ws is not None and not (isinstance(ws, torch.Tensor) and ws.dtype == torch.uint8 and ws.is_contiguous()
                                   and ws.device == r.device):
            raise RuntimeError("ws must be a new_rwkv6_varlen_workspace() buffer on the device of r")
        if not isinstance(seg_len, int) or isinstance(seg_len, bool) or seg_len < 0 or seg_len % 64 != 0:
            raise RuntimeError(f"seg_len must be 0 or a multiple of 64, got {seg_len!r}")
        if seg_len > 0 and algo == "scan":
            raise RuntimeError("seg_len > 0 cuts sequences on the chunked route only: not with algo='scan'")
        if seg_len > 0 and io != torch.bfloat16:
            raise RuntimeError(f"seg_len > 0 is a bf16 call, got {io}")
        split = force_split or seg_len > 0
        force_snap = force_snap or split
        snap = force_snap or not (state_slot_out is None and isinstance(snap_every, int) and snap_every == 0 and cu_snap is None and snap_slot is None)
        if snap:
            if not isinstance(snap_every, int) or snap_every < 0 or snap_every % 64 != 0:
                raise RuntimeError(f"snap_every must be 0 or a multiple of 64, got {snap_every!r}")
            if state_slot_out is not None:
                _ints(state_slot_out, (n_seq,), r.device, "state_slot_out must be a contiguous int32 [n_seq] tensor on the device of r")
            if snap_every == 0:
                if cu_snap is not None or snap_slot is not None:
                    raise RuntimeError("cu_snap and snap_slot belong to snap_every > 0")
            else:
                _ints(cu_snap, (n_seq + 1,), r.device, "cu_snap must be a contiguous int32 [n_seq + 1] tensor on the device of r")
                _ints(snap_slot, None, r.device, "snap_slot must be a contiguous int32 [n_snap] tensor on the device of r")
        dev = _check_tensors(n_seq, total_T, C, H, named, dtype=io)
        base = (int(total_T), n_seq, int(max_seqlen), C, H, _ptr(cu_seqlens), _ptr(state_slot), n_slots, *_ptrs(state_pool, r, k, v, w, u, y, ws),
                0 if ws is None else ws.numel(), _lib.ALGO_SCAN if algo == "scan" else 0)
        if not snap:
            _call("rwkv6_forward_varlen_" + _SUFFIX[io], "rwkv6 forward_varlen", dev, *base)
            return
        tail = (_ptr(state_slot_out), snap_every, _ptr(cu_snap), _ptr(snap_slot), 0 if snap_slot is None else snap_slot.numel())   # behind the stream
        if split:
            _call("rwkv6_forward_varlen_split_bf16", "rwkv6 forward_varlen", dev, *base, tail=tail + (seg_len,))
        else:
            _call("rwkv6_forward_varlen_snap_" + _SUFFIX[io], "rwkv6 forward_varlen", dev, *base, tail=tail)


# rwkv6.forward_varlen_{bf16,fp16,fp32}, forward_varlen_snap_{bf16,fp16,fp32} and forward_varlen_split_bf16: one definition per kind, made once
# per I/O type.  Only bf16 can cut sequences, so only its plain form has a seg_len (the others refuse the keyword as any unknown one).
def _varlen_plain(io):
    if io == torch.bfloat16:
        def fn(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, algo=None, ws=None, state_slot_out=None,
               snap_every=0, cu_snap=None, snap_slot=None, seg_len=0):
            _Rwkv6._call_varlen(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, algo, ws, io, state_slot_out,
                                snap_every, cu_snap, snap_slot, seg_len=seg_len)
    else:
        def fn(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, algo=None, ws=None, state_slot_out=None,
               snap_every=0, cu_snap=None, snap_slot=None):
            _Rwkv6._call_varlen(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, algo, ws, io, state_slot_out,
                                snap_every, cu_snap, snap_slot)
    return fn


def _varlen_snap(io):
    def fn(total_T, C, H, state_pool, state_slot, state_slot_out, r, k, v, w, u, y, cu_seqlens, max_seqlen, snap_every, cu_snap, snap_slot):
        _Rwkv6._call_varlen(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, None, None, io, state_slot_out,
                            snap_every, cu_snap, snap_slot, force_snap=True)
    fn.__doc__ = f"torch.ops.rwkv6.forward_varlen_snap_{_SUFFIX[io]}: always the snap entry point of the library, defaults included."
    return fn


def _varlen_split(io):
    def fn(total_T, C, H, state_pool, state_slot, state_slot_out, r, k, v, w, u, y, cu_seqlens, max_seqlen, snap_every, cu_snap, snap_slot,
           seg_len, ws=None):
        """torch.ops.rwkv6.forward_varlen_split_bf16: always the split entry point of the library, seg_len = 0 included."""
        _Rwkv6._call_varlen(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, None, ws, io, state_slot_out,
                            snap_every, cu_snap, snap_slot, seg_len=seg_len, force_split=True)
    return fn


for _kind, _make, _ios in (("", _varlen_plain, _SUFFIX), ("snap_", _varlen_snap, _SUFFIX), ("split_", _varlen_split, (torch.bfloat16,))):
    for _io in _ios:
        _fn = _make(_io)
        _fn.__name__ = f"forward_varlen_{_kind}{_SUFFIX[_io]}"
        _fn.__qualname__ = "_Rwkv6." + _fn.__name__          # as a method written out in the class would read in a TypeError
        setattr(_Rwkv6, _fn.__name__, staticmethod(_fn))


class _Wkv5:
    """Stand-in for the module object of `load(name="wkv5", ...)` (src/model.py:238-239): the RWKV-5 operator, whose decay is an
    [H,N] parameter.  forward (B,T,C,H, r,k,v, eew[f32 decay], u, y); backward(B,T,C,H, r,k,v, eew, ew[f32], u, gy, gr,gk,gv,
    gw[B,C], gu[B,C])  (cuda/wkv5_op.cpp:8-13)."""

    @staticmethod
    def forward(B, T, C, H, r, k, v, w, u, y):
        hn = (H, HEAD_SIZE)
        dev = _check_tensors(B, T, C, H, _named((B, T, C), None, r, k, v, w, u, wdt=torch.float32, wshape=hn, ushape=hn, y=y))
        _call("wkv5_cuda_forward", "wkv5 forward", dev, B, T, C, H, *_ptrs(r, k, v, w, u, y))

    @staticmethod
    def backward(B, T, C, H, r, k, v, w, ww, u, gy, gr, gk, gv, gw, gu):
        btc, hn = (B, T, C), (H, HEAD_SIZE)
        dev = _check_tensors(B, T, C, H, dict(        # (ww stands between w and u: not the head of _named)
            r=(r, btc, None), k=(k, btc, None), v=(v, btc, None), w=(w, hn, torch.float32), ww=(ww, hn, torch.float32),
            u=(u, hn, None), gy=(gy, btc, None), gr=(gr, btc, None), gk=(gk, btc, None), gv=(gv, btc, None),
            gw=(gw, (B, C), None), gu=(gu, (B, C), None)))
        _call("wkv5_cuda_backward", "wkv5 backward", dev, B, T, C, H, *_ptrs(r, k, v, w, ww, u, gy, gr, gk, gv, gw, gu))


rwkv6 = _Rwkv6
wkv5 = _Wkv5
wkv6_cuda = _Wkv6
wkv6_bi_cuda = _Wkv6Bi
wkv6state_cuda = _Wkv6State
wkv6infctx_cuda = _Wkv6Infctx


# ---- generic entry used by the autograd layer (raw bf16 decay, optional fp32 I/O, explicit state) ----
def new_checkpoint(B, T, C, H, device):
    """Buffer for the forward-state checkpoints that `forward_ex(..., ckpt=)` fills and `backward_ex(..., ckpt=)`
    consumes (also usable as the backward workspace)."""
    return torch.empty(_lib.load().wkv6_backward_workspace_bytes(B, T, C, H), dtype=torch.uint8, device=device)


def forward_ex(r, k, v, w, u, H, s0=None, s_out=None, w_is_ew=False, y=None, algo=None, ckpt=None):
    """y = WKV6(r,k,v,w,u[,s0]) with the I/O type of `r` (bf16, or fp32 for numerics tests).
    algo: None (library default: chunked MFMA kernel for bf16 I/O) or "scan" (exact token-serial kernels)."""
    B, T, C = btc = r.shape
    io = _io_of(r)
    named = _named(btc, io, r, k, v, w, u, wdt=torch.float32 if w_is_ew else io, ushape=(H, HEAD_SIZE))
    flags = _flags(io, w_is_ew, algo)
    if s0 is not None:
        named["s0"], per_batch = _s0_entry(s0, B, H, io)
        flags |= per_batch
    if s_out is not None:
        named["s_out"] = (s_out, (B, H, HEAD_SIZE, HEAD_SIZE), io)
    if y is None:
        y = torch.empty(btc, device=r.device, dtype=io)
    named["y"] = (y, btc, io)
    dev = _check_tensors(B, T, C, H, named, dtype=io)
    if ckpt is not None:       # training forward: also store the per-group state checkpoints for the backward
        _call("wkv6_forward_ckpt_ex", "wkv6 forward_ex", dev, B, T, C, H, *_ptrs(r, k, v, w, u, s0, s_out, y, ckpt), ckpt.numel(), flags)
    else:
        _call("wkv6_forward_ex", "wkv6 forward_ex", dev, B, T, C, H, *_ptrs(r, k, v, w, u, s0, s_out, y), flags)
    return y


def forward_gn_ex(r, k, v, w, u, H, gate, gamma, beta, eps, ckpt=None, want_y=True, want_stats=True):
    """The operator with the time-mix block's GroupNorm(H) * gate epilogue fused into its store (src/model.py:462-468, SURVEY.md
    row n1).  Returns (out, y or None, stats or None), or None where the library cannot fuse (so few (batch, head) pairs that
    two workgroups share one): the caller then runs the two kernels."""
    B, T, C = btc = r.shape
    bf = torch.bfloat16
    named = _named(btc, bf, r, k, v, w, u, ushape=(H, HEAD_SIZE), gate=gate)
    named["gamma"], named["beta"] = (gamma, (C,), bf), (beta, (C,), bf)
    dev = _check_tensors(B, T, C, H, named, dtype=bf)
    out = torch.empty(btc, device=dev, dtype=bf)
    y = torch.empty(btc, device=dev, dtype=bf) if want_y else None
    stats = torch.empty((B * T, H, 2), device=dev, dtype=torch.float32) if want_stats else None
    rc = _call("wkv6_forward_gn_ex", "wkv6 forward_gn_ex", dev, B, T, C, H, *_ptrs(r, k, v, w, u, None, None, y, ckpt),
               0 if ckpt is None else ckpt.numel(), *_ptrs(gate, gamma, beta), float(eps), _ptr(out), _ptr(stats), _lib.W_RAW, check=False)
    if rc == _lib.EUNSUPPORTED:
        return None
    _lib.check(rc, "wkv6 forward_gn_ex")
    return out, y, stats


def backward_ex(r, k, v, w, u, gy, H, s0=None, w_is_ew=False, want_gs=False, algo=None, ckpt=None):
    """Returns (gr, gk, gv, gw, gu[B,C], gs[B,H,N,N] or None): gradients in the I/O type of `r`, the per-batch partials gu / gs
    in fp32 (WKV6_PARTIALS_F32)."""
    B, T, C = btc = r.shape
    io = r.dtype
    named = _named(btc, io, r, k, v, w, u, wdt=torch.float32 if w_is_ew else io, ushape=(H, HEAD_SIZE), gy=gy)
    # gu / gs are per-batch partial sums the caller reduces: always fp32, so that the parameter gradient is rounded once
    flags = _flags(io, w_is_ew, algo) | _lib.PARTIALS_F32
    if s0 is not None:
        named["s0"], per_batch = _s0_entry(s0, B, H, io)
        flags |= per_batch
    dev = _check_tensors(B, T, C, H, named, dtype=io)
    gr, gk, gv, gw = (torch.empty(btc, device=dev, dtype=io) for _ in range(4))
    gu = torch.empty((B, C), device=dev, dtype=torch.float32)
    gs = torch.empty((B, H, HEAD_SIZE, HEAD_SIZE), device=dev, dtype=torch.float32) if want_gs else None
    # ckpt: the checkpoints written by forward_ex(..., ckpt=ckpt) on the same inputs.  Here, unlike in every other backward, a ckpt alone
    # marks them valid, whatever the I/O type and the algorithm
    ws, valid = _workspace_or_ckpt(ckpt, True, io, algo, new_checkpoint, B, T, C, H, dev, chunked_only=False)
    _call("wkv6_backward_ex", "wkv6 backward_ex", dev, B, T, C, H, *_ptrs(r, k, v, w, u, s0, gy, gr, gk, gv, gw, gu, gs, ws), ws.numel(),
          flags | valid)
    return gr, gk, gv, gw, gu, gs


# ---- packed variable-length batches (include/wkv6_amd.h: wkv6_*_varlen_ex) ----
def new_varlen_workspace(total_T, n_seq, C, H, device):
    """Workspace of the packed pair: the per-sequence int arrays and the state checkpoints that `forward_varlen_ex(..., ws=)` fills and
    `backward_varlen_ex(..., ws=, ckpt_valid=True)` consumes.  Sized from the host-side bound, no device data needed."""
    n = _lib.load().wkv6_varlen_workspace_bytes(total_T, n_seq, C, H)
    if n == 0:
        raise RuntimeError(f"bad packed shape: total_T {total_T}, n_seq {n_seq}, C {C}, H {H}")
    return torch.empty(n, dtype=torch.uint8, device=device)


def new_rwkv6_varlen_workspace(n_seq, device):
    """Workspace of rwkv6.forward_varlen_*: the four prepared int32 [n_seq] arrays (a caller that replays graphs owns it)."""
    n = _lib.load().rwkv6_varlen_workspace_bytes(n_seq)
    if n == 0:
        raise RuntimeError(f"bad n_seq {n_seq}")
    return torch.empty(n, dtype=torch.uint8, device=device)


def new_rwkv6_varlen_split_workspace(total_T, n_seq, seg_len, C, H, device):
    """Workspace of rwkv6.forward_varlen_bf16(..., seg_len=) / forward_varlen_split_bf16: the prepared int arrays, the item table and the
    per-item states of the cut (a caller that replays graphs owns it).  Sized from the host-side bound, no device data needed."""
    n = _lib.load().rwkv6_varlen_split_workspace_bytes(total_T, n_seq, seg_len, C, H)
    if n == 0:
        raise RuntimeError(f"bad packed shape: total_T {total_T}, n_seq {n_seq}, seg_len {seg_len}, C {C}, H {H}")
    return torch.empty(n, dtype=torch.uint8, device=device)


def _packed_dims(r, cu_seqlens, io_too=False):
    """(total_T, C, n_seq) of a packed call, judged in this order: r is 2-d, [its I/O type,] cu_seqlens."""
    if r.dim() != 2:
        raise RuntimeError("packed tensors are [total_T, C]")
    if io_too:
        _io_of(r)
    return r.shape[0], r.shape[1], _ints(cu_seqlens, _AT_LEAST_2, r.device, _CU_SEQLENS).numel() - 1


def _check_max_seqlen(max_seqlen):
    if int(max_seqlen) < 1:
        raise RuntimeError("max_seqlen must be >= 1")


def _varlen_common(r, k, v, w, u, H, cu_seqlens, max_seqlen, s0, w_is_ew, algo, **same):
    """(total_T, C, io, n_seq, named, flags) of the packed wrappers; same: further [total_T, C] tensors of the I/O type."""
    total, C, n_seq = _packed_dims(r, cu_seqlens, io_too=True)
    io = r.dtype
    named = _named((total, C), io, r, k, v, w, u, wdt=torch.float32 if w_is_ew else io, ushape=(H, HEAD_SIZE), **same)
    flags = _flags(io, w_is_ew, algo)
    if s0 is not None:
        named["s0"], per_seq = _s0_entry(s0, n_seq, H, io)
        flags |= per_seq
    _check_max_seqlen(max_seqlen)
    return total, C, io, n_seq, named, flags


def _varlen_backward_workspace(ws, ckpt_valid, io, algo, total, n_seq, C, H, dev):
    if ckpt_valid and ws is None:
        raise RuntimeError("ckpt_valid needs the workspace the forward filled")
    return _workspace_or_ckpt(ws, ckpt_valid, io, algo, new_varlen_workspace, total, n_seq, C, H, dev)


def forward_varlen_ex(r, k, v, w, u, H, cu_seqlens, max_seqlen, s0=None, s_out=None, w_is_ew=False, y=None, algo=None, ws=None):
    """y [total_T,C] = WKV6 of every sequence of a packed batch on its own (sequence s = rows cu_seqlens[s] .. cu_seqlens[s+1]-1, each
    from s0).  ws: a new_varlen_workspace() buffer that keeps the state checkpoints for backward_varlen_ex(..., ws=ws, ckpt_valid=True)."""
    total, C, io, n_seq, named, flags = _varlen_common(r, k, v, w, u, H, cu_seqlens, max_seqlen, s0, w_is_ew, algo)
    if s_out is not None:
        named["s_out"] = (s_out, (n_seq, H, HEAD_SIZE, HEAD_SIZE), io)
    if y is None:
        y = torch.empty((total, C), device=r.device, dtype=io)
    named["y"] = (y, (total, C), io)
    dev = _check_tensors(n_seq, total, C, H, named, dtype=io)
    _call("wkv6_forward_varlen_ex", "wkv6 forward_varlen_ex", dev, total, n_seq, int(max_seqlen), C, H,
          *_ptrs(cu_seqlens, r, k, v, w, u, s0, s_out, y, ws), 0 if ws is None else ws.numel(), flags)
    return y


def backward_varlen_ex(r, k, v, w, u, gy, H, cu_seqlens, max_seqlen, s0=None, w_is_ew=False, want_gs=False, algo=None, ws=None,
                       ckpt_valid=False):
    """Returns (gr, gk, gv, gw [total_T,C], gu [n_seq,C], gs [n_seq,H,N,N] or None); gu / gs are fp32 per-sequence partials
    (WKV6_PARTIALS_F32) for the caller to sum.  ckpt_valid: `ws` was filled by forward_varlen_ex(..., ws=ws) on the same inputs."""
    total, C, io, n_seq, named, flags = _varlen_common(r, k, v, w, u, H, cu_seqlens, max_seqlen, s0, w_is_ew, algo, gy=gy)
    dev = _check_tensors(n_seq, total, C, H, named, dtype=io)
    gr, gk, gv, gw = (torch.empty((total, C), device=dev, dtype=io) for _ in range(4))
    gu = torch.empty((n_seq, C), device=dev, dtype=torch.float32)
    gs = torch.empty((n_seq, H, HEAD_SIZE, HEAD_SIZE), device=dev, dtype=torch.float32) if want_gs else None
    ws, valid = _varlen_backward_workspace(ws, ckpt_valid, io, algo, total, n_seq, C, H, dev)
    _call("wkv6_backward_varlen_ex", "wkv6 backward_varlen_ex", dev, total, n_seq, int(max_seqlen), C, H,
          *_ptrs(cu_seqlens, r, k, v, w, u, s0, gy, gr, gk, gv, gw, gu, gs, ws), ws.numel(), flags | _lib.PARTIALS_F32 | valid)
    return gr, gk, gv, gw, gu, gs


def wkv5_forward_ex(r, k, v, w, u, H, y=None):
    """y = WKV5(r,k,v,w,u): w, u [H,N] raw parameters in the I/O type of `r` (bf16, or fp32 for numerics tests)."""
    B, T, C = btc = r.shape
    io = _io_of(r)
    hn = (H, HEAD_SIZE)
    if y is None:
        y = torch.empty(btc, device=r.device, dtype=io)
    dev = _check_tensors(B, T, C, H, _named(btc, io, r, k, v, w, u, wshape=hn, ushape=hn, y=y), dtype=io)
    _call("wkv5_forward_ex", "wkv5 forward_ex", dev, B, T, C, H, *_ptrs(r, k, v, w, u, y), _flags(io))
    return y


def wkv5_backward_ex(r, k, v, w, u, gy, H):
    """Returns (gr, gk, gv, gw[B,C], gu[B,C]): gradients in the I/O type of `r`, the per-batch partials gw (with respect to the raw
    w) and gu in fp32 (WKV6_PARTIALS_F32), for the caller to sum over the batch and round once."""
    B, T, C = btc = r.shape
    io = r.dtype
    hn = (H, HEAD_SIZE)
    dev = _check_tensors(B, T, C, H, _named(btc, io, r, k, v, w, u, wshape=hn, ushape=hn, gy=gy), dtype=io)
    gr, gk, gv = (torch.empty(btc, device=dev, dtype=io) for _ in range(3))
    gw, gu = (torch.empty((B, C), device=dev, dtype=torch.float32) for _ in range(2))
    _call("wkv5_backward_ex", "wkv5 backward_ex", dev, B, T, C, H, *_ptrs(r, k, v, w, None, u, gy, gr, gk, gv, gw, gu),
          _flags(io) | _lib.PARTIALS_F32)
    return gr, gk, gv, gw, gu


REV_R, REV_K, REV_V, REV_W, REV_Y, REV_ALL = _lib.REV_R, _lib.REV_K, _lib.REV_V, _lib.REV_W, _lib.REV_Y, _lib.REV_ALL


def _check_rev(n, what, rev_n, rev_mask, dev, or_none=False):
    """rev_n: int32 [n] (`what` names n in the message) on dev; or_none: the packed wrappers take None for "no map"."""
    if rev_n is not None or not or_none:
        _ints(rev_n, (n,), dev, f"rev_n must be a contiguous int32 [{what}] tensor on the device of r")
    if rev_mask & ~REV_ALL:
        raise RuntimeError(f"rev_mask {rev_mask} has unknown bits")


def forward_rev_ex(r, k, v, w, u, H, rev_n, rev_mask, y=None, ckpt=None, algo=None):
    """WKV6 over partially reversed sequences without materialising the reversal (include/wkv6_amd.h, wkv6_forward_rev_ex):
    tokens [0, rev_n[b]) of the tensors named in `rev_mask` (REV_R | REV_K | REV_V | REV_W | REV_Y) are taken in reverse
    order, the rest in place.  I/O type of `r`: bf16 (chunked MFMA kernels; algo="scan" forces the exact ones) or fp32 (exact
    scan kernels)."""
    B, T, C = btc = r.shape
    io = _io_of(r)
    if y is None:
        y = torch.empty(btc, device=r.device, dtype=io)
    dev = _check_tensors(B, T, C, H, _named(btc, io, r, k, v, w, u, ushape=(H, HEAD_SIZE), y=y), dtype=io)
    _check_rev(B, "B", rev_n, rev_mask, dev)
    _call("wkv6_forward_rev_ex", "wkv6 forward_rev_ex", dev, B, T, C, H, *_ptrs(r, k, v, w, u, y, ckpt), 0 if ckpt is None else ckpt.numel(),
          _ptr(rev_n), rev_mask, _flags(io, algo=algo))
    return y


def _pair_sets(n, shape, C, H, sets, u, bwd, packed):
    """Check and pack the two problems of a pair launch.  sets: two dicts with r, k, v, w (+ y | gy) [shape], ckpt, rev_n [n], rev_mask.
    Dense (n = B): ckpt is a new_checkpoint() buffer, and a problem without rev_n is not judged by its rev_mask.  packed (n = n_seq): ckpt is
    one new_varlen_workspace() buffer per problem, and the rev_mask is judged with or without rev_n."""
    bf = torch.bfloat16
    arr = (_lib.SeqSet * 2)()
    keep = []                                   # tensors the packed pointers refer to
    dev = None
    for i, q in enumerate(sets):
        named = {name: (q[name], shape, bf) for name in ("r", "k", "v", "w") + (("gy",) if bwd else ("y",))}
        named["u"] = (u, (H, HEAD_SIZE), bf)
        dev = _check_tensors(n, shape[-2], C, H, named, dtype=bf)
        rev_n, rev_mask = q.get("rev_n"), q.get("rev_mask", 0)
        if packed or rev_n is not None:
            _check_rev(n, "n_seq" if packed else "B", rev_n, rev_mask, dev, or_none=packed)
        ckpt = q.get("ckpt")
        if bwd and ckpt is None:
            raise RuntimeError("wkv6 packed pair backward: both problems need the workspaces their forward wrote" if packed else
                               "wkv6 pair backward: both problems need the checkpoints their forward wrote")
        e = arr[i]
        e.r, e.k, e.v, e.w = _ptrs(q["r"], q["k"], q["v"], q["w"])
        if bwd:
            outs = [torch.empty(shape, device=dev, dtype=bf) for _ in range(4)] + [torch.empty((n, C), device=dev, dtype=torch.float32)]
            e.gy, e.gr, e.gk, e.gv, e.gw, e.gu = _ptrs(q["gy"], *outs)
            keep.append(outs)
        else:
            e.y = _ptr(q["y"])
        e.ckpt, e.ckpt_bytes = _ptr(ckpt), 0 if ckpt is None else ckpt.numel()
        e.rev_n, e.rev_mask = _ptr(rev_n), rev_mask if rev_n is not None else 0
    return arr, keep, dev


def _pair_outputs(sets, shape):
    for q in sets:
        if q.get("y") is None:
            q["y"] = torch.empty(shape, device=q["r"].device, dtype=torch.bfloat16)


def forward_pair_ex(H, u, sets):
    """Both operator calls of a bidirectional time-mix layer in one launch (include/wkv6_amd.h, wkv6_forward_pair_ex; SURVEY.md
    row n2): `sets` = two dicts {r, k, v, w, [y], [ckpt], [rev_n, rev_mask]} of one shape.  Returns (y0, y1)."""
    B, T, C = btc = tuple(sets[0]["r"].shape)
    _pair_outputs(sets, btc)
    arr, _, dev = _pair_sets(B, btc, C, H, sets, u, bwd=False, packed=False)
    _call("wkv6_forward_pair_ex", "wkv6 forward_pair_ex", dev, B, T, C, H, _ptr(u), arr, _lib.W_RAW)
    return sets[0]["y"], sets[1]["y"]


def backward_pair_ex(H, u, sets):
    """Gradients of forward_pair_ex: two tuples (gr, gk, gv, gw, gu[B,C] fp32), one per problem; `sets` as in the forward plus gy."""
    B, T, C = btc = tuple(sets[0]["r"].shape)
    arr, keep, dev = _pair_sets(B, btc, C, H, sets, u, bwd=True, packed=False)
    _call("wkv6_backward_pair_ex", "wkv6 backward_pair_ex", dev, B, T, C, H, _ptr(u), arr, _lib.W_RAW | _lib.PARTIALS_F32)
    return tuple(keep[0]), tuple(keep[1])


def backward_rev_ex(r, k, v, w, u, gy, H, rev_n, rev_mask, ckpt=None, algo=None):
    """Gradients of forward_rev_ex: (gr, gk, gv, gw, gu[B,C]); each gradient is laid out like its tensor."""
    B, T, C = btc = r.shape
    io = _io_of(r)
    dev = _check_tensors(B, T, C, H, _named(btc, io, r, k, v, w, u, ushape=(H, HEAD_SIZE), gy=gy), dtype=io)
    _check_rev(B, "B", rev_n, rev_mask, dev)
    gr, gk, gv, gw = (torch.empty(btc, device=dev, dtype=io) for _ in range(4))
    gu = torch.empty((B, C), device=dev, dtype=torch.float32)
    exact = io == torch.float32 or algo == "scan"           # the exact kernels read no checkpoints: a ckpt is left alone, not used as workspace
    ws, valid = _workspace_or_ckpt(None if exact else ckpt, True, io, algo, new_checkpoint, B, T, C, H, dev)
    _call("wkv6_backward_rev_ex", "wkv6 backward_rev_ex", dev, B, T, C, H, *_ptrs(r, k, v, w, u, gy, gr, gk, gv, gw, gu, ws), ws.numel(),
          _ptr(rev_n), rev_mask, _flags(io, algo=algo) | _lib.PARTIALS_F32 | valid)
    return gr, gk, gv, gw, gu


# ---- reversal maps and the pair launch on packed batches (include/wkv6_amd.h: wkv6_*_varlen_rev_ex, wkv6_*_varlen_pair_ex) ----
def forward_varlen_rev_ex(r, k, v, w, u, H, cu_seqlens, max_seqlen, rev_n, rev_mask, y=None, algo=None, ws=None, w_is_ew=False):
    """forward_varlen_ex with the per-tensor reversal map of forward_rev_ex applied within every sequence: rev_n int32 [n_seq] (clamped to
    the sequence's length on the device; None: no map).  No initial state.  ws: a new_varlen_workspace() buffer that keeps the checkpoints
    for backward_varlen_rev_ex(..., ws=ws, ckpt_valid=True)."""
    total, C, io, n_seq, named, flags = _varlen_common(r, k, v, w, u, H, cu_seqlens, max_seqlen, None, w_is_ew, algo)
    if y is None:
        y = torch.empty((total, C), device=r.device, dtype=io)
    named["y"] = (y, (total, C), io)
    dev = _check_tensors(n_seq, total, C, H, named, dtype=io)
    _check_rev(n_seq, "n_seq", rev_n, rev_mask, dev, or_none=True)
    _call("wkv6_forward_varlen_rev_ex", "wkv6 forward_varlen_rev_ex", dev, total, n_seq, int(max_seqlen), C, H,
          *_ptrs(cu_seqlens, r, k, v, w, u, y, ws), 0 if ws is None else ws.numel(), _ptr(rev_n), rev_mask, flags)
    return y


def backward_varlen_rev_ex(r, k, v, w, u, gy, H, cu_seqlens, max_seqlen, rev_n, rev_mask, algo=None, ws=None, ckpt_valid=False,
                           w_is_ew=False):
    """Gradients of forward_varlen_rev_ex: (gr, gk, gv, gw [total_T,C], gu [n_seq,C] fp32 per-sequence partials); each gradient is laid
    out like its tensor.  ckpt_valid: `ws` was filled by forward_varlen_rev_ex(..., ws=ws) on the same inputs."""
    total, C, io, n_seq, named, flags = _varlen_common(r, k, v, w, u, H, cu_seqlens, max_seqlen, None, w_is_ew, algo, gy=gy)
    dev = _check_tensors(n_seq, total, C, H, named, dtype=io)
    _check_rev(n_seq, "n_seq", rev_n, rev_mask, dev, or_none=True)
    gr, gk, gv, gw = (torch.empty((total, C), device=dev, dtype=io) for _ in range(4))
    gu = torch.empty((n_seq, C), device=dev, dtype=torch.float32)
    ws, valid = _varlen_backward_workspace(ws, ckpt_valid, io, algo, total, n_seq, C, H, dev)
    _call("wkv6_backward_varlen_rev_ex", "wkv6 backward_varlen_rev_ex", dev, total, n_seq, int(max_seqlen), C, H,
          *_ptrs(cu_seqlens, r, k, v, w, u, gy, gr, gk, gv, gw, gu, ws), ws.numel(), _ptr(rev_n), rev_mask, flags | _lib.PARTIALS_F32 | valid)
    return gr, gk, gv, gw, gu


def forward_varlen_pair_ex(H, u, sets, cu_seqlens, max_seqlen):
    """forward_pair_ex on a packed batch: `sets` = two dicts {r, k, v, w [total_T,C], [y], [ckpt], [rev_n [n_seq], rev_mask]} over the
    same sequences; ckpt is one new_varlen_workspace() buffer per problem.  Returns (y0, y1)."""
    total, C, n_seq = _packed_dims(sets[0]["r"], cu_seqlens)
    _check_max_seqlen(max_seqlen)
    _pair_outputs(sets, (total, C))
    arr, _, dev = _pair_sets(n_seq, (total, C), C, H, sets, u, bwd=False, packed=True)
    _call("wkv6_forward_varlen_pair_ex", "wkv6 forward_varlen_pair_ex", dev, total, n_seq, int(max_seqlen), C, H, _ptr(cu_seqlens), _ptr(u), arr,
          _lib.W_RAW)
    return sets[0]["y"], sets[1]["y"]


def backward_varlen_pair_ex(H, u, sets, cu_seqlens, max_seqlen):
    """Gradients of forward_varlen_pair_ex: two tuples (gr, gk, gv, gw, gu [n_seq,C] fp32), one per problem; `sets` as in the forward
    (with the workspaces it filled) plus gy."""
    total, C, n_seq = _packed_dims(sets[0]["r"], cu_seqlens)
    _check_max_seqlen(max_seqlen)
    arr, keep, dev = _pair_sets(n_seq, (total, C), C, H, sets, u, bwd=True, packed=True)
    _call("wkv6_backward_varlen_pair_ex", "wkv6 backward_varlen_pair_ex", dev, total, n_seq, int(max_seqlen), C, H, _ptr(cu_seqlens), _ptr(u),
          arr, _lib.W_RAW | _lib.PARTIALS_F32)
    return tuple(keep[0]), tuple(keep[1])


def bi_new_workspace(B, T, C, H, device):
    """Workspace of the wkv6_bi pair: the forward's fp32 y side buffer, the state checkpoints of both scans (kept from
    forward to backward when `ws` is passed to both calls) and the backward's four fp32 gradient side buffers."""
    return torch.empty(_lib.load().wkv6bi_workspace_bytes(B, T, C, H), dtype=torch.uint8, device=device)


def bi_new_kept(B, T, C, H, device):
    """The part of the wkv6_bi workspace that has to live from the forward to the backward (row lengths, order, the state
    checkpoints of both scans: 2 x 4 B per token-channel at 64-token checkpoint spacing); passed as `ws`, the fp32 side buffers
    (4 B per token-channel in the forward, 16 B in the backward) become per-call scratch of the library."""
    return torch.empty(_lib.load().wkv6bi_kept_bytes(B, T, C, H), dtype=torch.uint8, device=device)


def _mask_or_lens(mask, lens, B, T):
    """wkv6bi_*_ex take the reference's int32 mask [B,T] (row length = 1 + index of its first zero) or, instead, the row lengths
    themselves as int32 [B] (0 .. T): exactly one of the two."""
    if (mask is None) == (lens is None):
        raise RuntimeError("pass either mask or lens")
    return {"mask": (mask, (B, T), torch.int32)} if lens is None else {"lens": (lens, (B,), torch.int32)}


def bi_forward_ex(mask, r, k, v, w, u, H, w_is_ew=False, algo=None, ws=None, lens=None):
    """ws: a bi_new_workspace() buffer the caller keeps for bi_backward_ex(..., ws=ws): the forward then stores the state
    checkpoints of both scans in it and the backward skips its two state passes.  lens: row lengths instead of the mask."""
    B, T, C = btc = r.shape
    io = r.dtype
    named = {**_mask_or_lens(mask, lens, B, T),
             **_named(btc, io, r, k, v, w, u, wdt=torch.float32 if w_is_ew else io, ushape=(H, HEAD_SIZE))}
    dev = _check_tensors(B, T, C, H, named, dtype=io)
    y = torch.empty(btc, device=dev, dtype=io)
    flags = _flags(io, w_is_ew, algo)
    if ws is not None:
        flags |= _lib.BI_KEEP_CKPT
    else:
        ws = bi_new_workspace(B, T, C, H, dev)
    _call("wkv6bi_forward_ex", "wkv6_bi forward_ex", dev, B, T, C, H, *_ptrs(mask, lens, r, k, v, w, u, y, ws), ws.numel(), flags)
    return y


def bi_backward_ex(mask, r, k, v, w, u, gy, H, w_is_ew=False, algo=None, ws=None, lens=None):
    """ws: the workspace a preceding bi_forward_ex(..., ws=ws) on the same inputs filled (checkpoints valid)."""
    B, T, C = btc = r.shape
    io = r.dtype
    named = {**_mask_or_lens(mask, lens, B, T),
             **_named(btc, io, r, k, v, w, u, wdt=torch.float32 if w_is_ew else io, ushape=(H, HEAD_SIZE), gy=gy)}
    dev = _check_tensors(B, T, C, H, named, dtype=io)
    gr, gk, gv, gw = (torch.empty(btc, device=dev, dtype=io) for _ in range(4))
    gu = torch.empty((B, C), device=dev, dtype=torch.float32)      # per-batch partials: fp32 (WKV6_PARTIALS_F32)
    ws, valid = _workspace_or_ckpt(ws, True, io, algo, bi_new_workspace, B, T, C, H, dev)
    _call("wkv6bi_backward_ex", "wkv6_bi backward_ex", dev, B, T, C, H, *_ptrs(mask, lens, r, k, v, w, u, gy, gr, gk, gv, gw, gu, ws),
          ws.numel(), _flags(io, w_is_ew, algo) | _lib.PARTIALS_F32 | valid)
    return gr, gk, gv, gw, gu


def selftest():
    """Cross-lane primitive self-test on the current device (0 = pass)."""
    return _lib.load().wkv6_selftest(_stream_ptr())


def pass_marker():
    """Launch the empty kernel wkv6::pass_marker_kernel on the current stream (a phase boundary in a profiler's dispatch list)."""
    _lib.check(_lib.load().wkv6_pass_marker(_stream_ptr()), "wkv6_pass_marker")


_DISPATCH = {"split": 0, "bi_fused": 1, "tsplit": 2, "bi_slots": 3}      # WKV6_DISPATCH_* of include/wkv6_amd.h


@contextlib.contextmanager
def dispatch(split=None, bi_fused=None, tsplit=None, bi_slots=None):
    """Override the library's launch-shape choices for the body (wkv6_set_dispatch, include/wkv6_amd.h), process-wide; None leaves a
    choice alone.  split: != 0 forces two workgroups per (batch, head), 0 one.  bi_fused = 0: the halves of wkv6_bi as two launches.
    tsplit: 0 / 1 turns the two-level forward over T off, n forces n segments where T % (64 n) == 0.  bi_slots = n >= 1: the persistent
    wkv6_bi launches use min(n, B*H) workgroup slots (-1: min(B*H, CUs)); split and bi_fused = 0 take precedence.  The previous values
    come back on exit, exceptions included."""
    lib = _lib.load()
    given = {name: v for name, v in (("split", split), ("bi_fused", bi_fused), ("tsplit", tsplit), ("bi_slots", bi_slots))
             if v is not None}
    prev = {}
    try:
        for name, v in given.items():
            prev[name] = lib.wkv6_set_dispatch(_DISPATCH[name], int(v))
        yield
    finally:
        for name, v in prev.items():
            lib.wkv6_set_dispatch(_DISPATCH[name], v)


class ClockProbe:
    """In-run shader clock and duration of the chunked kernels' launches (wkv6_set_clock_ring, include/wkv6_amd.h): while active, wave 0
    of the first `n_slots` workgroups of every chunked forward / backward launch stamps {s_memtime, s_memrealtime} at its start and end
    into a ring of the last `n_launches` launches of each kind.

        with ClockProbe(dev, n_slots=64, n_launches=4096) as probe:
            ... launches ...
            rec = probe.read()

    read() -> {"fwd_ghz", "bwd_ghz"} (median over the workgroups of d(s_memtime) / d(s_memrealtime) x 100 MHz for the LAST launch of
    each kind, None where nothing was stamped) plus, per kind, the lists "fwd_ghz_launches" / "fwd_us_launches" (oldest first: every
    launch still in the ring; us = max(end) - min(start) of s_memrealtime over the stamped workgroups) and "fwd_count".
    The probe owns the device buffer for as long as the library holds its address: close() (also on __exit__ / __del__) switches the
    stamps off first; read() after close() returns None values."""

    def __init__(self, device, n_slots=256, n_launches=1):
        self.n, self.nl = int(n_slots), int(n_launches)
        self.lib = _lib.load()
        self.buf = torch.zeros(2 * self.nl * self.n * 4, dtype=torch.int64, device=device)
        self.lib.wkv6_set_clock_ring(self.buf.data_ptr(), self.n, self.nl)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def counts(self):
        f, b = ctypes.c_long(0), ctypes.c_long(0)
        self.lib.wkv6_clock_ring_counts(ctypes.byref(f), ctypes.byref(b))
        return f.value, b.value

    def read(self):
        out = {}
        names = ("fwd", "bwd")
        if self.buf is None:
            for nm in names:
                out[nm + "_ghz"] = None
                out[nm + "_ghz_launches"], out[nm + "_us_launches"], out[nm + "_count"] = [], [], None
            return out
        d = self.buf.view(2, self.nl, self.n, 4).cpu().double()
        cnt = self.counts()
        for i, nm in enumerate(names):
            n = cnt[i]
            order = [j % self.nl for j in range(max(0, n - self.nl), n)]
            ghz, us = [], []
            for j in order:
                s = d[i, j]
                dc, dr = s[:, 2] - s[:, 0], s[:, 3] - s[:, 1]
                ok = (dr > 0) & (s[:, 0] > 0)
                if bool(ok.any()):
                    ghz.append(round(float((dc[ok] / dr[ok]).median()) * 0.1, 3))
                    us.append(round(float(s[ok, 3].max() - s[ok, 1].min()) * 0.01, 2))
                else:
                    ghz.append(None)
                    us.append(None)
            out[nm + "_ghz_launches"], out[nm + "_us_launches"], out[nm + "_count"] = ghz, us, n
            out[nm + "_ghz"] = ghz[-1] if ghz else None
        return out

    def close(self):
        if getattr(self, "buf", None) is None:
            return
        self.lib.wkv6_set_clock_ring(None, 0, 0)
        self.buf = None


class _Wkv6Varlen:
    """torch.ops.wkv6.forward_varlen / backward_varlen: the packed operator with the in-place output convention of the ops above."""

    @staticmethod
    def forward(total_T, C, H, r, k, v, w, u, cu_seqlens, max_seqlen, y):
        if tuple(r.shape) != (total_T, C):
            raise RuntimeError(f"r has shape {tuple(r.shape)}, expected {(total_T, C)}")
        forward_varlen_ex(r, k, v, w, u, H, cu_seqlens, max_seqlen, y=y)

    @staticmethod
    def backward(total_T, C, H, r, k, v, w, u, cu_seqlens, max_seqlen, gy, gr, gk, gv, gw, gu):
        if tuple(r.shape) != (total_T, C):
            raise RuntimeError(f"r has shape {tuple(r.shape)}, expected {(total_T, C)}")
        res = backward_varlen_ex(r, k, v, w, u, gy, H, cu_seqlens, max_seqlen)
        for dst, src in zip((gr, gk, gv, gw, gu), res):
            if dst.shape != src.shape:
                raise RuntimeError(f"gradient buffer has shape {tuple(dst.shape)}, expected {tuple(src.shape)}")
            dst.copy_(src)


# ---- torch.ops registration: the TORCH_LIBRARY(wkv6|wkv6bi|wkv6state|wkv6infctx, m) blocks ------------
def _register():
    T9 = "Tensor r, Tensor k, Tensor v, Tensor w, Tensor u"
    defs = {
        "wkv6": (f"(int B, int T, int C, int H, {T9}, Tensor(a!) y) -> ()",
                 f"(int B, int T, int C, int H, {T9}, Tensor gy, Tensor(a!) gr, Tensor(b!) gk, Tensor(c!) gv, "
                 f"Tensor(d!) gw, Tensor(e!) gu) -> ()", _Wkv6),
        "wkv6bi": (f"(int B, int T, int C, int H, Tensor mask, {T9}, Tensor(a!) y) -> ()",
                   f"(int B, int T, int C, int H, Tensor mask, {T9}, Tensor gy, Tensor(a!) gr, Tensor(b!) gk, "
                   f"Tensor(c!) gv, Tensor(d!) gw, Tensor(e!) gu) -> ()", _Wkv6Bi),
        "wkv6state": (f"(int B, int T, int C, int H, {T9}, Tensor s, Tensor(a!) y) -> ()",
                      f"(int B, int T, int C, int H, {T9}, Tensor s, Tensor gy, Tensor(a!) gr, Tensor(b!) gk, "
                      f"Tensor(c!) gv, Tensor(d!) gw, Tensor(e!) gu, Tensor(f!) gs) -> ()", _Wkv6State),
        "wkv6infctx": (f"(int B, int T, int C, int H, {T9}, Tensor(z!) s, Tensor(a!) y) -> ()",
                       f"(int B, int T, int C, int H, {T9}, Tensor s, Tensor gy, Tensor(a!) gr, Tensor(b!) gk, "
                       f"Tensor(c!) gv, Tensor(d!) gw, Tensor(e!) gu, Tensor(f!) gs) -> ()", _Wkv6Infctx),
    }
    libs = []
    rw = torch.library.Library("rwkv6", "DEF")          # TORCH_LIBRARY(rwkv6, m), cuda/rwkv6_op.cpp:30-34
    for name in ("forward_bf16", "forward_fp16", "forward_fp32"):
        rw.define(name + "(int B, int T, int C, int H, Tensor(s!) state, Tensor r, Tensor k, Tensor v, Tensor w, Tensor u, "
                         "Tensor(a!) y) -> ()")
        rw.impl(name, getattr(_Rwkv6, name), "CUDA")
    libs.append(rw)
    for ns, (fwd_schema, bwd_schema, impl) in defs.items():
        lib = torch.library.Library(ns, "DEF")
        lib.define("forward" + fwd_schema)
        lib.define("backward" + bwd_schema)
        lib.impl("forward", impl.forward, "CUDA")
        lib.impl("backward", impl.backward, "CUDA")
        libs.append(lib)
    # packed variable-length batches (no counterpart in the reference): r, k, v, w [total_T,C] bf16 with the raw decay, caller-allocated
    # outputs like the ops above; gu [n_seq,C] fp32 per-sequence partials
    vl = torch.library.Library("wkv6", "FRAGMENT")
    vl.define(f"forward_varlen(int total_T, int C, int H, {T9}, Tensor cu_seqlens, int max_seqlen, Tensor(a!) y) -> ()")
    vl.define(f"backward_varlen(int total_T, int C, int H, {T9}, Tensor cu_seqlens, int max_seqlen, Tensor gy, Tensor(a!) gr, Tensor(b!) gk, "
              f"Tensor(c!) gv, Tensor(d!) gw, Tensor(e!) gu) -> ()")
    vl.impl("forward_varlen", _Wkv6Varlen.forward, "CUDA")
    vl.impl("backward_varlen", _Wkv6Varlen.backward, "CUDA")
    libs.append(vl)
    # packed stateful inference: state_pool (fp32 [n_slots,H,N,N]) and y are written; state_slot None = slot s for sequence s
    rv = torch.library.Library("rwkv6", "FRAGMENT")
    for name in ("forward_varlen_bf16", "forward_varlen_fp16", "forward_varlen_fp32"):
        rv.define(name + "(int total_T, int C, int H, Tensor(s!) state_pool, Tensor? state_slot, Tensor r, Tensor k, Tensor v, Tensor w, "
                         "Tensor u, Tensor(a!) y, Tensor cu_seqlens, int max_seqlen) -> ()")
        rv.impl(name, getattr(_Rwkv6, name), "CUDA")
    # ... with a separate output slot and state snapshots; the snapshot slots of state_pool are written too
    for name in ("forward_varlen_snap_bf16", "forward_varlen_snap_fp16", "forward_varlen_snap_fp32"):
        rv.define(name + "(int total_T, int C, int H, Tensor(s!) state_pool, Tensor? state_slot, Tensor? state_slot_out, Tensor r, Tensor k, "
                         "Tensor v, Tensor w, Tensor u, Tensor(a!) y, Tensor cu_seqlens, int max_seqlen, int snap_every, Tensor? cu_snap, "
                         "Tensor? snap_slot) -> ()")
        rv.impl(name, getattr(_Rwkv6, name), "CUDA")
    # ... and with the sequences longer than seg_len tokens cut into segments (bf16 only)
    rv.define("forward_varlen_split_bf16(int total_T, int C, int H, Tensor(s!) state_pool, Tensor? state_slot, Tensor? state_slot_out, Tensor r, "
              "Tensor k, Tensor v, Tensor w, Tensor u, Tensor(a!) y, Tensor cu_seqlens, int max_seqlen, int snap_every, Tensor? cu_snap, "
              "Tensor? snap_slot, int seg_len) -> ()")
    rv.impl("forward_varlen_split_bf16", _Rwkv6.forward_varlen_split_bf16, "CUDA")
    libs.append(rv)
    w5 = torch.library.Library("wkv5", "DEF")           # TORCH_LIBRARY(wkv5, m), cuda/wkv5_op.cpp:19-22
    w5.define("forward(int B, int T, int C, int H, Tensor r, Tensor k, Tensor v, Tensor w, Tensor u, Tensor(a!) y) -> ()")
    w5.define("backward(int B, int T, int C, int H, Tensor r, Tensor k, Tensor v, Tensor w, Tensor ww, Tensor u, Tensor gy, "
              "Tensor(a!) gr, Tensor(b!) gk, Tensor(c!) gv, Tensor(d!) gw, Tensor(e!) gu) -> ()")
    w5.impl("forward", _Wkv5.forward, "CUDA")
    w5.impl("backward", _Wkv5.backward, "CUDA")
    libs.append(w5)
    return libs


_LIBRARIES = _register()
