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
"""
import contextlib

import torch

from . import _lib

HEAD_SIZE = 64


def _stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


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
    if dev.index not in _lib._selftested:
        with torch.cuda.device(dev):
            _lib.selftest_once(dev.index, _stream_ptr())
    return dev


class _Wkv6:
    """Stand-in for the module object of `load(name="wkv6", ...)` (src/model.py:188-189)."""

    @staticmethod
    def forward(B, T, C, H, r, k, v, w, u, y):
        btc = (B, T, C)
        dev = _check_tensors(B, T, C, H, dict(r=(r, btc, None), k=(k, btc, None), v=(v, btc, None),
                                              w=(w, btc, torch.float32), u=(u, None, None), y=(y, btc, None)))
        with torch.cuda.device(dev):
            rc = _lib.load().wkv6_cuda_forward(B, T, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(u), _ptr(y),
                                               _stream_ptr())
        _lib.check(rc, "wkv6 forward")

    @staticmethod
    def backward(B, T, C, H, r, k, v, w, u, gy, gr, gk, gv, gw, gu):
        btc = (B, T, C)
        dev = _check_tensors(B, T, C, H, dict(
            r=(r, btc, None), k=(k, btc, None), v=(v, btc, None), w=(w, btc, torch.float32), u=(u, None, None),
            gy=(gy, btc, None), gr=(gr, btc, None), gk=(gk, btc, None), gv=(gv, btc, None), gw=(gw, btc, None),
            gu=(gu, (B, C), None)))
        ws = torch.empty(_lib.load().wkv6_backward_workspace_bytes(B, T, C, H), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.load().wkv6_backward_ex(B, T, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(u), None,
                                              _ptr(gy), _ptr(gr), _ptr(gk), _ptr(gv), _ptr(gw), _ptr(gu), None,
                                              _ptr(ws), ws.numel(), _lib.W_EW_F32, _stream_ptr())
        _lib.check(rc, "wkv6 backward")


class _Wkv6Bi:
    """Stand-in for `load(name="wkv6_bi", ...)` (cuda/wkv6_bi.py:7)."""

    @staticmethod
    def forward(B, T, C, H, mask, r, k, v, w, u, y):
        btc = (B, T, C)
        dev = _check_tensors(B, T, C, H, dict(mask=(mask, (B, T), torch.int32), r=(r, btc, None), k=(k, btc, None),
                                              v=(v, btc, None), w=(w, btc, torch.float32), u=(u, None, None),
                                              y=(y, btc, None)))
        ws = torch.empty(_lib.load().wkv6bi_workspace_bytes(B, T, C, H), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.load().wkv6bi_forward_ex(B, T, C, H, _ptr(mask), None, _ptr(r), _ptr(k), _ptr(v), _ptr(w),
                                               _ptr(u), _ptr(y), _ptr(ws), ws.numel(), _lib.W_EW_F32, _stream_ptr())
        _lib.check(rc, "wkv6_bi forward")

    @staticmethod
    def backward(B, T, C, H, mask, r, k, v, w, u, gy, gr, gk, gv, gw, gu):
        btc = (B, T, C)
        dev = _check_tensors(B, T, C, H, dict(
            mask=(mask, (B, T), torch.int32), r=(r, btc, None), k=(k, btc, None), v=(v, btc, None),
            w=(w, btc, torch.float32), u=(u, None, None), gy=(gy, btc, None), gr=(gr, btc, None),
            gk=(gk, btc, None), gv=(gv, btc, None), gw=(gw, btc, None), gu=(gu, (B, C), None)))
        ws = torch.empty(_lib.load().wkv6bi_workspace_bytes(B, T, C, H), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.load().wkv6bi_backward_ex(B, T, C, H, _ptr(mask), None, _ptr(r), _ptr(k), _ptr(v), _ptr(w),
                                                _ptr(u), _ptr(gy), _ptr(gr), _ptr(gk), _ptr(gv), _ptr(gw),
                                                _ptr(gu), _ptr(ws), ws.numel(), _lib.W_EW_F32, _stream_ptr())
        _lib.check(rc, "wkv6_bi backward")


class _Wkv6State:
    """Stand-in for `load(name="wkv6state", ...)` (src/model.py:134-135); s: bf16 [H,N,N]."""
    _per_batch = False
    _name = "wkv6state"

    @classmethod
    def _s_shape(cls, B, H):
        return (B, H, HEAD_SIZE, HEAD_SIZE) if cls._per_batch else (H, HEAD_SIZE, HEAD_SIZE)

    @classmethod
    def forward(cls, B, T, C, H, r, k, v, w, u, s, y):
        btc = (B, T, C)
        dev = _check_tensors(B, T, C, H, dict(r=(r, btc, None), k=(k, btc, None), v=(v, btc, None), w=(w, btc, None),
                                              u=(u, None, None), s=(s, cls._s_shape(B, H), None), y=(y, btc, None)))
        fn = getattr(_lib.load(), cls._name + "_cuda_forward")
        with torch.cuda.device(dev):
            rc = fn(B, T, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(u), _ptr(s), _ptr(y), _stream_ptr())
        _lib.check(rc, cls._name + " forward")

    @classmethod
    def backward(cls, B, T, C, H, r, k, v, w, u, s, gy, gr, gk, gv, gw, gu, gs):
        btc = (B, T, C)
        dev = _check_tensors(B, T, C, H, dict(
            r=(r, btc, None), k=(k, btc, None), v=(v, btc, None), w=(w, btc, None), u=(u, None, None),
            s=(s, cls._s_shape(B, H), None), gy=(gy, btc, None), gr=(gr, btc, None), gk=(gk, btc, None),
            gv=(gv, btc, None), gw=(gw, btc, None), gu=(gu, (B, C), None),
            gs=(gs, (B, H, HEAD_SIZE, HEAD_SIZE), None)))
        flags = _lib.W_RAW | (_lib.S0_PER_BATCH if cls._per_batch else 0)
        ws = torch.empty(_lib.load().wkv6_backward_workspace_bytes(B, T, C, H), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.load().wkv6_backward_ex(B, T, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(u), _ptr(s),
                                              _ptr(gy), _ptr(gr), _ptr(gk), _ptr(gv), _ptr(gw), _ptr(gu), _ptr(gs),
                                              _ptr(ws), ws.numel(), flags, _stream_ptr())
        _lib.check(rc, cls._name + " backward")


class _Wkv6Infctx(_Wkv6State):
    """Stand-in for `load(name="wkv6infctx", ...)` (src/model.py:80-81); s: bf16 [B,H,N,N], the forward
    overwrites it with the final state (cuda/wkv6infctx_cuda.cu:65-67)."""
    _per_batch = True
    _name = "wkv6infctx"


class _Rwkv6:
    """Stand-in for `load(name="rwkv6", ...)` (src/model_run.py:46-47): stateful forward-only kernel for inference.
    forward_bf16 / forward_fp32 (B,T,C,H, state[f32], r,k,v, eew[f32 decay], u, y); state updated in place."""

    @staticmethod
    def _call(B, T, C, H, state, r, k, v, w, u, y, io):
        btc = (B, T, C)
        sshape = None if state.numel() == B * H * HEAD_SIZE * HEAD_SIZE else (-1,)
        dev = _check_tensors(B, T, C, H, dict(state=(state, sshape, torch.float32), r=(r, btc, io), k=(k, btc, io),
                                              v=(v, btc, io), w=(w, btc, torch.float32), u=(u, None, io), y=(y, btc, io)),
                             dtype=io)
        lib = _lib.load()
        fn = {torch.bfloat16: lib.rwkv6_cuda_forward_bf16, torch.float16: lib.rwkv6_cuda_forward_fp16,
              torch.float32: lib.rwkv6_cuda_forward_fp32}[io]
        with torch.cuda.device(dev):
            rc = fn(B, T, C, H, _ptr(state), _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(u), _ptr(y), _stream_ptr())
        _lib.check(rc, "rwkv6 forward")

    @staticmethod
    def forward_bf16(B, T, C, H, state, r, k, v, w, u, y):
        _Rwkv6._call(B, T, C, H, state, r, k, v, w, u, y, torch.bfloat16)

    @staticmethod
    def forward_fp32(B, T, C, H, state, r, k, v, w, u, y):
        _Rwkv6._call(B, T, C, H, state, r, k, v, w, u, y, torch.float32)

    @staticmethod
    def forward_fp16(B, T, C, H, state, r, k, v, w, u, y):
        """cuda/rwkv6_op.cpp:16-19: r, k, v, u, y in fp16; the kernel widens the inputs to fp32 (exact), computes and carries the
        state in fp32 and rounds y to fp16 once (cuda/rwkv6.cu:8-71)."""
        _Rwkv6._call(B, T, C, H, state, r, k, v, w, u, y, torch.float16)

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
        tc = (total_T, C)
        named = dict(state_pool=(state_pool, None, torch.float32), r=(r, tc, io), k=(k, tc, io), v=(v, tc, io),
                     w=(w, tc, torch.float32), u=(u, (H, HEAD_SIZE), io), y=(y, tc, io))
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
        n_seq = _check_cu_seqlens(cu_seqlens, r.device)
        if state_slot is None:
            if n_slots < n_seq:
                raise RuntimeError(f"state_slot=None names slot s for sequence s: the pool has {n_slots} slots for {n_seq} sequences")
        elif not (isinstance(state_slot, torch.Tensor) and state_slot.dtype == torch.int32 and state_slot.is_contiguous()
                  and tuple(state_slot.shape) == (n_seq,) and state_slot.device == r.device):
            raise RuntimeError("state_slot must be a contiguous int32 [n_seq] tensor on the device of r, or None")
        if ws is not None and not (isinstance(ws, torch.Tensor) and ws.dtype == torch.uint8 and ws.is_contiguous()
                                   and ws.device == r.device):
            raise RuntimeError("ws must be a new_rwkv6_varlen_workspace() buffer on the device of r")

        def int_array(name, t, shape, what):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1
                    and (shape is None or tuple(t.shape) == shape) and t.device == r.device):
                raise RuntimeError(f"{name} must be a contiguous int32 {what} tensor on the device of r")

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
                int_array("state_slot_out", state_slot_out, (n_seq,), "[n_seq]")
            if snap_every == 0:
                if cu_snap is not None or snap_slot is not None:
                    raise RuntimeError("cu_snap and snap_slot belong to snap_every > 0")
            else:
                int_array("cu_snap", cu_snap, (n_seq + 1,), "[n_seq + 1]")
                int_array("snap_slot", snap_slot, None, "[n_snap]")
        dev = _check_tensors(n_seq, total_T, C, H, named, dtype=io)
        lib = _lib.load()
        base = (int(total_T), n_seq, int(max_seqlen), C, H, _ptr(cu_seqlens), _ptr(state_slot), n_slots, _ptr(state_pool), _ptr(r),
                _ptr(k), _ptr(v), _ptr(w), _ptr(u), _ptr(y), _ptr(ws), 0 if ws is None else ws.numel(),
                _lib.ALGO_SCAN if algo == "scan" else 0)
        with torch.cuda.device(dev):
            if split:
                rc = lib.rwkv6_forward_varlen_split_bf16(*base, _stream_ptr(), _ptr(state_slot_out), snap_every, _ptr(cu_snap), _ptr(snap_slot),
                                                         0 if snap_slot is None else snap_slot.numel(), seg_len)
            elif snap:
                fn = {torch.bfloat16: lib.rwkv6_forward_varlen_snap_bf16, torch.float16: lib.rwkv6_forward_varlen_snap_fp16,
                      torch.float32: lib.rwkv6_forward_varlen_snap_fp32}[io]
                rc = fn(*base, _stream_ptr(), _ptr(state_slot_out), snap_every, _ptr(cu_snap), _ptr(snap_slot),
                        0 if snap_slot is None else snap_slot.numel())
            else:
                fn = {torch.bfloat16: lib.rwkv6_forward_varlen_bf16, torch.float16: lib.rwkv6_forward_varlen_fp16,
                      torch.float32: lib.rwkv6_forward_varlen_fp32}[io]
                rc = fn(*base, _stream_ptr())
        _lib.check(rc, "rwkv6 forward_varlen")

    @staticmethod
    def forward_varlen_bf16(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, algo=None, ws=None,
                            state_slot_out=None, snap_every=0, cu_snap=None, snap_slot=None, seg_len=0):
        _Rwkv6._call_varlen(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, algo, ws, torch.bfloat16,
                            state_slot_out, snap_every, cu_snap, snap_slot, seg_len=seg_len)

    @staticmethod
    def forward_varlen_split_bf16(total_T, C, H, state_pool, state_slot, state_slot_out, r, k, v, w, u, y, cu_seqlens, max_seqlen, snap_every,
                                  cu_snap, snap_slot, seg_len, ws=None):
        """torch.ops.rwkv6.forward_varlen_split_bf16: always the split entry point of the library, seg_len = 0 included."""
        _Rwkv6._call_varlen(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, None, ws, torch.bfloat16,
                            state_slot_out, snap_every, cu_snap, snap_slot, seg_len=seg_len, force_split=True)

    @staticmethod
    def forward_varlen_snap_bf16(total_T, C, H, state_pool, state_slot, state_slot_out, r, k, v, w, u, y, cu_seqlens, max_seqlen, snap_every,
                                 cu_snap, snap_slot):
        """torch.ops.rwkv6.forward_varlen_snap_bf16: always the snap entry point of the library, defaults included."""
        _Rwkv6._call_varlen(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, None, None, torch.bfloat16,
                            state_slot_out, snap_every, cu_snap, snap_slot, force_snap=True)

    @staticmethod
    def forward_varlen_fp16(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, algo=None, ws=None,
                            state_slot_out=None, snap_every=0, cu_snap=None, snap_slot=None):
        _Rwkv6._call_varlen(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, algo, ws, torch.float16,
                            state_slot_out, snap_every, cu_snap, snap_slot)

    @staticmethod
    def forward_varlen_snap_fp16(total_T, C, H, state_pool, state_slot, state_slot_out, r, k, v, w, u, y, cu_seqlens, max_seqlen, snap_every,
                                 cu_snap, snap_slot):
        """torch.ops.rwkv6.forward_varlen_snap_fp16: always the snap entry point of the library, defaults included."""
        _Rwkv6._call_varlen(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, None, None, torch.float16,
                            state_slot_out, snap_every, cu_snap, snap_slot, force_snap=True)

    @staticmethod
    def forward_varlen_fp32(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, algo=None, ws=None,
                            state_slot_out=None, snap_every=0, cu_snap=None, snap_slot=None):
        _Rwkv6._call_varlen(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, algo, ws, torch.float32,
                            state_slot_out, snap_every, cu_snap, snap_slot)

    @staticmethod
    def forward_varlen_snap_fp32(total_T, C, H, state_pool, state_slot, state_slot_out, r, k, v, w, u, y, cu_seqlens, max_seqlen, snap_every,
                                 cu_snap, snap_slot):
        """torch.ops.rwkv6.forward_varlen_snap_fp32: always the snap entry point of the library, defaults included."""
        _Rwkv6._call_varlen(total_T, C, H, state_pool, state_slot, r, k, v, w, u, y, cu_seqlens, max_seqlen, None, None, torch.float32,
                            state_slot_out, snap_every, cu_snap, snap_slot, force_snap=True)


class _Wkv5:
    """Stand-in for the module object of `load(name="wkv5", ...)` (src/model.py:238-239): the RWKV-5 operator, whose decay is an
    [H,N] parameter.  forward (B,T,C,H, r,k,v, eew[f32 decay], u, y); backward(B,T,C,H, r,k,v, eew, ew[f32], u, gy, gr,gk,gv,
    gw[B,C], gu[B,C])  (cuda/wkv5_op.cpp:8-13)."""

    @staticmethod
    def forward(B, T, C, H, r, k, v, w, u, y):
        btc, hn = (B, T, C), (H, HEAD_SIZE)
        dev = _check_tensors(B, T, C, H, dict(r=(r, btc, None), k=(k, btc, None), v=(v, btc, None),
                                              w=(w, hn, torch.float32), u=(u, hn, None), y=(y, btc, None)))
        with torch.cuda.device(dev):
            rc = _lib.load().wkv5_cuda_forward(B, T, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(u), _ptr(y), _stream_ptr())
        _lib.check(rc, "wkv5 forward")

    @staticmethod
    def backward(B, T, C, H, r, k, v, w, ww, u, gy, gr, gk, gv, gw, gu):
        btc, hn = (B, T, C), (H, HEAD_SIZE)
        dev = _check_tensors(B, T, C, H, dict(
            r=(r, btc, None), k=(k, btc, None), v=(v, btc, None), w=(w, hn, torch.float32), ww=(ww, hn, torch.float32),
            u=(u, hn, None), gy=(gy, btc, None), gr=(gr, btc, None), gk=(gk, btc, None), gv=(gv, btc, None),
            gw=(gw, (B, C), None), gu=(gu, (B, C), None)))
        with torch.cuda.device(dev):
            rc = _lib.load().wkv5_cuda_backward(B, T, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(ww), _ptr(u), _ptr(gy),
                                                _ptr(gr), _ptr(gk), _ptr(gv), _ptr(gw), _ptr(gu), _stream_ptr())
        _lib.check(rc, "wkv5 backward")


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
    B, T, C = r.shape
    io = r.dtype
    if io not in (torch.bfloat16, torch.float32):
        raise RuntimeError(f"unsupported I/O dtype {io}")
    btc = (B, T, C)
    wdt = torch.float32 if w_is_ew else io
    named = dict(r=(r, btc, io), k=(k, btc, io), v=(v, btc, io), w=(w, btc, wdt), u=(u, (H, HEAD_SIZE), io))
    flags = (_lib.W_EW_F32 if w_is_ew else _lib.W_RAW) | (_lib.IO_F32 if io == torch.float32 else 0)
    flags |= _lib.ALGO_SCAN if algo == "scan" else 0
    if s0 is not None:
        per_batch = s0.dim() == 4
        named["s0"] = (s0, (B, H, HEAD_SIZE, HEAD_SIZE) if per_batch else (H, HEAD_SIZE, HEAD_SIZE), io)
        flags |= _lib.S0_PER_BATCH if per_batch else 0
    if s_out is not None:
        named["s_out"] = (s_out, (B, H, HEAD_SIZE, HEAD_SIZE), io)
    if y is None:
        y = torch.empty(btc, device=r.device, dtype=io)
    named["y"] = (y, btc, io)
    dev = _check_tensors(B, T, C, H, named, dtype=io)
    with torch.cuda.device(dev):
        if ckpt is not None:       # training forward: also store the per-group state checkpoints for the backward
            rc = _lib.load().wkv6_forward_ckpt_ex(B, T, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(u), _ptr(s0),
                                                  _ptr(s_out), _ptr(y), _ptr(ckpt), ckpt.numel(), flags, _stream_ptr())
        else:
            rc = _lib.load().wkv6_forward_ex(B, T, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(u), _ptr(s0),
                                             _ptr(s_out), _ptr(y), flags, _stream_ptr())
    _lib.check(rc, "wkv6 forward_ex")
    return y


def forward_gn_ex(r, k, v, w, u, H, gate, gamma, beta, eps, ckpt=None, want_y=True, want_stats=True):
    """The operator with the time-mix block's GroupNorm(H) * gate epilogue fused into its store (src/model.py:462-468, SURVEY.md
    row n1).  Returns (out, y or None, stats or None), or None where the library cannot fuse (so few (batch, head) pairs that
    two workgroups share one): the caller then runs the two kernels."""
    B, T, C = r.shape
    bf = torch.bfloat16
    btc = (B, T, C)
    named = dict(r=(r, btc, bf), k=(k, btc, bf), v=(v, btc, bf), w=(w, btc, bf), u=(u, (H, HEAD_SIZE), bf),
                 gate=(gate, btc, bf), gamma=(gamma, (C,), bf), beta=(beta, (C,), bf))
    dev = _check_tensors(B, T, C, H, named, dtype=bf)
    out = torch.empty(btc, device=dev, dtype=bf)
    y = torch.empty(btc, device=dev, dtype=bf) if want_y else None
    stats = torch.empty((B * T, H, 2), device=dev, dtype=torch.float32) if want_stats else None
    with torch.cuda.device(dev):
        rc = _lib.load().wkv6_forward_gn_ex(B, T, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(u), None, None, _ptr(y),
                                            _ptr(ckpt), 0 if ckpt is None else ckpt.numel(), _ptr(gate), _ptr(gamma), _ptr(beta),
                                            float(eps), _ptr(out), _ptr(stats), _lib.W_RAW, _stream_ptr())
    if rc == _lib.EUNSUPPORTED:
        return None
    _lib.check(rc, "wkv6 forward_gn_ex")
    return out, y, stats


def backward_ex(r, k, v, w, u, gy, H, s0=None, w_is_ew=False, want_gs=False, algo=None, ckpt=None):
    """Returns (gr, gk, gv, gw, gu[B,C], gs[B,H,N,N] or None): gradients in the I/O type of `r`, the per-batch partials gu / gs
    in fp32 (WKV6_PARTIALS_F32)."""
    B, T, C = r.shape
    io = r.dtype
    btc = (B, T, C)
    wdt = torch.float32 if w_is_ew else io
    named = dict(r=(r, btc, io), k=(k, btc, io), v=(v, btc, io), w=(w, btc, wdt), u=(u, (H, HEAD_SIZE), io),
                 gy=(gy, btc, io))
    flags = (_lib.W_EW_F32 if w_is_ew else _lib.W_RAW) | (_lib.IO_F32 if io == torch.float32 else 0)
    flags |= _lib.ALGO_SCAN if algo == "scan" else 0
    if s0 is not None:
        per_batch = s0.dim() == 4
        named["s0"] = (s0, (B, H, HEAD_SIZE, HEAD_SIZE) if per_batch else (H, HEAD_SIZE, HEAD_SIZE), io)
        flags |= _lib.S0_PER_BATCH if per_batch else 0
    dev = _check_tensors(B, T, C, H, named, dtype=io)
    gr, gk, gv, gw = (torch.empty(btc, device=dev, dtype=io) for _ in range(4))
    # gu / gs are per-batch partial sums the caller reduces: always fp32, so that the parameter gradient is rounded once
    flags |= _lib.PARTIALS_F32
    gu = torch.empty((B, C), device=dev, dtype=torch.float32)
    gs = torch.empty((B, H, HEAD_SIZE, HEAD_SIZE), device=dev, dtype=torch.float32) if want_gs else None
    if ckpt is not None:           # checkpoints written by forward_ex(..., ckpt=ckpt) on the same inputs
        ws = ckpt
        flags |= _lib.CKPT_VALID
    else:
        ws = torch.empty(_lib.load().wkv6_backward_workspace_bytes(B, T, C, H), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv6_backward_ex(B, T, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(u), _ptr(s0),
                                          _ptr(gy), _ptr(gr), _ptr(gk), _ptr(gv), _ptr(gw), _ptr(gu), _ptr(gs),
                                          _ptr(ws), ws.numel(), flags, _stream_ptr())
    _lib.check(rc, "wkv6 backward_ex")
    return gr, gk, gv, gw, gu, gs


# ---- packed variable-length batches (include/wkv6_amd.h: wkv6_*_varlen_ex) ----
def _check_cu_seqlens(cu_seqlens, dev):
    if not (isinstance(cu_seqlens, torch.Tensor) and cu_seqlens.dtype == torch.int32 and cu_seqlens.is_contiguous()
            and cu_seqlens.dim() == 1 and cu_seqlens.numel() >= 2 and cu_seqlens.device == dev):
        raise RuntimeError("cu_seqlens must be a contiguous int32 [n_seq + 1] tensor on the device of r")
    return cu_seqlens.numel() - 1


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


def _varlen_common(r, k, v, w, u, H, cu_seqlens, max_seqlen, s0, w_is_ew, algo, extra):
    if r.dim() != 2:
        raise RuntimeError("packed tensors are [total_T, C]")
    total, C = r.shape
    io = r.dtype
    if io not in (torch.bfloat16, torch.float32):
        raise RuntimeError(f"unsupported I/O dtype {io}")
    tc = (total, C)
    wdt = torch.float32 if w_is_ew else io
    named = dict(r=(r, tc, io), k=(k, tc, io), v=(v, tc, io), w=(w, tc, wdt), u=(u, (H, HEAD_SIZE), io))
    for name, t in extra.items():
        named[name] = (t, tc, io)
    flags = (_lib.W_EW_F32 if w_is_ew else _lib.W_RAW) | (_lib.IO_F32 if io == torch.float32 else 0)
    flags |= _lib.ALGO_SCAN if algo == "scan" else 0
    n_seq = _check_cu_seqlens(cu_seqlens, r.device)
    if s0 is not None:
        per_seq = s0.dim() == 4
        named["s0"] = (s0, (n_seq, H, HEAD_SIZE, HEAD_SIZE) if per_seq else (H, HEAD_SIZE, HEAD_SIZE), io)
        flags |= _lib.S0_PER_BATCH if per_seq else 0
    if int(max_seqlen) < 1:
        raise RuntimeError("max_seqlen must be >= 1")
    return total, C, io, n_seq, named, flags


def forward_varlen_ex(r, k, v, w, u, H, cu_seqlens, max_seqlen, s0=None, s_out=None, w_is_ew=False, y=None, algo=None, ws=None):
    """y [total_T,C] = WKV6 of every sequence of a packed batch on its own (sequence s = rows cu_seqlens[s] .. cu_seqlens[s+1]-1, each
    from s0).  ws: a new_varlen_workspace() buffer that keeps the state checkpoints for backward_varlen_ex(..., ws=ws, ckpt_valid=True)."""
    total, C, io, n_seq, named, flags = _varlen_common(r, k, v, w, u, H, cu_seqlens, max_seqlen, s0, w_is_ew, algo, {})
    if s_out is not None:
        named["s_out"] = (s_out, (n_seq, H, HEAD_SIZE, HEAD_SIZE), io)
    if y is None:
        y = torch.empty((total, C), device=r.device, dtype=io)
    named["y"] = (y, (total, C), io)
    dev = _check_tensors(n_seq, total, C, H, named, dtype=io)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv6_forward_varlen_ex(total, n_seq, int(max_seqlen), C, H, _ptr(cu_seqlens), _ptr(r), _ptr(k), _ptr(v),
                                                _ptr(w), _ptr(u), _ptr(s0), _ptr(s_out), _ptr(y), _ptr(ws),
                                                0 if ws is None else ws.numel(), flags, _stream_ptr())
    _lib.check(rc, "wkv6 forward_varlen_ex")
    return y


def backward_varlen_ex(r, k, v, w, u, gy, H, cu_seqlens, max_seqlen, s0=None, w_is_ew=False, want_gs=False, algo=None, ws=None,
                       ckpt_valid=False):
    """Returns (gr, gk, gv, gw [total_T,C], gu [n_seq,C], gs [n_seq,H,N,N] or None); gu / gs are fp32 per-sequence partials
    (WKV6_PARTIALS_F32) for the caller to sum.  ckpt_valid: `ws` was filled by forward_varlen_ex(..., ws=ws) on the same inputs."""
    total, C, io, n_seq, named, flags = _varlen_common(r, k, v, w, u, H, cu_seqlens, max_seqlen, s0, w_is_ew, algo, {"gy": gy})
    dev = _check_tensors(n_seq, total, C, H, named, dtype=io)
    gr, gk, gv, gw = (torch.empty((total, C), device=dev, dtype=io) for _ in range(4))
    flags |= _lib.PARTIALS_F32
    gu = torch.empty((n_seq, C), device=dev, dtype=torch.float32)
    gs = torch.empty((n_seq, H, HEAD_SIZE, HEAD_SIZE), device=dev, dtype=torch.float32) if want_gs else None
    if ckpt_valid:
        if ws is None:
            raise RuntimeError("ckpt_valid needs the workspace the forward filled")
        if io == torch.bfloat16 and algo != "scan":
            flags |= _lib.CKPT_VALID
    if ws is None:
        ws = new_varlen_workspace(total, n_seq, C, H, dev)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv6_backward_varlen_ex(total, n_seq, int(max_seqlen), C, H, _ptr(cu_seqlens), _ptr(r), _ptr(k), _ptr(v),
                                                 _ptr(w), _ptr(u), _ptr(s0), _ptr(gy), _ptr(gr), _ptr(gk), _ptr(gv), _ptr(gw),
                                                 _ptr(gu), _ptr(gs), _ptr(ws), ws.numel(), flags, _stream_ptr())
    _lib.check(rc, "wkv6 backward_varlen_ex")
    return gr, gk, gv, gw, gu, gs


def wkv5_forward_ex(r, k, v, w, u, H, y=None):
    """y = WKV5(r,k,v,w,u): w, u [H,N] raw parameters in the I/O type of `r` (bf16, or fp32 for numerics tests)."""
    B, T, C = r.shape
    io = r.dtype
    if io not in (torch.bfloat16, torch.float32):
        raise RuntimeError(f"unsupported I/O dtype {io}")
    btc, hn = (B, T, C), (H, HEAD_SIZE)
    if y is None:
        y = torch.empty(btc, device=r.device, dtype=io)
    dev = _check_tensors(B, T, C, H, dict(r=(r, btc, io), k=(k, btc, io), v=(v, btc, io), w=(w, hn, io), u=(u, hn, io),
                                          y=(y, btc, io)), dtype=io)
    flags = _lib.W_RAW | (_lib.IO_F32 if io == torch.float32 else 0)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv5_forward_ex(B, T, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(u), _ptr(y), flags, _stream_ptr())
    _lib.check(rc, "wkv5 forward_ex")
    return y


def wkv5_backward_ex(r, k, v, w, u, gy, H):
    """Returns (gr, gk, gv, gw[B,C], gu[B,C]): gradients in the I/O type of `r`, the per-batch partials gw (with respect to the raw
    w) and gu in fp32 (WKV6_PARTIALS_F32), for the caller to sum over the batch and round once."""
    B, T, C = r.shape
    io = r.dtype
    btc, hn = (B, T, C), (H, HEAD_SIZE)
    dev = _check_tensors(B, T, C, H, dict(r=(r, btc, io), k=(k, btc, io), v=(v, btc, io), w=(w, hn, io), u=(u, hn, io),
                                          gy=(gy, btc, io)), dtype=io)
    gr, gk, gv = (torch.empty(btc, device=dev, dtype=io) for _ in range(3))
    gw, gu = (torch.empty((B, C), device=dev, dtype=torch.float32) for _ in range(2))
    flags = _lib.W_RAW | _lib.PARTIALS_F32 | (_lib.IO_F32 if io == torch.float32 else 0)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv5_backward_ex(B, T, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), None, _ptr(u), _ptr(gy), _ptr(gr),
                                          _ptr(gk), _ptr(gv), _ptr(gw), _ptr(gu), flags, _stream_ptr())
    _lib.check(rc, "wkv5 backward_ex")
    return gr, gk, gv, gw, gu


REV_R, REV_K, REV_V, REV_W, REV_Y, REV_ALL = _lib.REV_R, _lib.REV_K, _lib.REV_V, _lib.REV_W, _lib.REV_Y, _lib.REV_ALL


def _check_rev(B, rev_n, rev_mask, dev):
    if not (isinstance(rev_n, torch.Tensor) and rev_n.dtype == torch.int32 and rev_n.is_contiguous() and
            tuple(rev_n.shape) == (B,) and rev_n.device == dev):
        raise RuntimeError("rev_n must be a contiguous int32 [B] tensor on the device of r")
    if rev_mask & ~REV_ALL:
        raise RuntimeError(f"rev_mask {rev_mask} has unknown bits")


def forward_rev_ex(r, k, v, w, u, H, rev_n, rev_mask, y=None, ckpt=None, algo=None):
    """WKV6 over partially reversed sequences without materialising the reversal (include/wkv6_amd.h, wkv6_forward_rev_ex):
    tokens [0, rev_n[b]) of the tensors named in `rev_mask` (REV_R | REV_K | REV_V | REV_W | REV_Y) are taken in reverse
    order, the rest in place.  I/O type of `r`: bf16 (chunked MFMA kernels; algo="scan" forces the exact ones) or fp32 (exact
    scan kernels)."""
    B, T, C = r.shape
    btc, io = (B, T, C), r.dtype
    if io not in (torch.bfloat16, torch.float32):
        raise RuntimeError(f"unsupported I/O dtype {io}")
    if y is None:
        y = torch.empty(btc, device=r.device, dtype=io)
    named = dict(r=(r, btc, io), k=(k, btc, io), v=(v, btc, io), w=(w, btc, io), u=(u, (H, HEAD_SIZE), io), y=(y, btc, io))
    dev = _check_tensors(B, T, C, H, named, dtype=io)
    _check_rev(B, rev_n, rev_mask, dev)
    flags = _lib.W_RAW | (_lib.IO_F32 if io == torch.float32 else 0) | (_lib.ALGO_SCAN if algo == "scan" else 0)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv6_forward_rev_ex(B, T, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(u), _ptr(y), _ptr(ckpt),
                                             0 if ckpt is None else ckpt.numel(), _ptr(rev_n), rev_mask, flags,
                                             _stream_ptr())
    _lib.check(rc, "wkv6 forward_rev_ex")
    return y


def _pair_sets(B, T, C, H, sets, u, bwd):
    """Check and pack the two problems of a pair launch.  sets: two dicts with r, k, v, w (+ y | gy), ckpt, rev_n, rev_mask."""
    bf = torch.bfloat16
    btc = (B, T, C)
    arr = (_lib.SeqSet * 2)()
    keep = []                                   # tensors the packed pointers refer to
    dev = None
    for i, q in enumerate(sets):
        named = {n: (q[n], btc, bf) for n in ("r", "k", "v", "w") + (("gy",) if bwd else ("y",))}
        named["u"] = (u, (H, HEAD_SIZE), bf)
        dev = _check_tensors(B, T, C, H, named, dtype=bf)
        rev_n, rev_mask = q.get("rev_n"), q.get("rev_mask", 0)
        if rev_n is not None:
            _check_rev(B, rev_n, rev_mask, dev)
        ckpt = q.get("ckpt")
        if bwd and ckpt is None:
            raise RuntimeError("wkv6 pair backward: both problems need the checkpoints their forward wrote")
        e = arr[i]
        e.r, e.k, e.v, e.w = _ptr(q["r"]), _ptr(q["k"]), _ptr(q["v"]), _ptr(q["w"])
        if bwd:
            outs = [torch.empty(btc, device=dev, dtype=bf) for _ in range(4)] + [torch.empty((B, C), device=dev, dtype=torch.float32)]
            e.gy, e.gr, e.gk, e.gv, e.gw, e.gu = (_ptr(t) for t in [q["gy"]] + outs)
            keep.append(outs)
        else:
            e.y = _ptr(q["y"])
        e.ckpt, e.ckpt_bytes = _ptr(ckpt), 0 if ckpt is None else ckpt.numel()
        e.rev_n, e.rev_mask = _ptr(rev_n), rev_mask if rev_n is not None else 0
    return arr, keep, dev


def forward_pair_ex(H, u, sets):
    """Both operator calls of a bidirectional time-mix layer in one launch (include/wkv6_amd.h, wkv6_forward_pair_ex; SURVEY.md
    row n2): `sets` = two dicts {r, k, v, w, [y], [ckpt], [rev_n, rev_mask]} of one shape.  Returns (y0, y1)."""
    B, T, C = sets[0]["r"].shape
    for q in sets:
        if q.get("y") is None:
            q["y"] = torch.empty((B, T, C), device=q["r"].device, dtype=torch.bfloat16)
    arr, _, dev = _pair_sets(B, T, C, H, sets, u, bwd=False)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv6_forward_pair_ex(B, T, C, H, _ptr(u), arr, _lib.W_RAW, _stream_ptr())
    _lib.check(rc, "wkv6 forward_pair_ex")
    return sets[0]["y"], sets[1]["y"]


def backward_pair_ex(H, u, sets):
    """Gradients of forward_pair_ex: two tuples (gr, gk, gv, gw, gu[B,C] fp32), one per problem; `sets` as in the forward plus gy."""
    B, T, C = sets[0]["r"].shape
    arr, keep, dev = _pair_sets(B, T, C, H, sets, u, bwd=True)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv6_backward_pair_ex(B, T, C, H, _ptr(u), arr, _lib.W_RAW | _lib.PARTIALS_F32, _stream_ptr())
    _lib.check(rc, "wkv6 backward_pair_ex")
    return tuple(keep[0]), tuple(keep[1])


def backward_rev_ex(r, k, v, w, u, gy, H, rev_n, rev_mask, ckpt=None, algo=None):
    """Gradients of forward_rev_ex: (gr, gk, gv, gw, gu[B,C]); each gradient is laid out like its tensor."""
    B, T, C = r.shape
    btc, io = (B, T, C), r.dtype
    if io not in (torch.bfloat16, torch.float32):
        raise RuntimeError(f"unsupported I/O dtype {io}")
    named = dict(r=(r, btc, io), k=(k, btc, io), v=(v, btc, io), w=(w, btc, io), u=(u, (H, HEAD_SIZE), io), gy=(gy, btc, io))
    dev = _check_tensors(B, T, C, H, named, dtype=io)
    _check_rev(B, rev_n, rev_mask, dev)
    gr, gk, gv, gw = (torch.empty(btc, device=dev, dtype=io) for _ in range(4))
    gu = torch.empty((B, C), device=dev, dtype=torch.float32)
    exact = io == torch.float32 or algo == "scan"
    flags = _lib.W_RAW | _lib.PARTIALS_F32 | (_lib.IO_F32 if io == torch.float32 else 0) | (_lib.ALGO_SCAN if algo == "scan" else 0)
    if ckpt is not None and not exact:
        ws = ckpt
        flags |= _lib.CKPT_VALID
    else:
        ws = torch.empty(_lib.load().wkv6_backward_workspace_bytes(B, T, C, H), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv6_backward_rev_ex(B, T, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(u), _ptr(gy), _ptr(gr),
                                              _ptr(gk), _ptr(gv), _ptr(gw), _ptr(gu), _ptr(ws), ws.numel(), _ptr(rev_n),
                                              rev_mask, flags, _stream_ptr())
    _lib.check(rc, "wkv6 backward_rev_ex")
    return gr, gk, gv, gw, gu


# ---- reversal maps and the pair launch on packed batches (include/wkv6_amd.h: wkv6_*_varlen_rev_ex, wkv6_*_varlen_pair_ex) ----
def _check_rev_varlen(n_seq, rev_n, rev_mask, dev):
    if rev_n is not None and not (isinstance(rev_n, torch.Tensor) and rev_n.dtype == torch.int32 and rev_n.is_contiguous() and
                                  tuple(rev_n.shape) == (n_seq,) and rev_n.device == dev):
        raise RuntimeError("rev_n must be a contiguous int32 [n_seq] tensor on the device of r")
    if rev_mask & ~REV_ALL:
        raise RuntimeError(f"rev_mask {rev_mask} has unknown bits")


def forward_varlen_rev_ex(r, k, v, w, u, H, cu_seqlens, max_seqlen, rev_n, rev_mask, y=None, algo=None, ws=None, w_is_ew=False):
    """forward_varlen_ex with the per-tensor reversal map of forward_rev_ex applied within every sequence: rev_n int32 [n_seq] (clamped to
    the sequence's length on the device; None: no map).  No initial state.  ws: a new_varlen_workspace() buffer that keeps the checkpoints
    for backward_varlen_rev_ex(..., ws=ws, ckpt_valid=True)."""
    total, C, io, n_seq, named, flags = _varlen_common(r, k, v, w, u, H, cu_seqlens, max_seqlen, None, w_is_ew, algo, {})
    if y is None:
        y = torch.empty((total, C), device=r.device, dtype=io)
    named["y"] = (y, (total, C), io)
    dev = _check_tensors(n_seq, total, C, H, named, dtype=io)
    _check_rev_varlen(n_seq, rev_n, rev_mask, dev)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv6_forward_varlen_rev_ex(total, n_seq, int(max_seqlen), C, H, _ptr(cu_seqlens), _ptr(r), _ptr(k), _ptr(v),
                                                    _ptr(w), _ptr(u), _ptr(y), _ptr(ws), 0 if ws is None else ws.numel(),
                                                    _ptr(rev_n), rev_mask, flags, _stream_ptr())
    _lib.check(rc, "wkv6 forward_varlen_rev_ex")
    return y


def backward_varlen_rev_ex(r, k, v, w, u, gy, H, cu_seqlens, max_seqlen, rev_n, rev_mask, algo=None, ws=None, ckpt_valid=False,
                           w_is_ew=False):
    """Gradients of forward_varlen_rev_ex: (gr, gk, gv, gw [total_T,C], gu [n_seq,C] fp32 per-sequence partials); each gradient is laid
    out like its tensor.  ckpt_valid: `ws` was filled by forward_varlen_rev_ex(..., ws=ws) on the same inputs."""
    total, C, io, n_seq, named, flags = _varlen_common(r, k, v, w, u, H, cu_seqlens, max_seqlen, None, w_is_ew, algo, {"gy": gy})
    dev = _check_tensors(n_seq, total, C, H, named, dtype=io)
    _check_rev_varlen(n_seq, rev_n, rev_mask, dev)
    gr, gk, gv, gw = (torch.empty((total, C), device=dev, dtype=io) for _ in range(4))
    flags |= _lib.PARTIALS_F32
    gu = torch.empty((n_seq, C), device=dev, dtype=torch.float32)
    if ckpt_valid:
        if ws is None:
            raise RuntimeError("ckpt_valid needs the workspace the forward filled")
        if io == torch.bfloat16 and algo != "scan":
            flags |= _lib.CKPT_VALID
    if ws is None:
        ws = new_varlen_workspace(total, n_seq, C, H, dev)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv6_backward_varlen_rev_ex(total, n_seq, int(max_seqlen), C, H, _ptr(cu_seqlens), _ptr(r), _ptr(k), _ptr(v),
                                                     _ptr(w), _ptr(u), _ptr(gy), _ptr(gr), _ptr(gk), _ptr(gv), _ptr(gw), _ptr(gu),
                                                     _ptr(ws), ws.numel(), _ptr(rev_n), rev_mask, flags, _stream_ptr())
    _lib.check(rc, "wkv6 backward_varlen_rev_ex")
    return gr, gk, gv, gw, gu


def _varlen_pair_sets(total, C, H, n_seq, sets, u, bwd):
    """_pair_sets for packed problems: tensors [total_T, C], rev_n [n_seq], ckpt = a new_varlen_workspace() buffer per problem."""
    bf = torch.bfloat16
    tc = (total, C)
    arr = (_lib.SeqSet * 2)()
    keep = []
    dev = None
    for i, q in enumerate(sets):
        named = {n: (q[n], tc, bf) for n in ("r", "k", "v", "w") + (("gy",) if bwd else ("y",))}
        named["u"] = (u, (H, HEAD_SIZE), bf)
        dev = _check_tensors(n_seq, total, C, H, named, dtype=bf)
        rev_n, rev_mask = q.get("rev_n"), q.get("rev_mask", 0)
        _check_rev_varlen(n_seq, rev_n, rev_mask, dev)
        ckpt = q.get("ckpt")
        if bwd and ckpt is None:
            raise RuntimeError("wkv6 packed pair backward: both problems need the workspaces their forward wrote")
        e = arr[i]
        e.r, e.k, e.v, e.w = _ptr(q["r"]), _ptr(q["k"]), _ptr(q["v"]), _ptr(q["w"])
        if bwd:
            outs = [torch.empty(tc, device=dev, dtype=bf) for _ in range(4)] + [torch.empty((n_seq, C), device=dev, dtype=torch.float32)]
            e.gy, e.gr, e.gk, e.gv, e.gw, e.gu = (_ptr(t) for t in [q["gy"]] + outs)
            keep.append(outs)
        else:
            e.y = _ptr(q["y"])
        e.ckpt, e.ckpt_bytes = _ptr(ckpt), 0 if ckpt is None else ckpt.numel()
        e.rev_n, e.rev_mask = _ptr(rev_n), rev_mask if rev_n is not None else 0
    return arr, keep, dev


def forward_varlen_pair_ex(H, u, sets, cu_seqlens, max_seqlen):
    """forward_pair_ex on a packed batch: `sets` = two dicts {r, k, v, w [total_T,C], [y], [ckpt], [rev_n [n_seq], rev_mask]} over the
    same sequences; ckpt is one new_varlen_workspace() buffer per problem.  Returns (y0, y1)."""
    if sets[0]["r"].dim() != 2:
        raise RuntimeError("packed tensors are [total_T, C]")
    total, C = sets[0]["r"].shape
    n_seq = _check_cu_seqlens(cu_seqlens, sets[0]["r"].device)
    if int(max_seqlen) < 1:
        raise RuntimeError("max_seqlen must be >= 1")
    for q in sets:
        if q.get("y") is None:
            q["y"] = torch.empty((total, C), device=q["r"].device, dtype=torch.bfloat16)
    arr, _, dev = _varlen_pair_sets(total, C, H, n_seq, sets, u, bwd=False)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv6_forward_varlen_pair_ex(total, n_seq, int(max_seqlen), C, H, _ptr(cu_seqlens), _ptr(u), arr, _lib.W_RAW,
                                                     _stream_ptr())
    _lib.check(rc, "wkv6 forward_varlen_pair_ex")
    return sets[0]["y"], sets[1]["y"]


def backward_varlen_pair_ex(H, u, sets, cu_seqlens, max_seqlen):
    """Gradients of forward_varlen_pair_ex: two tuples (gr, gk, gv, gw, gu [n_seq,C] fp32), one per problem; `sets` as in the forward
    (with the workspaces it filled) plus gy."""
    if sets[0]["r"].dim() != 2:
        raise RuntimeError("packed tensors are [total_T, C]")
    total, C = sets[0]["r"].shape
    n_seq = _check_cu_seqlens(cu_seqlens, sets[0]["r"].device)
    if int(max_seqlen) < 1:
        raise RuntimeError("max_seqlen must be >= 1")
    arr, keep, dev = _varlen_pair_sets(total, C, H, n_seq, sets, u, bwd=True)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv6_backward_varlen_pair_ex(total, n_seq, int(max_seqlen), C, H, _ptr(cu_seqlens), _ptr(u), arr,
                                                      _lib.W_RAW | _lib.PARTIALS_F32, _stream_ptr())
    _lib.check(rc, "wkv6 backward_varlen_pair_ex")
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
    B, T, C = r.shape
    io = r.dtype
    btc = (B, T, C)
    wdt = torch.float32 if w_is_ew else io
    named = dict(**_mask_or_lens(mask, lens, B, T), r=(r, btc, io), k=(k, btc, io), v=(v, btc, io),
                 w=(w, btc, wdt), u=(u, (H, HEAD_SIZE), io))
    flags = (_lib.W_EW_F32 if w_is_ew else _lib.W_RAW) | (_lib.IO_F32 if io == torch.float32 else 0)
    flags |= _lib.ALGO_SCAN if algo == "scan" else 0
    dev = _check_tensors(B, T, C, H, named, dtype=io)
    y = torch.empty(btc, device=dev, dtype=io)
    if ws is not None:
        flags |= _lib.BI_KEEP_CKPT
    else:
        ws = bi_new_workspace(B, T, C, H, dev)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv6bi_forward_ex(B, T, C, H, _ptr(mask), _ptr(lens), _ptr(r), _ptr(k), _ptr(v), _ptr(w),
                                           _ptr(u), _ptr(y), _ptr(ws), ws.numel(), flags, _stream_ptr())
    _lib.check(rc, "wkv6_bi forward_ex")
    return y


def bi_backward_ex(mask, r, k, v, w, u, gy, H, w_is_ew=False, algo=None, ws=None, lens=None):
    """ws: the workspace a preceding bi_forward_ex(..., ws=ws) on the same inputs filled (checkpoints valid)."""
    B, T, C = r.shape
    io = r.dtype
    btc = (B, T, C)
    wdt = torch.float32 if w_is_ew else io
    named = dict(**_mask_or_lens(mask, lens, B, T), r=(r, btc, io), k=(k, btc, io), v=(v, btc, io),
                 w=(w, btc, wdt), u=(u, (H, HEAD_SIZE), io), gy=(gy, btc, io))
    flags = (_lib.W_EW_F32 if w_is_ew else _lib.W_RAW) | (_lib.IO_F32 if io == torch.float32 else 0)
    flags |= _lib.ALGO_SCAN if algo == "scan" else 0
    dev = _check_tensors(B, T, C, H, named, dtype=io)
    gr, gk, gv, gw = (torch.empty(btc, device=dev, dtype=io) for _ in range(4))
    gu = torch.empty((B, C), device=dev, dtype=torch.float32)      # per-batch partials: fp32 (WKV6_PARTIALS_F32)
    flags |= _lib.PARTIALS_F32
    if ws is not None and io == torch.bfloat16 and algo != "scan":
        flags |= _lib.CKPT_VALID
    elif ws is None:
        ws = bi_new_workspace(B, T, C, H, dev)
    with torch.cuda.device(dev):
        rc = _lib.load().wkv6bi_backward_ex(B, T, C, H, _ptr(mask), _ptr(lens), _ptr(r), _ptr(k), _ptr(v), _ptr(w),
                                            _ptr(u), _ptr(gy), _ptr(gr), _ptr(gk), _ptr(gv), _ptr(gw), _ptr(gu),
                                            _ptr(ws), ws.numel(), flags, _stream_ptr())
    _lib.check(rc, "wkv6_bi backward_ex")
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
        import ctypes
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
