"""Shared pieces of the operator layer (wkv6_op.py, mix_op.py): one int32-array check, one flag builder, one library call.

The two modules are the only way from Python into librwkv6_amd.so.  What they hold in common lives here, under these invariants:

1. The public surface of wkv6_op, mix_op, wkv, infctx, callers and adapters (names, signatures, defaults, torch.ops schemas, the lifetime
   of `_LIBRARIES`) does not depend on anything in this file.
2. A refused call keeps its exception type and message, and of several faults the same one is reported first: the messages are arguments
   of the helpers, never composed by them.
3. A refusal that comes before `_lib.load()` stays before it: nothing here loads the library except `_call`.
4. An accepted call makes the same library calls in the same order with the same arguments, workspace-size queries included, and
   allocates the same tensors (tests/test_op_calls_gpu.py pins the calls without running a kernel).
5. No host reads: no synchronisation, no .item() / .cpu(), no cu_seqlens on the host.
6. The per-call host cost does not grow: no per-call closures, dict-of-lambda tables or inspection on the way to a launch."""
import torch

from . import _lib

HEAD_SIZE = 64
_AT_LEAST_2 = "1-d with at least 2 elements"           # the shape of a cu_seqlens array for _ints


def _stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ptrs(*tensors):
    return [None if t is None else t.data_ptr() for t in tensors]


def _ints(t, shape, dev, message):
    """The one check of a contiguous int32 array.  shape: a tuple, None (any 1-d length) or _AT_LEAST_2 (cu_seqlens); dev: the device it
    has to be on, or None where the caller judges the device later.  Raises RuntimeError(message); returns t."""
    ok = isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_contiguous()
    if ok and shape is None:
        ok = t.dim() == 1
    elif ok and shape is _AT_LEAST_2:
        ok = t.dim() == 1 and t.numel() >= 2
    elif ok:
        ok = tuple(t.shape) == shape
    if not (ok and (dev is None or t.device == dev)):
        raise RuntimeError(message)
    return t


def _io_of(r):
    if r.dtype not in (torch.bfloat16, torch.float32):
        raise RuntimeError(f"unsupported I/O dtype {r.dtype}")
    return r.dtype


def _flags(io, w_is_ew=False, algo=None):
    """The decay form, the I/O type and the algorithm as the flag word of include/wkv6_amd.h."""
    return ((_lib.W_EW_F32 if w_is_ew else _lib.W_RAW) | (_lib.IO_F32 if io == torch.float32 else 0)
            | (_lib.ALGO_SCAN if algo == "scan" else 0))


def _named(shape, io, r, k, v, w, u, wdt=None, wshape=None, ushape=None, then=None, **same):
    """The `named` dict of wkv6_op._check_tensors (checked, and reported, in this order): r, k, v [shape]; w [wshape or shape] of wdt (or
    io); u [ushape, None: any]; the (tensor, shape, dtype) entries of `then`; every keyword tensor, [shape] as well.  io None: the default
    dtype of the check."""
    named = {"r": (r, shape, io), "k": (k, shape, io), "v": (v, shape, io), "w": (w, wshape or shape, wdt or io), "u": (u, ushape, io)}
    if then:
        named.update(then)
    for name, t in same.items():
        named[name] = (t, shape, io)
    return named


def _s0_entry(s0, n, H, io):
    """(entry of `named`, S0_PER_BATCH or 0) for an initial state [H,N,N] or, one per batch row or sequence, [n,H,N,N]."""
    per_batch = s0.dim() == 4
    return ((s0, (n, H, HEAD_SIZE, HEAD_SIZE) if per_batch else (H, HEAD_SIZE, HEAD_SIZE), io), _lib.S0_PER_BATCH if per_batch else 0)


def _on_device(dev, fn, *args):
    """fn(*args, the current stream of dev) with dev current."""
    with torch.cuda.device(dev):
        return fn(*args, _stream_ptr())


def _call(fn_name, what, dev, *args, tail=(), check=True):
    """The one way into the library: symbol fn_name with (*args, stream, *tail) on the current stream of dev; a nonzero code raises
    "`what` failed: ..." (check=False: the code is returned as it is).  tail: what the rwkv6_forward_varlen_snap_* / _split_* entry points
    take behind their stream."""
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), fn_name)(*args, _stream_ptr(), *tail)
    if check:
        _lib.check(rc, what)
    return rc


def _workspace_or_ckpt(ws, valid, io, algo, alloc, *alloc_args, chunked_only=True):
    """(workspace, CKPT_VALID or 0) of a backward.  ws: the caller's buffer, used as the workspace whatever it holds, or None: alloc(
    *alloc_args) makes one.  valid: the caller says that ws holds the checkpoints its forward wrote; the flag is set for it where the
    chunked kernels run (bf16 and not algo="scan": only they read checkpoints).  chunked_only=False is backward_ex, where a ckpt alone
    sets the flag, fp32 and algo="scan" included.  That difference between the wrappers is as old as they are and is kept."""
    if ws is None:
        return alloc(*alloc_args), 0
    chunked = io == torch.bfloat16 and algo != "scan"
    return ws, _lib.CKPT_VALID if valid and (chunked or not chunked_only) else 0
