"""CPU tier of the snapshot entry points (include/wkv6_amd.h: rwkv6_forward_varlen_snap_bf16 / _fp16 / _fp32): the symbols are exported with
the documented argument list, every documented refusal returns its code before anything is launched -- what the plain call refuses
included -- and the Python wrappers refuse what they can see is wrong before they call the library.

The pointers passed here are dummies (64: aligned, never dereferenced), as in test_rwkv6_varlen_abi_cpu.py."""
import ctypes
import os
import re

import pytest

EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4
P = 64
ALGO_SCAN = 16
NAMES = ("rwkv6_forward_varlen_snap_bf16", "rwkv6_forward_varlen_snap_fp16", "rwkv6_forward_varlen_snap_fp32")
PTRS = ("cu", "state_slot", "state_pool", "r", "k", "v", "w", "u", "y")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


def args(total_T=256, n_seq=3, max_seqlen=128, C=128, H=2, n_slots=8, ws=P, ws_bytes=1 << 40, flags=0, state_slot_out=P, snap_every=64,
         cu_snap=P, snap_slot=P, n_snap=4, **ptrs):
    p = {n: ptrs.get(n, P) for n in PTRS}
    return (total_T, n_seq, max_seqlen, C, H, p["cu"], p["state_slot"], n_slots, p["state_pool"], p["r"], p["k"], p["v"], p["w"], p["u"],
            p["y"], ws, ws_bytes, flags, None, state_slot_out, snap_every, cu_snap, snap_slot, n_snap)


def test_symbols_and_signature(lib):
    """The three symbols exist; header, ctypes table and the plain call agree: the plain argument list, then const int* state_slot_out,
    int snap_every, const int* cu_snap, const int* snap_slot, int n_snap."""
    from rwkv_lm_ext_amd import _lib
    header = open(os.path.join(ROOT, "include", "wkv6_amd.h")).read()
    tail = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    for name in NAMES:
        fn = getattr(lib, name)
        res, argtypes = _lib.SIGNATURES[name]
        plain = _lib.SIGNATURES[name.replace("_snap", "")]
        assert res is ctypes.c_int and list(argtypes) == list(plain[1]) + tail
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(argtypes)
        decl = re.search(r"int " + name + r"\(([^;]*)\);", header).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        assert len(params) == len(argtypes) == 24
        assert params[-5:] == ["const int* state_slot_out", "int snap_every", "const int* cu_snap", "const int* snap_slot", "int n_snap"]
        plain_decl = re.search(r"int " + name.replace("_snap", "") + r"\(([^;]*)\);", header).group(1)
        assert params[:-5] == [" ".join(p.split()) for p in plain_decl.split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_snapshot_refusals(lib, name):
    fn = getattr(lib, name)
    for bad in (-64, -1, 1, 32, 63, 65, 96, 100, 127):
        assert fn(*args(snap_every=bad)) == EINVAL, bad
    for n_snap in (-1, -100):
        assert fn(*args(n_snap=n_snap)) == EINVAL, n_snap
        assert fn(*args(snap_every=0, n_snap=n_snap)) == EINVAL, n_snap
    assert fn(*args(cu_snap=None)) == ENULL
    assert fn(*args(snap_slot=None)) == ENULL
    assert fn(*args(cu_snap=None, snap_slot=None)) == ENULL
    # accepted (probed through the check behind: a NULL tensor gives ENULL, which a refused snapshot argument would not reach ...)
    for ok in (dict(snap_every=0, cu_snap=None, snap_slot=None, n_snap=0), dict(snap_every=0), dict(snap_every=64), dict(snap_every=128),
               dict(snap_every=1 << 20), dict(state_slot_out=None), dict(n_snap=0), dict(state_slot_out=None, state_slot=None)):
        assert fn(*args(y=None, **ok)) == ENULL, ok
    # (... except the snapshot pointers' own ENULL, which comes first: a bad shape behind a good snapshot list is still EINVAL)
    assert fn(*args(C=96)) == EINVAL
    assert fn(*args(snap_every=33, cu_snap=None)) == EINVAL


@pytest.mark.parametrize("name", NAMES)
def test_everything_the_plain_call_refuses(lib, name):
    fn = getattr(lib, name)
    for kw in ({"C": 96}, {"C": 128, "H": 3}, {"n_seq": 0}, {"n_seq": -2}, {"total_T": 0}, {"total_T": -7}, {"max_seqlen": 0},
               {"max_seqlen": -1}, {"H": 0, "C": 0}, {"n_slots": 0}, {"n_slots": -4}):
        assert fn(*args(**kw)) == EINVAL, kw
    assert fn(*args(state_slot=None, n_slots=2)) == EINVAL                  # slot = sequence index: the pool must hold n_seq slots
    assert fn(*args(state_slot=None, n_slots=3, r=None)) == ENULL
    for bit in (1, 2, 4, 8, 32, 64, 128, 256, 1 << 20, 1 << 31):
        assert fn(*args(flags=bit)) == EINVAL, bit
        assert fn(*args(flags=ALGO_SCAN | bit)) == EINVAL, bit
    assert fn(*args(flags=ALGO_SCAN, r=None)) == ENULL
    for p in PTRS:
        if p != "state_slot":
            assert fn(*args(**{p: None})) == ENULL, p
    need = lib.rwkv6_varlen_workspace_bytes(3)
    for short in (0, 1, need - 1):
        assert fn(*args(ws_bytes=short)) == EWORKSPACE, short
    for bad in (65, 66, 72):
        assert fn(*args(ws_bytes=need, y=bad)) == EINVAL, bad


def test_row_addressing_limits_follow_the_route(lib):
    C, H = 4096, 64
    full, half = (1 << 31) // C - 64, (1 << 30) // C - 64
    bf16, fp16, fp32 = (getattr(lib, n) for n in NAMES)
    big = dict(total_T=full, C=C, H=H)
    assert bf16(*args(max_seqlen=half, **big)) == EUNSUPPORTED
    assert bf16(*args(max_seqlen=half - 1, r=None, **big)) == ENULL
    assert bf16(*args(max_seqlen=half, flags=ALGO_SCAN, r=None, **big)) == ENULL
    for fn, fl in ((bf16, ALGO_SCAN), (fp16, 0), (fp32, 0)):
        assert fn(*args(max_seqlen=full, flags=fl, **big)) == EUNSUPPORTED
        assert fn(*args(max_seqlen=full - 1, flags=fl, r=None, **big)) == ENULL


def test_python_wrappers_refuse_before_calling_the_library(monkeypatch):
    import torch
    from rwkv_lm_ext_amd import _lib, wkv6_op

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", no_library)
    bf, i32 = torch.bfloat16, torch.int32
    T, C, H = 8, 128, 2
    ok = dict(state_pool=torch.zeros(4, H, 64, 64), state_slot=torch.zeros(2, dtype=i32), r=torch.zeros(T, C, dtype=bf),
              k=torch.zeros(T, C, dtype=bf), v=torch.zeros(T, C, dtype=bf), w=torch.zeros(T, C), u=torch.zeros(H, 64, dtype=bf),
              y=torch.zeros(T, C, dtype=bf), cu_seqlens=torch.tensor([0, 3, 8], dtype=i32))
    order = ("state_pool", "state_slot", "r", "k", "v", "w", "u", "y", "cu_seqlens")
    good = dict(state_slot_out=torch.zeros(2, dtype=i32), snap_every=64, cu_snap=torch.zeros(3, dtype=i32), snap_slot=torch.zeros(5, dtype=i32))

    def call(**over):
        return wkv6_op.rwkv6.forward_varlen_bf16(T, C, H, *(ok[n] for n in order), 8, **dict(good, **over))

    with pytest.raises(RuntimeError, match="must be on the GPU"):            # everything else is right: no CPU path
        call()
    for bad in (-64, 1, 65, 96, 64.0, "64"):
        with pytest.raises(RuntimeError, match="snap_every must be"):
            call(snap_every=bad)
    for bad in (good["state_slot_out"].long(), torch.zeros(3, dtype=i32), torch.zeros(4, dtype=i32)[::2], [0, 1]):
        with pytest.raises(RuntimeError, match="state_slot_out must be"):
            call(state_slot_out=bad)
    for bad in (None, good["cu_snap"].long(), torch.zeros(2, dtype=i32), torch.zeros(4, dtype=i32)):
        with pytest.raises(RuntimeError, match="cu_snap must be"):
            call(cu_snap=bad)
    for bad in (None, good["snap_slot"].float(), torch.zeros(2, 2, dtype=i32), (1, 2)):
        with pytest.raises(RuntimeError, match="snap_slot must be"):
            call(snap_slot=bad)
    with pytest.raises(RuntimeError, match="belong to snap_every > 0"):
        call(snap_every=0)
    if torch.cuda.is_available():                                           # an int array on another device than the tensors
        dev = {n: t.cuda() for n, t in ok.items()}
        with pytest.raises(RuntimeError, match="state_slot_out must be"):
            wkv6_op.rwkv6.forward_varlen_bf16(T, C, H, *(dev[n] for n in order), 8, **good)
    assert all(hasattr(torch.ops.rwkv6, n) for n in ("forward_varlen_snap_bf16", "forward_varlen_snap_fp16", "forward_varlen_snap_fp32"))
    for fn in (wkv6_op.rwkv6.forward_varlen_snap_bf16, wkv6_op.rwkv6.forward_varlen_snap_fp16, wkv6_op.rwkv6.forward_varlen_snap_fp32):
        assert callable(fn)
