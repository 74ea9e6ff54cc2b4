"""CPU tier of the split entry point (include/wkv6_amd.h: rwkv6_forward_varlen_split_bf16, rwkv6_varlen_split_workspace_bytes): the symbols
are exported with the documented argument lists, every documented refusal returns its code before anything is launched -- what the snap call
refuses included, with the same codes -- the workspace bound behaves as documented, and the Python wrappers refuse what they can see is wrong
before they call the library.

The pointers passed here are dummies (64: aligned, never dereferenced), as in test_rwkv6_snap_abi_cpu.py."""
import ctypes
import os
import re

import pytest

EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4
P = 64
ALGO_SCAN = 16
NAME = "rwkv6_forward_varlen_split_bf16"
PTRS = ("cu", "state_slot", "state_pool", "r", "k", "v", "w", "u", "y")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


def args(total_T=256, n_seq=3, max_seqlen=128, C=128, H=2, n_slots=8, ws=P, ws_bytes=1 << 40, flags=0, state_slot_out=P, snap_every=64,
         cu_snap=P, snap_slot=P, n_snap=4, seg_len=64, **ptrs):
    p = {n: ptrs.get(n, P) for n in PTRS}
    return (total_T, n_seq, max_seqlen, C, H, p["cu"], p["state_slot"], n_slots, p["state_pool"], p["r"], p["k"], p["v"], p["w"], p["u"],
            p["y"], ws, ws_bytes, flags, None, state_slot_out, snap_every, cu_snap, snap_slot, n_snap, seg_len)


def test_symbols_and_signatures(lib):
    """Header, ctypes table and the snap call agree: the snap argument list, then int seg_len; the workspace bound takes
    (long total_T, int n_seq, int seg_len, int C, int H) and returns a size_t."""
    from rwkv_lm_ext_amd import _lib
    header = open(os.path.join(ROOT, "include", "wkv6_amd.h")).read()
    fn = getattr(lib, NAME)
    res, argtypes = _lib.SIGNATURES[NAME]
    snap = _lib.SIGNATURES["rwkv6_forward_varlen_snap_bf16"]
    assert res is ctypes.c_int and list(argtypes) == list(snap[1]) + [ctypes.c_int]
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(argtypes)
    decl = re.search(r"int " + NAME + r"\(([^;]*)\);", header).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert len(params) == len(argtypes) == 25
    assert params[-1] == "int seg_len"
    snap_decl = re.search(r"int rwkv6_forward_varlen_snap_bf16\(([^;]*)\);", header).group(1)
    assert params[:-1] == [" ".join(p.split()) for p in snap_decl.split(",")]
    ws = lib.rwkv6_varlen_split_workspace_bytes
    res, argtypes = _lib.SIGNATURES["rwkv6_varlen_split_workspace_bytes"]
    assert res is ctypes.c_size_t and list(argtypes) == [ctypes.c_long] + [ctypes.c_int] * 4
    assert ws.restype is ctypes.c_size_t and list(ws.argtypes) == list(argtypes)
    assert re.search(r"size_t rwkv6_varlen_split_workspace_bytes\(long total_T, int n_seq, int seg_len, int C, int H\);", header)
    # no fp16 / fp32 split entry point: those I/O types stay on the exact scan
    for io in ("fp16", "fp32"):
        assert not hasattr(lib, "rwkv6_forward_varlen_split_" + io)
        assert "rwkv6_forward_varlen_split_" + io not in header


def test_seg_len_refusals(lib):
    fn = getattr(lib, NAME)
    for bad in (-64, 1, 32, 100, -1, 63, 65, 96):
        assert fn(*args(seg_len=bad)) == EINVAL, bad
        assert fn(*args(seg_len=bad, flags=ALGO_SCAN)) == EINVAL, bad
    assert fn(*args(seg_len=64, flags=ALGO_SCAN)) == EUNSUPPORTED
    assert fn(*args(seg_len=1 << 20, flags=ALGO_SCAN)) == EUNSUPPORTED
    # accepted (probed through the check behind: a NULL tensor gives ENULL, which a refused seg_len would not reach)
    for ok in (0, 64, 128, 192, 512, 1 << 20):
        assert fn(*args(seg_len=ok, y=None)) == ENULL, ok
    assert fn(*args(seg_len=0, flags=ALGO_SCAN, y=None)) == ENULL          # the snap call's scan route
    # a bad argument behind a good seg_len keeps its own code, ALGO_SCAN or not
    assert fn(*args(C=96)) == EINVAL
    assert fn(*args(C=96, flags=ALGO_SCAN)) == EINVAL
    assert fn(*args(flags=ALGO_SCAN, r=None)) == ENULL


@pytest.mark.parametrize("seg_len", [0, 64, 128])
def test_everything_the_snap_call_refuses(lib, seg_len):
    fn, snap = getattr(lib, NAME), lib.rwkv6_forward_varlen_snap_bf16

    def both(expect, **kw):
        a = args(seg_len=seg_len, **kw)
        assert snap(*a[:-1]) == expect, kw
        assert fn(*a) == expect, kw

    for kw in ({"C": 96}, {"C": 128, "H": 3}, {"n_seq": 0}, {"n_seq": -2}, {"total_T": 0}, {"total_T": -7}, {"max_seqlen": 0},
               {"max_seqlen": -1}, {"H": 0, "C": 0}, {"n_slots": 0}, {"n_slots": -4}):
        both(EINVAL, **kw)
    both(EINVAL, state_slot=None, n_slots=2)
    both(ENULL, state_slot=None, n_slots=3, r=None)
    for bit in (1, 2, 4, 8, 32, 64, 128, 256, 1 << 20, 1 << 31):
        both(EINVAL, flags=bit)
        both(EINVAL, flags=ALGO_SCAN | bit)
    for p in PTRS:
        if p != "state_slot":
            both(ENULL, **{p: None})
    for bad in (-64, -1, 1, 32, 63, 65, 96, 100, 127):
        both(EINVAL, snap_every=bad)
    for n_snap in (-1, -100):
        both(EINVAL, n_snap=n_snap)
        both(EINVAL, snap_every=0, n_snap=n_snap)
    both(ENULL, cu_snap=None)
    both(ENULL, snap_slot=None)
    for bad in (65, 66, 72):
        both(EINVAL, y=bad)
    C, H = 4096, 64
    full, half = (1 << 31) // C - 64, (1 << 30) // C - 64
    both(EUNSUPPORTED, total_T=full, C=C, H=H, max_seqlen=half)
    both(ENULL, total_T=full, C=C, H=H, max_seqlen=half - 1, r=None)


def test_workspace_bound(lib):
    fn, need = getattr(lib, NAME), lib.rwkv6_varlen_split_workspace_bytes
    plain = lib.rwkv6_varlen_workspace_bytes
    for n_seq in (0, -1, -100):
        for seg_len in (0, 64, 512):
            assert need(256, n_seq, seg_len, 128, 2) == 0
    for seg_len in (64, 128, 512, 2048):
        last = 0
        for total_T in (1, 63, 64, 65, 256, 1000, 4096, 16384, 1 << 20):
            n = need(total_T, 3, seg_len, 128, 2)
            assert n >= last and n >= plain(3) > 0, (seg_len, total_T)
            last = n
        assert need(1 << 20, 3, seg_len, 128, 2) > need(64, 3, seg_len, 128, 2)
        for n_seq in (1, 3, 300):
            assert need(4096, n_seq, seg_len, 128, 2) >= plain(n_seq)
    for n_seq in (1, 3, 300):
        assert need(4096, n_seq, 0, 128, 2) == plain(n_seq)
    # per item and head: A (items with a successor), the entry state, 16 KB each, and the decay sums, 1 KB
    n_table, extra, H = 3 + 256 // 64, 256 // 64, 2
    assert need(256, 3, 64, 128, H) >= plain(3) + (n_table + extra) * H * 16384 + extra * H * 1024
    # a workspace one byte short is refused, the exact size passes that check (and fails the next one: ENULL)
    for seg_len in (64, 128):
        n = need(256, 3, seg_len, 128, 2)
        for short in (0, 1, plain(3), n - 1):
            assert fn(*args(seg_len=seg_len, ws_bytes=short)) == EWORKSPACE, (seg_len, short)
        assert fn(*args(seg_len=seg_len, ws_bytes=n, y=65)) == EINVAL
    # nothing to cut below the chunked route's 32 tokens: the plain workspace is enough
    assert fn(*args(seg_len=64, max_seqlen=16, ws_bytes=plain(3), y=65)) == EINVAL
    n0 = plain(3)
    for short in (0, 1, n0 - 1):
        assert fn(*args(seg_len=0, ws_bytes=short)) == EWORKSPACE


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

    def call(**over):
        return wkv6_op.rwkv6.forward_varlen_bf16(T, C, H, *(ok[n] for n in order), 8, **over)

    with pytest.raises(RuntimeError, match="must be on the GPU"):            # everything else is right: no CPU path
        call(seg_len=64)
    for bad in (-64, 1, 32, 100, 64.0, "64", True):
        with pytest.raises(RuntimeError, match="seg_len must be"):
            call(seg_len=bad)
    with pytest.raises(RuntimeError, match="not with algo='scan'"):
        call(seg_len=64, algo="scan")
    with pytest.raises(RuntimeError, match="must be on the GPU"):            # seg_len = 0 with the scan stays legal
        call(seg_len=0, algo="scan")
    # the split op proper: same checks, seg_len = 0 included
    def split(seg_len, **over):
        a = dict(ok, **over)
        return wkv6_op.rwkv6.forward_varlen_split_bf16(T, C, H, a["state_pool"], a["state_slot"], None, a["r"], a["k"], a["v"], a["w"], a["u"],
                                                       a["y"], a["cu_seqlens"], 8, 0, None, None, seg_len)
    for bad in (-64, 1, 32, 100):
        with pytest.raises(RuntimeError, match="seg_len must be"):
            split(bad)
    for good in (0, 64):
        with pytest.raises(RuntimeError, match="must be on the GPU"):
            split(good)
    with pytest.raises(RuntimeError, match="must be torch.bfloat16"):
        split(64, r=ok["r"].half())
    # no other I/O type takes a seg_len
    for name in ("forward_varlen_fp16", "forward_varlen_fp32"):
        with pytest.raises(TypeError):
            getattr(wkv6_op.rwkv6, name)(T, C, H, *(ok[n] for n in order), 8, seg_len=64)
    assert hasattr(torch.ops.rwkv6, "forward_varlen_split_bf16")
    assert callable(wkv6_op.new_rwkv6_varlen_split_workspace)
    import inspect
    from rwkv_lm_ext_amd import infctx, wkv
    assert inspect.signature(wkv.RUN_RWKV_6_VARLEN).parameters["seg_len"].default == 0
    assert inspect.signature(infctx.tmix_forward_packed).parameters["seg_len"].default == 0
