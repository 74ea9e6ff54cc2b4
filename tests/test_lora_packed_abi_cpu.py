"""CPU tier of the per-sequence LoRA operator (include/wkv6_amd.h: wkv6_lora_packed_bf16, wkv6_lora_packed_workspace_bytes): both symbols
are exported with the documented argument lists, every documented refusal returns its code before anything is launched and in the
documented order, the workspace formula holds, and mix_op.lora_packed refuses what it can see is wrong before it calls the library.

The pointers passed here are dummies (multiples of 64 far apart, never dereferenced), as in test_packed_shift_abi_cpu.py."""
import ctypes
import os
import re

import pytest

EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4
X, APOOL, BPOOL, Y, WORK, P = 1 << 40, 2 << 40, 3 << 40, 4 << 40, 5 << 40, 64        # 1 TiB apart: no test shape makes them overlap
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


def args(total_T=100, n_seq=3, K=128, N=192, R=8, n_adapters=5, cu=P, adapter=P, x=X, A=APOOL, B=BPOOL, scale=P, y=Y, work=WORK,
         work_bytes=1 << 40):
    return (total_T, n_seq, K, N, R, n_adapters, cu, adapter, x, A, B, scale, y, work, work_bytes, None)


def test_symbols_and_signatures(lib):
    from rwkv_lm_ext_amd import _lib
    header = open(os.path.join(ROOT, "include", "wkv6_amd.h")).read()
    I, L, VP, SZ = ctypes.c_int, ctypes.c_long, ctypes.c_void_p, ctypes.c_size_t
    want = {"wkv6_lora_packed_workspace_bytes": (SZ, "size_t", [L, I], ["long total_T", "int R"]),
            "wkv6_lora_packed_bf16": (I, "int", [L, I, I, I, I, I, VP, VP, VP, VP, VP, VP, VP, VP, SZ, VP],
                                      ["long total_T", "int n_seq", "int K", "int N", "int R", "int n_adapters", "const int* cu_seqlens",
                                       "const int* adapter", "const void* x", "const void* A_pool", "const void* B_pool",
                                       "const float* scale", "void* y", "void* workspace", "size_t workspace_bytes", "void* stream"])}
    for name, (restype, cres, argtypes, params) in want.items():
        fn = getattr(lib, name)
        res, table = _lib.SIGNATURES[name]
        assert res is restype and list(table) == argtypes
        assert fn.restype is restype and list(fn.argtypes) == argtypes
        decl = re.search(cres + " " + name + r"\(([^;]*)\);", header).group(1)
        assert [" ".join(p.split()) for p in decl.split(",")] == params


def test_workspace_formula(lib):
    fn = lib.wkv6_lora_packed_workspace_bytes
    for total_T in (1, 15, 16, 17, 129, 4096, 100003, (1 << 31) - 1):
        for R in (8, 16, 32, 64):
            assert fn(total_T, R) == (total_T * R * 2 + 255) // 256 * 256, (total_T, R)
    for total_T, R in ((0, 8), (-1, 8), (1 << 31, 8), (16, 0), (16, 4), (16, 12), (16, 24), (16, 128), (16, -8)):
        assert fn(total_T, R) == 0, (total_T, R)


def test_refusals_and_their_order(lib):
    fn = lib.wkv6_lora_packed_bf16
    # (1) sizes
    for kw in ({"total_T": 0}, {"total_T": -3}, {"n_seq": 0}, {"n_seq": -1}, {"n_adapters": 0}, {"n_adapters": -2}, {"R": 0}, {"R": -8},
               {"K": 0}, {"K": 32}, {"K": 96}, {"K": 16384 + 64}, {"N": 0}, {"N": 32}, {"N": 160}, {"N": 16384 + 64}):
        assert fn(*args(**kw)) == EINVAL, kw
        assert fn(*args(**dict(kw, x=None))) == EINVAL, kw                  # ... in front of the NULL check
    assert fn(*args(K=96, R=12)) == EINVAL                                  # ... and of the rank
    assert fn(*args(N=32, total_T=1 << 31)) == EINVAL
    # (2) what the kernels do not have
    for R in (1, 4, 12, 24, 48, 128):
        assert fn(*args(R=R)) == EUNSUPPORTED, R
        assert fn(*args(R=R, y=None)) == EUNSUPPORTED, R                    # in front of the NULL check
    assert fn(*args(total_T=1 << 31)) == EUNSUPPORTED
    assert fn(*args(total_T=1 << 31, cu=None)) == EUNSUPPORTED
    assert fn(*args(total_T=(1 << 31) - 1, K=64, N=64, x=None)) == ENULL    # INT_MAX itself goes on to the next check
    # (3) NULL pointers, the workspace included; in front of alignment, overlap and the workspace size
    for p in ("cu", "adapter", "x", "A", "B", "scale", "y", "work"):
        assert fn(*args(**{p: None})) == ENULL, p
        assert fn(*args(**dict({p: None}, work_bytes=0))) == ENULL, p
    assert fn(*args(x=None, y=Y + 2)) == ENULL
    assert fn(*args(A=None, y=X)) == ENULL
    # (4) alignment: 16 bytes for the bf16 tensors and the workspace, 4 for the int arrays and scale
    for p, base in (("x", X), ("A", APOOL), ("B", BPOOL), ("y", Y), ("work", WORK)):
        for off in (1, 2, 4, 8, 12):
            assert fn(*args(**{p: base + off})) == EINVAL, (p, off)
            assert fn(*args(**dict({p: base + off}, work_bytes=0))) == EINVAL, (p, off)     # in front of the workspace size
    for p in ("cu", "adapter", "scale"):
        for off in (1, 2, 3):
            assert fn(*args(**{p: P + off})) == EINVAL, (p, off)
        assert fn(*args(**dict({p: P + 4}, work_bytes=0))) == EWORKSPACE, p                # 4-byte aligned: accepted so far
    # (4) y [total_T,N] against x [total_T,K], A_pool [n_adapters,R,K], B_pool [n_adapters,N,R] (2 bytes an element): touching at either
    # end is an overlap, adjacent is not (probed through the check that comes next)
    T, K, N, R, n = 100, 128, 192, 8, 5
    for base, size in ((X, T * K * 2), (APOOL, n * R * K * 2), (BPOOL, n * N * R * 2)):
        for y in (base, base - T * N * 2 + 16, base + size - 16):
            assert fn(*args(y=y)) == EINVAL, (base, y)
            assert fn(*args(y=y, work_bytes=0)) == EINVAL, (base, y)
        for y in (base - T * N * 2, base + size):
            assert fn(*args(y=y, work_bytes=0)) == EWORKSPACE, (base, y)
    # (5) the workspace size, last
    for total_T, R in ((100, 8), (100, 64), (4097, 16), (1, 32)):
        need = lib.wkv6_lora_packed_workspace_bytes(total_T, R)
        assert need == (total_T * R * 2 + 255) // 256 * 256
        for short in (0, 1, need - 1):
            assert fn(*args(total_T=total_T, R=R, work_bytes=short)) == EWORKSPACE, (total_T, R, short)


def test_lora_packed_refuses_before_calling_the_library(monkeypatch):
    import torch
    from rwkv_lm_ext_amd import _lib, mix_op

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", no_library)
    bf, i32 = torch.bfloat16, torch.int32
    T, K, N, R, n = 10, 128, 64, 8, 3
    good = dict(x=torch.zeros(1, T, K, dtype=bf), y=torch.zeros(1, T, N, dtype=bf), A=torch.zeros(n, R, K, dtype=bf),
                B=torch.zeros(n, N, R, dtype=bf), scale=torch.ones(n), adapter=torch.zeros(2, dtype=i32), cu=torch.tensor([0, 4, T], dtype=i32))

    def call(**o):
        a = dict(good, **o)
        return mix_op.lora_packed(a["x"], a["y"], a["A"], a["B"], a["scale"], a["adapter"], a["cu"])

    with pytest.raises(RuntimeError, match="must be on the GPU"):            # everything else is right: no CPU path
        call()
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        call(x=good["x"][0], y=good["y"][0])
    for bad in (good["x"].float(), good["x"].half(), torch.zeros(2, T, K, dtype=bf), torch.zeros(T * K, dtype=bf),
                torch.zeros(1, T, 2 * K, dtype=bf)[..., :K], None):
        with pytest.raises(RuntimeError, match="x must be"):
            call(x=bad)
    for bad in (good["y"].float(), torch.zeros(T, N, dtype=bf), torch.zeros(1, T + 1, N, dtype=bf), torch.zeros(1, T, 2 * N, dtype=bf)[..., :N],
                None):
        with pytest.raises(RuntimeError, match="y must be"):
            call(y=bad)
    for bad in (good["A"].float(), torch.zeros(n, R, K + 64, dtype=bf), torch.zeros(R, K, dtype=bf), torch.zeros(n, 2 * R, K, dtype=bf)[:, ::2],
                None):
        with pytest.raises(RuntimeError, match="A_pool must be"):
            call(A=bad)
    for bad in (good["B"].float(), torch.zeros(n, R, N, dtype=bf), torch.zeros(n + 1, N, R, dtype=bf), torch.zeros(n, N, 16, dtype=bf), None):
        with pytest.raises(RuntimeError, match="B_pool must be"):
            call(B=bad)
    for bad in (good["scale"].to(bf), good["scale"].double(), torch.ones(n + 1), torch.ones(2 * n)[::2], 4.0):
        with pytest.raises(RuntimeError, match="scale must be"):
            call(scale=bad)
    for r in (4, 12, 128):
        with pytest.raises(RuntimeError, match="R must be one of"):
            call(A=torch.zeros(n, r, K, dtype=bf), B=torch.zeros(n, N, r, dtype=bf))
    with pytest.raises(RuntimeError, match="multiples of 64"):
        call(x=torch.zeros(1, T, 96, dtype=bf), A=torch.zeros(n, R, 96, dtype=bf))
    with pytest.raises(RuntimeError, match="multiples of 64"):
        call(y=torch.zeros(1, T, 32, dtype=bf), B=torch.zeros(n, 32, R, dtype=bf))
    for bad in (good["cu"].long(), torch.zeros(1, dtype=i32), torch.zeros(6, dtype=i32)[::2], [0, 4, T], None):
        with pytest.raises(RuntimeError, match="cu_seqlens must be"):
            call(cu=bad)
    for bad in (good["adapter"].long(), torch.zeros(3, dtype=i32), torch.zeros(4, dtype=i32)[::2], [0, 1], None):
        with pytest.raises(RuntimeError, match="adapter must be"):
            call(adapter=bad)
    for t in ("x", "A", "B"):
        with pytest.raises(RuntimeError, match="has no backward"):
            call(**{t: good[t].clone().requires_grad_()})
    with torch.no_grad(), pytest.raises(RuntimeError, match="must be on the GPU"):      # ... which no_grad lifts
        call(x=good["x"].clone().requires_grad_())
