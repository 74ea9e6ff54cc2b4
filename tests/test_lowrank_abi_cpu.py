"""CPU tier of the low-rank time-mix calls (include/wkv6_amd.h: wkv6_tmix_lerp_lowrank_bf16, wkv6_decay_lowrank_bf16,
wkv6_lowrank_workspace_bytes): the symbols are exported with the documented argument lists, every documented refusal returns its code
before anything is launched and in the documented order, the workspace formula holds, and mix_op.tmix_inputs / mix_op.decay_lowrank refuse
what they can see is wrong before they call the library.

The pointers passed here are dummies (multiples of 64 far apart, never dereferenced), as in test_lora_packed_abi_cpu.py."""
import ctypes
import os
import re

import pytest

EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4
X, FRONT, MAAX, W1, W2, MAA5, OUT, WORK, P = (i << 40 for i in range(1, 10))       # 1 TiB apart: no test shape makes them overlap
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


def targs(total_T=100, n_seq=3, C=128, D=32, cu=P, x=X, front=FRONT, n_slots=4, slot=P + 64, maa_x=MAAX, W1t=W1, W2t=W2, maa5=MAA5, out=OUT,
          work=WORK, work_bytes=1 << 40):
    return (total_T, n_seq, C, D, cu, x, front, n_slots, slot, maa_x, W1t, W2t, maa5, out, work, work_bytes, None)


def dargs(rows=100, C=128, Dd=64, N=192, xw=X, D1t=W1, D2t=W2, time_decay=MAA5, w=OUT, work=WORK, work_bytes=1 << 40):
    return (rows, C, Dd, N, xw, D1t, D2t, time_decay, w, work, work_bytes, None)


def test_symbols_and_signatures(lib):
    from rwkv_lm_ext_amd import _lib
    header = open(os.path.join(ROOT, "include", "wkv6_amd.h")).read()
    I, L, VP, SZ = ctypes.c_int, ctypes.c_long, ctypes.c_void_p, ctypes.c_size_t
    want = {"wkv6_lowrank_workspace_bytes": (SZ, "size_t", [L, I], ["long rows", "int D_total"]),
            "wkv6_tmix_lerp_lowrank_bf16": (I, "int", [L, I, I, I, VP, VP, VP, I, VP, VP, VP, VP, VP, VP, VP, SZ, VP],
                                            ["long total_T", "int n_seq", "int C", "int D", "const int* cu_seqlens", "const void* x",
                                             "const void* front", "int n_slots", "const int* slot", "const void* maa_x", "const void* W1t",
                                             "const void* W2t", "const void* maa5", "void* out", "void* workspace", "size_t workspace_bytes",
                                             "void* stream"]),
            "wkv6_decay_lowrank_bf16": (I, "int", [L, I, I, I, VP, VP, VP, VP, VP, VP, SZ, VP],
                                        ["long rows", "int C", "int Dd", "int N", "const void* xw", "const void* D1t", "const void* D2t",
                                         "const void* time_decay", "void* w", "void* workspace", "size_t workspace_bytes", "void* stream"])}
    for name, (restype, cres, argtypes, params) in want.items():
        fn = getattr(lib, name)
        res, table = _lib.SIGNATURES[name]
        assert res is restype and list(table) == argtypes
        assert fn.restype is restype and list(fn.argtypes) == argtypes
        decl = re.search(cres + " " + name + r"\(([^;]*)\);", header).group(1)
        assert [" ".join(p.split()) for p in decl.split(",")] == params


def test_workspace_formula(lib):
    fn = lib.wkv6_lowrank_workspace_bytes
    for rows in (1, 15, 16, 17, 129, 4096, 100003, (1 << 31) - 1):
        for D_total in (160, 320, 64, 128):
            assert fn(rows, D_total) == (rows * D_total * 2 + 255) // 256 * 256, (rows, D_total)
    assert fn(1, 64) == 256 and fn(256, 160) == 81920 and fn(33, 320) == 21248
    for rows, D_total in ((0, 64), (-1, 160), (1 << 31, 64), (16, 0), (16, 32), (16, 80), (16, 96), (16, 256), (16, 640), (16, -64)):
        assert fn(rows, D_total) == 0, (rows, D_total)


def test_tmix_refusals_and_their_order(lib):
    fn = lib.wkv6_tmix_lerp_lowrank_bf16
    assert fn(*targs(work_bytes=0)) == EWORKSPACE                             # the arguments are right up to the last check
    # (1) sizes
    for kw in ({"total_T": 0}, {"total_T": -3}, {"n_seq": 0}, {"n_seq": -1}, {"D": 0}, {"D": -32}, {"C": 0}, {"C": 32}, {"C": 96},
               {"C": 4096 + 64}, {"cu": None, "total_T": 100, "n_seq": 3}, {"n_slots": 0}, {"n_slots": -1}, {"slot": None, "n_slots": 2}):
        assert fn(*targs(**kw)) == EINVAL, kw
        assert fn(*targs(**dict(kw, x=None))) == EINVAL, kw                    # ... in front of the NULL check
        if "D" not in kw:
            assert fn(*targs(**dict(kw, D=48))) == EINVAL, kw                  # ... and of the widths the kernels have
    assert fn(*targs(cu=None, total_T=99, work_bytes=0)) == EWORKSPACE          # dense: 3 sequences of 33 rows
    assert fn(*targs(slot=None, n_slots=3, work_bytes=0)) == EWORKSPACE
    assert fn(*targs(front=None, n_slots=0, slot=None, work_bytes=0)) == EWORKSPACE      # no front: n_slots does not count
    assert fn(*targs(front=None, n_slots=-7, work_bytes=0)) == EWORKSPACE
    # (2) what the kernels do not have
    for D in (1, 8, 16, 48, 128):
        assert fn(*targs(D=D)) == EUNSUPPORTED, D
        assert fn(*targs(D=D, out=None)) == EUNSUPPORTED, D                    # in front of the NULL check
    assert fn(*targs(total_T=1 << 31)) == EUNSUPPORTED
    assert fn(*targs(total_T=1 << 31, x=None)) == EUNSUPPORTED
    assert fn(*targs(total_T=(1 << 31) - 1, C=64, x=None)) == ENULL            # INT_MAX itself goes on to the next check
    # (3) NULL pointers, the workspace included; in front of alignment, overlap and the workspace size.  cu_seqlens, front and slot may be NULL
    for p in ("x", "maa_x", "W1t", "W2t", "maa5", "out", "work"):
        assert fn(*targs(**{p: None})) == ENULL, p
        assert fn(*targs(**dict({p: None}, work_bytes=0))) == ENULL, p
    assert fn(*targs(x=None, out=OUT + 2)) == ENULL
    assert fn(*targs(W1t=None, out=X)) == ENULL
    # (4) alignment: 16 bytes for the bf16 tensors and the workspace, 4 for the int arrays
    for p, base in (("x", X), ("front", FRONT), ("maa_x", MAAX), ("W1t", W1), ("W2t", W2), ("maa5", MAA5), ("out", OUT), ("work", WORK)):
        for off in (1, 2, 4, 8, 12):
            assert fn(*targs(**{p: base + off})) == EINVAL, (p, off)
            assert fn(*targs(**dict({p: base + off}, work_bytes=0))) == EINVAL, (p, off)         # in front of the workspace size
    for p in ("cu", "slot"):
        for off in (1, 2, 3):
            assert fn(*targs(**{p: P + off})) == EINVAL, (p, off)
        assert fn(*targs(**dict({p: P + 4}, work_bytes=0))) == EWORKSPACE, p                    # 4-byte aligned: accepted so far
    # (4) out [5,total_T,C] against every input and the workspace: touching at either end is an overlap, adjacent is not
    T, C, D, n_slots = 100, 128, 32, 4
    ob = 5 * T * C * 2
    need = lib.wkv6_lowrank_workspace_bytes(T, 5 * D)
    for base, size in ((X, T * C * 2), (FRONT, n_slots * C * 2), (MAAX, C * 2), (W1, 5 * D * C * 2), (W2, 5 * C * D * 2), (MAA5, 5 * C * 2),
                       (WORK, need)):
        for out in (base, base - ob + 16, base + size - 16):
            assert fn(*targs(out=out)) == EINVAL, (base, out)
            assert fn(*targs(out=out, work_bytes=0)) == EINVAL, (base, out)
        for out in (base - ob, base + size):
            assert fn(*targs(out=out, work_bytes=0)) == EWORKSPACE, (base, out)
    # (5) the workspace size, last
    for total_T, D in ((100, 32), (100, 64), (4097, 32), (1, 64)):
        need = lib.wkv6_lowrank_workspace_bytes(total_T, 5 * D)
        assert need == (total_T * 5 * D * 2 + 255) // 256 * 256
        for short in (0, 1, need - 1):
            assert fn(*targs(total_T=total_T, n_seq=1, D=D, work_bytes=short)) == EWORKSPACE, (total_T, D, short)


def test_decay_refusals_and_their_order(lib):
    fn = lib.wkv6_decay_lowrank_bf16
    assert fn(*dargs(work_bytes=0)) == EWORKSPACE
    for kw in ({"rows": 0}, {"rows": -3}, {"Dd": 0}, {"Dd": -64}, {"C": 0}, {"C": 32}, {"C": 96}, {"C": 4096 + 64}, {"N": 0}, {"N": 32},
               {"N": 160}, {"N": 4096 + 64}):
        assert fn(*dargs(**kw)) == EINVAL, kw
        assert fn(*dargs(**dict(kw, xw=None))) == EINVAL, kw
        if "Dd" not in kw:
            assert fn(*dargs(**dict(kw, Dd=32))) == EINVAL, kw
    for Dd in (1, 16, 32, 96, 256):
        assert fn(*dargs(Dd=Dd)) == EUNSUPPORTED, Dd
        assert fn(*dargs(Dd=Dd, w=None)) == EUNSUPPORTED, Dd
    assert fn(*dargs(rows=1 << 31)) == EUNSUPPORTED
    assert fn(*dargs(rows=1 << 31, xw=None)) == EUNSUPPORTED
    assert fn(*dargs(rows=(1 << 31) - 1, C=64, N=64, xw=None)) == ENULL
    for p in ("xw", "D1t", "D2t", "time_decay", "w", "work"):
        assert fn(*dargs(**{p: None})) == ENULL, p
        assert fn(*dargs(**dict({p: None}, work_bytes=0))) == ENULL, p
    assert fn(*dargs(xw=None, w=OUT + 2)) == ENULL
    for p, base in (("xw", X), ("D1t", W1), ("D2t", W2), ("time_decay", MAA5), ("w", OUT), ("work", WORK)):
        for off in (1, 2, 4, 8, 12):
            assert fn(*dargs(**{p: base + off})) == EINVAL, (p, off)
            assert fn(*dargs(**dict({p: base + off}, work_bytes=0))) == EINVAL, (p, off)
    rows, C, Dd, N = 100, 128, 64, 192
    wb = rows * N * 2
    need = lib.wkv6_lowrank_workspace_bytes(rows, Dd)
    for base, size in ((X, rows * C * 2), (W1, Dd * C * 2), (W2, N * Dd * 2), (MAA5, N * 2), (WORK, need)):
        for w in (base, base - wb + 16, base + size - 16):
            assert fn(*dargs(w=w)) == EINVAL, (base, w)
            assert fn(*dargs(w=w, work_bytes=0)) == EINVAL, (base, w)
        for w in (base - wb, base + size):
            assert fn(*dargs(w=w, work_bytes=0)) == EWORKSPACE, (base, w)
    for rows, Dd in ((100, 64), (100, 128), (4097, 64), (1, 128)):
        need = lib.wkv6_lowrank_workspace_bytes(rows, Dd)
        for short in (0, 1, need - 1):
            assert fn(*dargs(rows=rows, Dd=Dd, work_bytes=short)) == EWORKSPACE, (rows, Dd, short)


def test_the_python_ops_refuse_before_calling_the_library(monkeypatch):
    import torch
    from rwkv_lm_ext_amd import _lib, mix_op

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", no_library)
    bf, i32 = torch.bfloat16, torch.int32
    T, C, D, Dd, n = 10, 128, 32, 64, 2
    z = lambda *s: torch.zeros(*s, dtype=bf)
    good = dict(x=z(1, T, C), maa_x=z(C), W1t=z(5 * D, C), W2t=z(5, C, D), maa5=z(5, C), cu=torch.tensor([0, 4, T], dtype=i32), shifted0=None,
                pool=None, slots=None)

    def call(**o):
        a = dict(good, **o)
        return mix_op.tmix_inputs(a["x"], a["maa_x"], a["W1t"], a["W2t"], a["maa5"], a["cu"], a["shifted0"], a["pool"], a["slots"])

    with pytest.raises(RuntimeError, match="must be on the GPU"):            # everything else is right: no CPU path
        call()
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        call(x=z(2, 5, C), cu=None, shifted0=z(2, C))
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        call(pool=z(4, C), slots=torch.zeros(n, dtype=i32))
    for bad in (good["x"].float(), z(T * C), z(1, T, 2 * C)[..., :C], None):
        with pytest.raises(RuntimeError, match="x must be"):
            call(x=bad)
    with pytest.raises(RuntimeError, match="x must be"):
        call(x=z(T, C), cu=None)                                             # dense is [B, T, C]
    with pytest.raises(RuntimeError, match="a packed batch is"):
        call(x=z(2, T, C))
    for bad in (good["maa_x"].float(), z(C + 64), z(2 * C)[::2], None):
        with pytest.raises(RuntimeError, match="maa_x must be"):
            call(maa_x=bad)
    for bad in (good["W1t"].float(), z(5 * D, C + 64), z(C, 5 * D), z(5 * D + 1, C), z(C, 5 * D).t(), None):
        with pytest.raises(RuntimeError, match="W1t must be"):
            call(W1t=bad)
    for bad in (good["W2t"].float(), z(5, D, C), z(5, C, 2 * D), z(5, D, C).transpose(1, 2), None):
        with pytest.raises(RuntimeError, match="W2t must be"):
            call(W2t=bad)
    for bad in (good["maa5"].float(), z(5, C + 64), z(4, C), None):
        with pytest.raises(RuntimeError, match="maa5 must be"):
            call(maa5=bad)
    for d in (16, 48, 128):
        with pytest.raises(RuntimeError, match="D must be one of"):
            call(W1t=z(5 * d, C), W2t=z(5, C, d))
    with pytest.raises(RuntimeError, match="multiple of 64"):
        call(x=z(1, T, 96), maa_x=z(96), W1t=z(5 * D, 96), W2t=z(5, 96, D), maa5=z(5, 96))
    for bad in (good["cu"].long(), torch.zeros(1, dtype=i32), torch.zeros(6, dtype=i32)[::2], [0, 4, T]):
        with pytest.raises(RuntimeError, match="cu_seqlens must be"):
            call(cu=bad)
    with pytest.raises(RuntimeError, match="exclude each other"):
        call(shifted0=z(n, C), pool=z(4, C))
    with pytest.raises(RuntimeError, match="belong to a packed batch"):
        call(x=z(2, 5, C), cu=None, pool=z(4, C))
    with pytest.raises(RuntimeError, match="slots name rows"):
        call(slots=torch.zeros(n, dtype=i32))
    for bad in (z(n, C).float(), z(n + 1, C), z(n, 2 * C)[:, :C]):
        with pytest.raises(RuntimeError, match="shifted0 must be"):
            call(shifted0=bad)
    for bad in (z(4, C).float(), z(4, C + 64), z(4 * C), z(4, 2 * C)[:, :C]):
        with pytest.raises(RuntimeError, match="shift_pool must be"):
            call(pool=bad)
    with pytest.raises(RuntimeError, match="the pool must hold n_seq slots"):
        call(pool=z(1, C))
    for bad in (torch.zeros(n, dtype=torch.int64), torch.zeros(n + 1, dtype=i32), [0, 1]):
        with pytest.raises(RuntimeError, match="slots must be"):
            call(pool=z(4, C), slots=bad)
    for t in ("x", "maa_x", "W1t", "W2t", "maa5"):
        with pytest.raises(RuntimeError, match="has no backward"):
            call(**{t: good[t].clone().requires_grad_()})
    with pytest.raises(RuntimeError, match="has no backward"):
        call(pool=z(4, C).requires_grad_())
    with torch.no_grad(), pytest.raises(RuntimeError, match="must be on the GPU"):      # ... which no_grad lifts
        call(x=good["x"].clone().requires_grad_())

    dgood = dict(xw=z(1, T, C), D1t=z(Dd, C), D2t=z(192, Dd), td=z(1, 1, 192))

    def dcall(**o):
        a = dict(dgood, **o)
        return mix_op.decay_lowrank(a["xw"], a["D1t"], a["D2t"], a["td"])

    with pytest.raises(RuntimeError, match="must be on the GPU"):
        dcall()
    for bad in (dgood["xw"].float(), z(C), z(T, 2 * C)[:, :C], None):
        with pytest.raises(RuntimeError, match="xw must be"):
            dcall(xw=bad)
    for bad in (dgood["D1t"].float(), z(Dd, C + 64), z(C, Dd).t(), None):
        with pytest.raises(RuntimeError, match="D1t must be"):
            dcall(D1t=bad)
    for bad in (dgood["D2t"].float(), z(192, 2 * Dd), z(Dd, 192).t(), None):
        with pytest.raises(RuntimeError, match="D2t must be"):
            dcall(D2t=bad)
    for bad in (dgood["td"].float(), z(128), None):
        with pytest.raises(RuntimeError, match="time_decay must be"):
            dcall(td=bad)
    for dd in (32, 96, 256):
        with pytest.raises(RuntimeError, match="Dd must be one of"):
            dcall(D1t=z(dd, C), D2t=z(192, dd))
    with pytest.raises(RuntimeError, match="multiples of 64"):
        dcall(D2t=z(96, Dd), td=z(96))
    for t in ("xw", "D1t", "D2t", "td"):
        with pytest.raises(RuntimeError, match="has no backward"):
            dcall(**{t: dgood[t].clone().requires_grad_()})
