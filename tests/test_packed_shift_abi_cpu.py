"""CPU tier of the token-shift slot pool (include/wkv6_amd.h: wkv6_ddlerp_slots_forward, wkv6_shift_keep): the symbols are exported with
the documented argument lists, every documented refusal returns its code before anything is launched, the Python wrappers
(mix_op.ddlerp_slots, mix_op.shift_keep, Tmix_x060.jit_func(shift_pool=, slots=)) refuse what they can see is wrong before they call the
library, and infctx's pool_kernels=True raises where the kernels do not apply.

The pointers passed here are dummies (multiples of 64 far apart, never dereferenced), as in test_rwkv6_snap_abi_cpu.py."""
import ctypes
import os
import re

import pytest

EINVAL, ENULL, EUNSUPPORTED = -1, -2, -4
X, POOL, OUT, P = 1 << 30, 2 << 30, 3 << 30, 64        # x, the pool and out: 1 GiB apart, so no test shape makes them overlap
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


def lerp_args(total_T=256, n_seq=3, C=128, NS=1, cu=P, x=X, pool=POOL, n_slots=8, slot=P, m=None, maa=P, out=OUT):
    return (total_T, n_seq, C, NS, cu, x, pool, n_slots, slot, m, maa, out, None)


def keep_args(total_T=256, n_seq=3, max_seqlen=128, C=128, cu=P, x=X, pool=POOL, n_slots=8, slot_out=P, snap_every=3, cu_snap=P,
              snap_slot=P, n_snap=4):
    return (total_T, n_seq, max_seqlen, C, cu, x, pool, n_slots, slot_out, snap_every, cu_snap, snap_slot, n_snap, None)


def test_symbols_and_signatures(lib):
    from rwkv_lm_ext_amd import _lib
    header = open(os.path.join(ROOT, "include", "wkv6_amd.h")).read()
    I, L, VP = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    want = {"wkv6_ddlerp_slots_forward": ([L, I, I, I, VP, VP, VP, I, VP, VP, VP, VP, VP],
                                          ["long total_T", "int n_seq", "int C", "int NS", "const int* cu_seqlens", "const void* x",
                                           "const void* shift_pool", "int n_slots", "const int* slot", "const void* m", "const void* maa",
                                           "void* out", "void* stream"]),
            "wkv6_shift_keep": ([L, I, I, I, VP, VP, VP, I, VP, I, VP, VP, I, VP],
                                ["long total_T", "int n_seq", "int max_seqlen", "int C", "const int* cu_seqlens", "const void* x",
                                 "void* shift_pool", "int n_slots", "const int* slot_out", "int snap_every", "const int* cu_snap",
                                 "const int* snap_slot", "int n_snap", "void* stream"])}
    for name, (argtypes, params) in want.items():
        fn = getattr(lib, name)
        res, table = _lib.SIGNATURES[name]
        assert res is I and list(table) == argtypes
        assert fn.restype is I and list(fn.argtypes) == argtypes
        decl = re.search(r"int " + name + r"\(([^;]*)\);", header).group(1)
        assert [" ".join(p.split()) for p in decl.split(",")] == params


def test_ddlerp_slots_refusals(lib):
    fn = lib.wkv6_ddlerp_slots_forward
    for kw in ({"C": 96}, {"C": 32}, {"C": 0}, {"C": 4160}, {"total_T": 0}, {"total_T": -3}, {"n_seq": 0}, {"n_seq": -1}, {"n_slots": 0},
               {"n_slots": -8}):
        assert fn(*lerp_args(**kw)) == EINVAL, kw
    assert fn(*lerp_args(slot=None, n_slots=2)) == EINVAL                   # slot = sequence index: the pool must hold n_seq slots
    assert fn(*lerp_args(slot=None, n_slots=3, maa=None)) == ENULL          # (... and with 3 slots the call goes on to the next check)
    for p in ("cu", "x", "pool", "maa", "out"):
        assert fn(*lerp_args(**{p: None})) == ENULL, p
    for p, base in (("x", X), ("out", OUT), ("pool", POOL)):
        for off in (1, 2, 4, 6):
            assert fn(*lerp_args(**{p: base + off})) == EINVAL, (p, off)
    # out [NS,total_T,C] against the pool [n_slots,C] (2 bytes an element): touching at either end is an overlap, one row apart is not
    T, C, n = 256, 128, 8
    for NS, m in ((1, None), (2, None), (5, P)):
        assert fn(*lerp_args(NS=NS, m=m, out=POOL - NS * T * C * 2 + 8)) == EINVAL, NS
        assert fn(*lerp_args(NS=NS, m=m, out=POOL + n * C * 2 - 8)) == EINVAL, NS
        assert fn(*lerp_args(NS=NS, m=m, out=POOL)) == EINVAL, NS
        assert fn(*lerp_args(NS=NS, m=m, out=POOL - NS * T * C * 2, maa=None)) == ENULL, NS        # adjacent: accepted so far
        assert fn(*lerp_args(NS=NS, m=m, out=POOL + n * C * 2, maa=None)) == ENULL, NS
    assert fn(*lerp_args(total_T=(1 << 31), C=64)) == EUNSUPPORTED
    assert fn(*lerp_args(total_T=(1 << 31) - 1, C=64, maa=None)) == ENULL
    # the (NS, m) pairs of the ddlerp: everything else is EUNSUPPORTED, behind every argument check
    for NS, m in ((2, P), (5, None), (3, None), (0, None), (4, P)):
        assert fn(*lerp_args(NS=NS, m=m)) == EUNSUPPORTED, (NS, m)


def test_shift_keep_refusals(lib):
    fn = lib.wkv6_shift_keep
    for kw in ({"C": 96}, {"C": 32}, {"C": 4160}, {"total_T": 0}, {"total_T": -3}, {"n_seq": 0}, {"n_seq": -1}, {"n_slots": 0},
               {"n_slots": -8}, {"max_seqlen": 0}, {"max_seqlen": -5}, {"snap_every": -1}, {"snap_every": -64}, {"n_snap": -1},
               {"snap_every": 0, "n_snap": -2}):
        assert fn(*keep_args(**kw)) == EINVAL, kw
    assert fn(*keep_args(slot_out=None, n_slots=2)) == EINVAL
    assert fn(*keep_args(slot_out=None, n_slots=3, x=None)) == ENULL
    for p in ("cu", "x", "pool"):
        assert fn(*keep_args(**{p: None})) == ENULL, p
    assert fn(*keep_args(cu_snap=None)) == ENULL
    assert fn(*keep_args(snap_slot=None)) == ENULL
    assert fn(*keep_args(cu_snap=None, snap_slot=None)) == ENULL
    for p, base in (("x", X), ("pool", POOL)):
        for off in (1, 2, 4, 6):
            assert fn(*keep_args(**{p: base + off})) == EINVAL, (p, off)
    T, C, n = 256, 128, 8
    for x in (POOL, POOL - T * C * 2 + 8, POOL + n * C * 2 - 8, POOL + 256):
        assert fn(*keep_args(x=x)) == EINVAL, x
    assert fn(*keep_args(total_T=(1 << 31), C=64)) == EUNSUPPORTED
    # accepted, probed through a check that comes later: an unaligned x is EINVAL only if nothing before it refused the call
    for ok in (dict(snap_every=0, cu_snap=None, snap_slot=None, n_snap=0), dict(snap_every=0, cu_snap=None, snap_slot=None),
               dict(n_snap=0, cu_snap=None, snap_slot=None), dict(snap_every=1), dict(snap_every=3), dict(snap_every=64),
               dict(snap_every=1 << 30), dict(slot_out=None), dict(max_seqlen=1), dict(max_seqlen=(1 << 31) - 1),
               dict(x=POOL - T * C * 2 + 2), dict(x=POOL + n * C * 2 + 2), dict(total_T=(1 << 31) - 1, C=64, x=(1 << 50) + 2)):
        assert fn(*keep_args(**dict(dict(x=X + 2), **ok))) == EINVAL, ok
        assert fn(*keep_args(**dict(ok, x=None))) == ENULL, ok


def test_python_wrappers_refuse_before_calling_the_library(monkeypatch):
    import torch
    from rwkv_lm_ext_amd import _lib, mix_op

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", no_library)
    bf, i32 = torch.bfloat16, torch.int32
    T, C, n_seq, n = 8, 128, 2, 4
    x, pool, maa = torch.zeros(1, T, C, dtype=bf), torch.zeros(n, C, dtype=bf), torch.zeros(1, C, dtype=bf)
    cu, slots = torch.tensor([0, 3, 8], dtype=i32), torch.zeros(n_seq, dtype=i32)
    snap = (3, torch.zeros(n_seq + 1, dtype=i32), torch.zeros(5, dtype=i32))

    with pytest.raises(RuntimeError, match="must be on the GPU"):            # everything else is right: no CPU path
        mix_op.ddlerp_slots(x, maa, None, pool, slots, cu)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        mix_op.shift_keep(x, cu, T, pool, slots, snap)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        mix_op.shift_keep(x[0], cu, T, pool, None)
    for call in (lambda **o: mix_op.ddlerp_slots(o.get("x", x), maa, None, o.get("pool", pool), o.get("slots", slots), o.get("cu", cu)),
                 lambda **o: mix_op.shift_keep(o.get("x", x), o.get("cu", cu), T, o.get("pool", pool), o.get("slots", slots), snap)):
        for bad in (x.float(), x.half(), torch.zeros(2, T, C, dtype=bf), torch.zeros(T * C, dtype=bf), None):
            with pytest.raises(RuntimeError, match="x must be|a packed batch is"):
                call(x=bad)
        for bad in (pool.float(), torch.zeros(n, 2 * C, dtype=bf)[:, :C], torch.zeros(n, C + 64, dtype=bf), torch.zeros(1, n, C, dtype=bf), None):
            with pytest.raises(RuntimeError, match="shift_pool must be"):
                call(pool=bad)
        for bad in (cu.long(), torch.zeros(1, dtype=i32), torch.zeros(6, dtype=i32)[::2], [0, 3, 8], None):
            with pytest.raises(RuntimeError, match="cu_seqlens must be"):
                call(cu=bad)
        for bad in (slots.long(), torch.zeros(3, dtype=i32), torch.zeros(4, dtype=i32)[::2], [0, 1]):
            with pytest.raises(RuntimeError, match="slot(s|_out) must be"):
                call(slots=bad)
    with pytest.raises(RuntimeError, match="the pool must hold n_seq slots"):
        mix_op.ddlerp_slots(x, maa, None, pool[:1], None, cu)
    with pytest.raises(RuntimeError, match="the pool must hold n_seq slots"):
        mix_op.shift_keep(x, cu, T, pool[:1], None)
    # the lerp's own arguments
    with pytest.raises(RuntimeError, match="maa must be"):
        mix_op.ddlerp_slots(x, maa.float(), None, pool, slots, cu)
    with pytest.raises(RuntimeError, match="m must be"):
        mix_op.ddlerp_slots(x, maa, torch.zeros(1, 1, T, C), pool, slots, cu)
    with pytest.raises(RuntimeError, match="m must be"):
        mix_op.ddlerp_slots(x, maa, torch.zeros(5, 1, T, C, dtype=bf), pool, slots, cu)
    for NS, m in ((2, torch.zeros(2, 1, T, C, dtype=bf)), (5, None), (3, None)):
        with pytest.raises(RuntimeError, match="supported are"):
            mix_op.ddlerp_slots(x, torch.zeros(NS, C, dtype=bf), m, pool, slots, cu)
    for t in ("x", "maa"):
        with pytest.raises(RuntimeError, match="has no backward"):
            mix_op.ddlerp_slots(x.clone().requires_grad_(t == "x"), maa.clone().requires_grad_(t == "maa"), None, pool, slots, cu)
    with torch.no_grad(), pytest.raises(RuntimeError, match="must be on the GPU"):      # ... which no_grad lifts
        mix_op.ddlerp_slots(x.clone().requires_grad_(), maa, None, pool, slots, cu)
    # shift_keep's own arguments
    for bad in (0, -1, 2.0, "8", None, True):
        with pytest.raises(RuntimeError, match="max_seqlen must be"):
            mix_op.shift_keep(x, cu, bad, pool, slots)
    for bad in (-1, 3.0, "3", None, True):
        with pytest.raises(RuntimeError, match="snap_every must be"):
            mix_op.shift_keep(x, cu, T, pool, slots, (bad,) + snap[1:])
    for bad in (None, snap[1].long(), torch.zeros(2, dtype=i32), torch.zeros(4, dtype=i32)):
        with pytest.raises(RuntimeError, match="cu_snap must be"):
            mix_op.shift_keep(x, cu, T, pool, slots, (3, bad, snap[2]))
    for bad in (None, snap[2].float(), torch.zeros(2, 2, dtype=i32), (1, 2)):
        with pytest.raises(RuntimeError, match="snap_slots must be"):
            mix_op.shift_keep(x, cu, T, pool, slots, (3, snap[1], bad))
    with pytest.raises(RuntimeError, match="must be on the GPU"):            # snap_every = 0: the arrays are not looked at
        mix_op.shift_keep(x, cu, T, pool, slots, (0, None, None))
    with pytest.raises(RuntimeError, match="has no backward"):
        mix_op.shift_keep(x, cu, T, pool.clone().requires_grad_(), slots)


def test_jit_func_and_pool_kernels_refuse_where_the_kernels_do_not_apply(monkeypatch):
    import torch
    from rwkv_lm_ext_amd import _lib, callers, infctx

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", no_library)
    bf, i32 = torch.bfloat16, torch.int32
    T, C, n = 8, 128, 4
    tm, cm = callers.Tmix_x060(C, C), callers.CMix_x060(C, 2 * C)
    x = torch.zeros(1, T, C)
    cu, slots = torch.tensor([0, 3, 8], dtype=i32), torch.zeros(2, dtype=i32)
    pool, wkv = torch.zeros(n, C), torch.zeros(n, C // 64, 64, 64)
    # jit_func: the pool excludes shifted0, needs a packed batch, and exists in the fused path only
    with pytest.raises(AssertionError, match="shift_pool / slots belong to a packed batch"):
        tm.jit_func(x, cu_seqlens=cu, shifted0=torch.zeros(2, C), shift_pool=pool, slots=slots)
    with pytest.raises(AssertionError, match="shift_pool / slots belong to a packed batch"):
        tm.jit_func(x, shift_pool=pool, slots=slots)
    with pytest.raises(AssertionError, match="slots name rows of shift_pool"):
        tm.jit_func(x, cu_seqlens=cu, slots=slots)
    with pytest.raises(RuntimeError, match="fused .HIP. path only"):
        tm.jit_func(x, cu_seqlens=cu, shift_pool=pool, slots=slots)
    # pool_kernels=True on fp32 CPU tensors: the fused path does not apply
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="pool_kernels=True: the module's fused"):
            infctx.tmix_forward_packed(tm, x, cu, T, pool, wkv, slots, pool_kernels=True)
        with pytest.raises(RuntimeError, match="pool_kernels=True: the module's fused"):
            infctx.cmix_forward_packed(cm, x, cu, pool, slots, pool_kernels=True)
    # the other two conditions, with the fused path forced on (nothing is launched: the refusal comes first).  bf16 "GPU" activations are
    # needed to get that far, so this part runs where there is a GPU
    if torch.cuda.is_available():
        tm, cm = tm.cuda().to(bf), cm.cuda().to(bf)
        xg, cug, sg = x.cuda().to(bf), cu.cuda(), slots.cuda()
        for bad in (pool.cuda(), pool.cuda().half(), torch.zeros(n, 2 * C, dtype=bf, device="cuda")[:, :C], pool.to(bf)):
            with torch.no_grad(), pytest.raises(RuntimeError, match="pool_kernels=True: the shift pool must be"):
                infctx.cmix_forward_packed(cm, xg, cug, bad, sg, pool_kernels=True)
            with torch.no_grad(), pytest.raises(RuntimeError, match="pool_kernels=True: the shift pool must be"):
                infctx.tmix_forward_packed(tm, xg, cug, T, bad, wkv.cuda(), sg, pool_kernels=True)
        with pytest.raises(RuntimeError, match="pool_kernels=True: a gradient is required"):
            infctx.cmix_forward_packed(cm, xg, cug, pool.cuda().to(bf), sg, pool_kernels=True)
        with pytest.raises(RuntimeError, match="pool_kernels=True: a gradient is required"):
            infctx.tmix_forward_packed(tm, xg, cug, T, pool.cuda().to(bf), wkv.cuda(), sg, pool_kernels=True)
    # the new functions are there
    pools = infctx.PackedPools.create(2, 5, C, C // 64, "cpu", bf)
    assert tuple(pools.shift_att.shape) == tuple(pools.shift_ffn.shape) == (2, 5, C) and pools.shift_att.dtype == bf
    assert tuple(pools.wkv.shape) == (2, 5, C // 64, 64, 64) and pools.wkv.dtype == torch.float32
    assert not pools.shift_att.any() and not pools.shift_ffn.any() and not pools.wkv.any()
    assert all(callable(getattr(infctx, f)) for f in ("block_forward_packed", "step_packed", "last_token_rows"))
