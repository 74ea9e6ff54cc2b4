"""CPU tier of the packed reversal-map and pair entry points (include/wkv6_amd.h: wkv6_*_varlen_rev_ex, wkv6_*_varlen_pair_ex,
wkv6_ddlerp_varlen_rev_*): bad arguments are refused with the documented code before anything is launched.

The pointers passed here are dummies, as in test_varlen_abi_cpu.py: every call must return from its argument checks.  An accepted
argument is probed through the check that follows it (a NULL required pointer is reported only once everything before it was accepted)."""
import ctypes

import pytest

EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4
P = 1
W_RAW, IO_F32, S0_PER_BATCH, ALGO_SCAN, CKPT_VALID, BI_KEEP_CKPT, PARTIALS_F32 = 1, 2, 4, 16, 32, 64, 128
REV_ALL = 31
SYMBOLS = ("wkv6_forward_varlen_rev_ex", "wkv6_backward_varlen_rev_ex", "wkv6_forward_varlen_pair_ex", "wkv6_backward_varlen_pair_ex",
           "wkv6_ddlerp_varlen_rev_forward", "wkv6_ddlerp_varlen_rev_backward")


@pytest.fixture(scope="module")
def lib():
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


def test_the_six_symbols_exist_and_are_declared(lib):
    import os
    from rwkv_lm_ext_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wkv6_amd.h")).read()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None and name in _lib.SIGNATURES and f"int {name}(" in header, name
    assert "reversal maps, the pair" not in header                      # the "Not available packed" sentence no longer lists them


# ---- rev calls ------------------------------------------------------------------------------------------------------------------------
FWD_PTRS = ("cu", "r", "k", "v", "w", "u", "y")
BWD_PTRS = ("cu", "r", "k", "v", "w", "u", "gy", "gr", "gk", "gv", "gw", "gu")
OPTIONAL = {"gu"}
REV = {"wkv6_forward_varlen_rev_ex": False, "wkv6_backward_varlen_rev_ex": True}


def rev_args(bwd, total_T=256, n_seq=3, max_seqlen=128, C=128, H=2, ws=P, ws_bytes=1 << 40, rev_n=P, rev_mask=REV_ALL, flags=W_RAW, **ptrs):
    names = BWD_PTRS if bwd else FWD_PTRS
    vals = [ptrs.get(n, None if n in OPTIONAL else P) for n in names]
    return (total_T, n_seq, max_seqlen, C, H, *vals, ws, ws_bytes, rev_n, rev_mask, flags, None)


@pytest.mark.parametrize("name", sorted(REV))
def test_rev_calls_reject_bad_shapes_flags_and_masks(lib, name):
    fn, bwd = getattr(lib, name), REV[name]
    for kw in ({"C": 96}, {"C": 128, "H": 3}, {"n_seq": 0}, {"n_seq": -2}, {"total_T": 0}, {"total_T": -7}, {"max_seqlen": 0},
               {"max_seqlen": -1}, {"H": 0, "C": 0}):
        assert fn(*rev_args(bwd, **kw)) == EINVAL, kw
    for bit in (8, BI_KEEP_CKPT, 256, 1 << 20, 1 << 31, S0_PER_BATCH):       # no initial state here: S0_PER_BATCH is an unknown bit
        assert fn(*rev_args(bwd, flags=W_RAW | bit)) == EINVAL, bit
    for mask in (32, 64, REV_ALL | 32, 1 << 31):
        assert fn(*rev_args(bwd, rev_mask=mask)) == EINVAL, mask
    for flags in (W_RAW, 0, W_RAW | IO_F32, W_RAW | ALGO_SCAN, W_RAW | PARTIALS_F32, W_RAW | CKPT_VALID):   # known bits reach the pointer check
        assert fn(*rev_args(bwd, flags=flags, r=None)) == ENULL, flags


@pytest.mark.parametrize("name", sorted(REV))
def test_rev_calls_reject_null_pointers_and_accept_a_null_map(lib, name):
    fn, bwd = getattr(lib, name), REV[name]
    for p in (BWD_PTRS if bwd else FWD_PTRS):
        if p not in OPTIONAL:
            assert fn(*rev_args(bwd, **{p: None})) == ENULL, p
    if bwd:
        assert fn(*rev_args(True, ws=None, ws_bytes=0, flags=W_RAW | CKPT_VALID)) == ENULL
    # rev_n = NULL (no map) is accepted: the call goes on to the checks behind the pointers
    assert fn(*rev_args(bwd, rev_n=None, ws_bytes=1)) == EWORKSPACE
    aligned = {n: 64 for n in (BWD_PTRS if bwd else FWD_PTRS) if n not in OPTIONAL}
    assert fn(*rev_args(bwd, rev_n=None, ws=64, **(aligned | {("gw" if bwd else "y"): 72}))) == EINVAL


@pytest.mark.parametrize("name", sorted(REV))
def test_rev_calls_reject_a_short_workspace_and_misaligned_outputs(lib, name):
    fn, bwd = getattr(lib, name), REV[name]
    need = lib.wkv6_varlen_workspace_bytes(256, 3, 128, 2)
    assert need > 0
    for short in (0, 1, need - 1):
        assert fn(*rev_args(bwd, ws_bytes=short)) == EWORKSPACE, short
    names = BWD_PTRS if bwd else FWD_PTRS
    aligned = {n: 64 for n in names if n not in OPTIONAL}
    for out in (("gr", "gk", "gv", "gw") if bwd else ("y",)):
        for bad in (65, 66, 72):
            assert fn(*rev_args(bwd, ws=64, rev_n=64, **(aligned | {out: bad}))) == EINVAL, (out, bad)


@pytest.mark.parametrize("name", sorted(REV))
def test_rev_calls_keep_the_per_sequence_row_limit(lib, name):
    fn, bwd = getattr(lib, name), REV[name]
    C, H = 4096, 64
    big_row = (1 << 31) // C - 64                                             # (max_seqlen + 64) * C == 2^31
    assert fn(*rev_args(bwd, total_T=big_row, max_seqlen=big_row, C=C, H=H)) == EUNSUPPORTED
    assert fn(*rev_args(bwd, total_T=big_row, max_seqlen=big_row - 1, C=C, H=H, r=None)) == ENULL
    half = (1 << 30) // C - 64
    assert fn(*rev_args(bwd, total_T=big_row, max_seqlen=half, C=C, H=H, flags=0)) == EUNSUPPORTED       # fp32 ew, chunked
    assert fn(*rev_args(bwd, total_T=big_row, max_seqlen=half - 1, C=C, H=H, flags=0, r=None)) == ENULL
    assert fn(*rev_args(bwd, total_T=big_row, max_seqlen=half, C=C, H=H, flags=ALGO_SCAN, r=None)) == ENULL
    total = (1 << 31) // C * 4                                                # total_T * C = 2^33
    assert fn(*rev_args(bwd, total_T=total, n_seq=total // 512, max_seqlen=512, C=C, H=H, r=None)) == ENULL
    assert fn(*rev_args(bwd, total_T=1 << 31, max_seqlen=512, C=C, H=H)) == EUNSUPPORTED                 # cu_seqlens is int32


# ---- pair calls -----------------------------------------------------------------------------------------------------------------------
PAIR = {"wkv6_forward_varlen_pair_ex": False, "wkv6_backward_varlen_pair_ex": True}
IN = ("r", "k", "v", "w")
FWD_SET, BWD_SET = IN + ("y",), IN + ("gy", "gr", "gk", "gv", "gw", "ckpt")


def seq_sets(bwd, over=None, value=64):
    """Two fully populated sets of aligned dummies; over: {(set index, member): value}."""
    from rwkv_lm_ext_amd import _lib
    arr = (_lib.SeqSet * 2)()
    for i, e in enumerate(arr):
        for n in IN + ("y", "gy", "gr", "gk", "gv", "gw", "gu", "ckpt", "rev_n"):
            setattr(e, n, value)
        e.ckpt_bytes, e.rev_mask = 1 << 40, REV_ALL
    for (i, n), v in (over or {}).items():
        setattr(arr[i], n, v)
    return arr


def pair_args(arr, total_T=256, n_seq=3, max_seqlen=128, C=128, H=2, cu=P, u=P, flags=W_RAW):
    return (total_T, n_seq, max_seqlen, C, H, cu, u, arr, flags, None)


@pytest.mark.parametrize("name", sorted(PAIR))
def test_pair_calls_reject_bad_shapes_flags_and_masks(lib, name):
    fn, bwd = getattr(lib, name), PAIR[name]
    for kw in ({"C": 96}, {"C": 128, "H": 3}, {"n_seq": 0}, {"total_T": 0}, {"max_seqlen": 0}, {"max_seqlen": -1}, {"H": 0, "C": 0}):
        assert fn(*pair_args(seq_sets(bwd), **kw)) == EINVAL, kw
    for bit in (8, BI_KEEP_CKPT, 256, 1 << 20, 1 << 31, S0_PER_BATCH, CKPT_VALID):
        assert fn(*pair_args(seq_sets(bwd), flags=W_RAW | bit)) == EINVAL, bit
    for bit in (IO_F32, ALGO_SCAN, IO_F32 | ALGO_SCAN):
        assert fn(*pair_args(seq_sets(bwd), flags=W_RAW | bit)) == EUNSUPPORTED, bit
    for i in (0, 1):
        assert fn(*pair_args(seq_sets(bwd, {(i, "rev_mask"): 32}))) == EINVAL, i
    for flags in (W_RAW, 0, W_RAW | PARTIALS_F32):
        assert fn(*pair_args(seq_sets(bwd), flags=flags, u=None)) == ENULL, flags


@pytest.mark.parametrize("name", sorted(PAIR))
def test_pair_calls_reject_null_pointers(lib, name):
    fn, bwd = getattr(lib, name), PAIR[name]
    null_sets = ctypes.POINTER(type(seq_sets(bwd)[0]))()
    assert fn(*pair_args(null_sets)) == ENULL
    assert fn(*pair_args(seq_sets(bwd), cu=None)) == ENULL
    assert fn(*pair_args(seq_sets(bwd), u=None)) == ENULL
    for i in (0, 1):
        for member in (BWD_SET if bwd else FWD_SET):
            assert fn(*pair_args(seq_sets(bwd, {(i, member): None}))) == ENULL, (i, member)


@pytest.mark.parametrize("name", sorted(PAIR))
def test_pair_calls_reject_short_workspaces_and_misaligned_outputs(lib, name):
    fn, bwd = getattr(lib, name), PAIR[name]
    need = lib.wkv6_varlen_workspace_bytes(256, 3, 128, 2)
    for i in (0, 1):
        for short in (0, 1, need - 1):
            assert fn(*pair_args(seq_sets(bwd, {(i, "ckpt_bytes"): short}))) == EWORKSPACE, (i, short)
        for out in (("gr", "gk", "gv", "gw") if bwd else ("y",)):
            for bad in (65, 72):
                assert fn(*pair_args(seq_sets(bwd, {(i, out): bad}))) == EINVAL, (i, out, bad)


@pytest.mark.parametrize("name", sorted(PAIR))
def test_pair_calls_keep_the_per_sequence_row_limit(lib, name):
    fn, bwd = getattr(lib, name), PAIR[name]
    C, H = 4096, 64
    big_row = (1 << 31) // C - 64
    assert fn(*pair_args(seq_sets(bwd), total_T=big_row, max_seqlen=big_row, C=C, H=H)) == EUNSUPPORTED
    assert fn(*pair_args(seq_sets(bwd), total_T=big_row, max_seqlen=big_row - 1, C=C, H=H, u=None)) == ENULL
    half = (1 << 30) // C - 64
    assert fn(*pair_args(seq_sets(bwd), total_T=big_row, max_seqlen=half, C=C, H=H, flags=0)) == EUNSUPPORTED
    assert fn(*pair_args(seq_sets(bwd), total_T=big_row, max_seqlen=half - 1, C=C, H=H, flags=0, u=None)) == ENULL
    assert fn(*pair_args(seq_sets(bwd), total_T=1 << 31, max_seqlen=512, C=C, H=H)) == EUNSUPPORTED


# ---- token shift ----------------------------------------------------------------------------------------------------------------------
def lerp_fwd(total_T=8, n_seq=2, C=64, NS=1, cu=P, x=P, shifted0=None, m=None, maa=P, rev_n=P, out=P):
    return (total_T, n_seq, C, NS, cu, x, shifted0, m, maa, rev_n, out, None)


def lerp_bwd(total_T=8, n_seq=2, C=64, NS=1, cu=P, x=P, shifted0=None, m=None, maa=P, rev_n=P, dout=P, dx=P, dm=None, part=P, nparts=1):
    return (total_T, n_seq, C, NS, cu, x, shifted0, m, maa, rev_n, dout, dx, dm, part, nparts, None)


@pytest.mark.parametrize("rev_n", [P, None], ids=["map", "no_map"])
def test_token_shift_entry_points_check_their_arguments(lib, rev_n):
    f, b = lib.wkv6_ddlerp_varlen_rev_forward, lib.wkv6_ddlerp_varlen_rev_backward
    for kw in ({"total_T": 0}, {"n_seq": 0}, {"C": 96}, {"C": 32}):
        assert f(*lerp_fwd(rev_n=rev_n, **kw)) == EINVAL and b(*lerp_bwd(rev_n=rev_n, **kw)) == EINVAL, kw
    assert b(*lerp_bwd(rev_n=rev_n, nparts=0)) == EINVAL
    assert f(*lerp_fwd(rev_n=rev_n, total_T=1 << 31)) == EUNSUPPORTED and b(*lerp_bwd(rev_n=rev_n, total_T=1 << 31)) == EUNSUPPORTED
    for p in ("cu", "x", "maa", "out"):
        assert f(*lerp_fwd(rev_n=rev_n, **{p: None})) == ENULL, p
    for p in ("cu", "x", "maa", "dout", "dx", "part"):
        assert b(*lerp_bwd(rev_n=rev_n, **{p: None})) == ENULL, p
    assert b(*lerp_bwd(rev_n=rev_n, m=P, dm=None)) == ENULL
