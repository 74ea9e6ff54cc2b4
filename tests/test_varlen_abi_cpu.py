"""CPU tier of the packed variable-length entry points (include/wkv6_amd.h: wkv6_*_varlen_ex, wkv6_ddlerp_varlen_*): bad arguments are
refused with the documented code before anything is launched, and the host-side workspace bound covers what the kernels touch.

The pointers passed here are dummies (1), as in test_mix_abi_cpu.py: every call must return from its argument checks."""
import pytest

from varlen_common import CALLER_LENS, EDGE_LENS, LONG_LENS, bench_lens, exact_workspace_need

EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4
P = 1
W_RAW, IO_F32, S0_PER_BATCH, ALGO_SCAN, CKPT_VALID, BI_KEEP_CKPT, PARTIALS_F32 = 1, 2, 4, 16, 32, 64, 128


@pytest.fixture(scope="module")
def lib():
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


FWD_PTRS = ("cu", "r", "k", "v", "w", "u", "s0", "s_out", "y")
BWD_PTRS = ("cu", "r", "k", "v", "w", "u", "s0", "gy", "gr", "gk", "gv", "gw", "gu", "gs")
OPTIONAL = {"s0", "s_out", "gu", "gs"}


def op_args(bwd, total_T=256, n_seq=3, max_seqlen=128, C=128, H=2, ws=P, ws_bytes=1 << 40, flags=W_RAW, **ptrs):
    names = BWD_PTRS if bwd else FWD_PTRS
    vals = [ptrs.get(n, None if n in OPTIONAL else P) for n in names]
    return (total_T, n_seq, max_seqlen, C, H, *vals, ws, ws_bytes, flags, None)


OPS = {"wkv6_forward_varlen_ex": False, "wkv6_backward_varlen_ex": True}


@pytest.mark.parametrize("name", sorted(OPS))
def test_operator_entry_points_reject_bad_shapes_and_flags(lib, name):
    fn, bwd = getattr(lib, name), OPS[name]
    for kw in ({"C": 96}, {"C": 128, "H": 3}, {"n_seq": 0}, {"n_seq": -2}, {"total_T": 0}, {"total_T": -7}, {"max_seqlen": 0},
               {"max_seqlen": -1}, {"H": 0, "C": 0}):
        assert fn(*op_args(bwd, **kw)) == EINVAL, kw
    for bit in (8, BI_KEEP_CKPT, 256, 1 << 20, 1 << 31):                   # bits no packed call knows
        assert fn(*op_args(bwd, flags=W_RAW | bit)) == EINVAL, bit


@pytest.mark.parametrize("name", sorted(OPS))
def test_operator_entry_points_reject_null_pointers(lib, name):
    fn, bwd = getattr(lib, name), OPS[name]
    for p in (BWD_PTRS if bwd else FWD_PTRS):
        if p not in OPTIONAL:
            assert fn(*op_args(bwd, **{p: None})) == ENULL, p
    if bwd:     # the checkpoints live in the workspace: "valid" without one is a missing pointer
        assert fn(*op_args(True, ws=None, ws_bytes=0, flags=W_RAW | CKPT_VALID)) == ENULL


@pytest.mark.parametrize("name", sorted(OPS))
def test_operator_entry_points_reject_a_short_workspace(lib, name):
    fn, bwd = getattr(lib, name), OPS[name]
    need = lib.wkv6_varlen_workspace_bytes(256, 3, 128, 2)
    assert need > 0
    for short in (0, 1, need - 1):
        assert fn(*op_args(bwd, ws_bytes=short)) == EWORKSPACE, short


@pytest.mark.parametrize("name", sorted(OPS))
def test_operator_entry_points_reject_misaligned_outputs(lib, name):
    """y, gr, gk, gv, gw are zeroed outside the sequences with 16-byte stores: a base that is not 16-byte aligned is refused, after the
    shape, pointer and workspace checks and before anything is launched (every other pointer here is an aligned dummy)."""
    fn, bwd = getattr(lib, name), OPS[name]
    names = BWD_PTRS if bwd else FWD_PTRS
    aligned = {n: 64 for n in names if n not in OPTIONAL}
    for out in (("gr", "gk", "gv", "gw") if bwd else ("y",)):
        for bad in (65, 66, 72):
            assert fn(*op_args(bwd, ws=64, **(aligned | {out: bad}))) == EINVAL, (out, bad)


@pytest.mark.parametrize("name", sorted(OPS))
def test_row_addressing_limit_is_per_sequence_not_per_batch(lib, name):
    """(max_seqlen + 64) * C must stay below 2^31 (2^30 with the fp32 ew decay on the chunked kernels); total_T * C may pass it.  The
    accepted case cannot be launched with dummy pointers, so it is probed through the check that follows the shape checks: a NULL
    required pointer is reported (ENULL) only once the shape has been accepted."""
    fn, bwd = getattr(lib, name), OPS[name]
    C, H = 4096, 64
    big_row = (1 << 31) // C - 64                                             # (max_seqlen + 64) * C == 2^31
    assert fn(*op_args(bwd, total_T=big_row, max_seqlen=big_row, C=C, H=H)) == EUNSUPPORTED
    assert fn(*op_args(bwd, total_T=big_row, max_seqlen=big_row - 1, C=C, H=H, r=None)) == ENULL
    half = (1 << 30) // C - 64
    assert fn(*op_args(bwd, total_T=big_row, max_seqlen=half, C=C, H=H, flags=0)) == EUNSUPPORTED       # fp32 ew, chunked
    assert fn(*op_args(bwd, total_T=big_row, max_seqlen=half - 1, C=C, H=H, flags=0, r=None)) == ENULL
    assert fn(*op_args(bwd, total_T=big_row, max_seqlen=half, C=C, H=H, flags=ALGO_SCAN, r=None)) == ENULL   # the scan kernels: 64-bit
    total = (1 << 31) // C * 4                                                # total_T * C = 2^33
    assert fn(*op_args(bwd, total_T=total, n_seq=total // 512, max_seqlen=512, C=C, H=H, r=None)) == ENULL
    assert fn(*op_args(bwd, total_T=1 << 31, max_seqlen=512, C=C, H=H)) == EUNSUPPORTED                 # cu_seqlens is int32


def test_workspace_bound_is_monotone_and_covers_the_exact_need(lib):
    f = lib.wkv6_varlen_workspace_bytes
    assert f(0, 1, 128, 2) == 0 and f(64, 0, 128, 2) == 0 and f(64, 1, 96, 2) == 0          # bad shapes have no size
    prev = 0
    for total in (1, 63, 64, 65, 1000, 4096, 1 << 17, 1 << 22):
        cur = f(total, 16, 2048, 32)
        assert cur >= prev > -1
        prev = cur
    prev = 0
    for n_seq in (1, 2, 48, 1000, 1 << 16):
        cur = f(1 << 17, n_seq, 2048, 32)
        assert cur >= prev
        prev = cur
    assert f(4096, 16, 4096, 64) >= f(4096, 16, 2048, 32)
    for lens, H in ((EDGE_LENS, 2), (LONG_LENS, 2), (bench_lens(48), 32), (CALLER_LENS, 2), ([512] * 48, 32), ([1] * 300, 1)):
        total, n_seq = max(sum(lens), 1), len(lens)
        assert f(total, n_seq, 64 * H, H) >= exact_workspace_need(lens, H), lens
        # the scan path's fp32 [total_T, C] scratch lies over the checkpoint area
        assert f(total, n_seq, 64 * H, H) >= (4 * n_seq * 4 + 255) // 256 * 256 + total * 64 * H * 4


# ---- token shift on a packed batch ------------------------------------------------------------------------------------------------
def lerp_fwd(total_T=8, n_seq=2, C=64, NS=1, cu=P, x=P, shifted0=None, m=None, maa=P, out=P):
    return (total_T, n_seq, C, NS, cu, x, shifted0, m, maa, out, None)


def lerp_bwd(total_T=8, n_seq=2, C=64, NS=1, cu=P, x=P, shifted0=None, m=None, maa=P, dout=P, dx=P, dm=None, part=P, nparts=1):
    return (total_T, n_seq, C, NS, cu, x, shifted0, m, maa, dout, dx, dm, part, nparts, None)


LERP = {"wkv6_ddlerp_varlen_forward": lerp_fwd, "wkv6_ddlerp_varlen_backward": lerp_bwd}


@pytest.mark.parametrize("name", sorted(LERP))
def test_ddlerp_varlen_rejects_bad_arguments(lib, name):
    fn, args = getattr(lib, name), LERP[name]
    bwd = "backward" in name
    for kw in ({"total_T": 0}, {"total_T": -3}, {"n_seq": 0}, {"n_seq": -1}, {"C": 0}, {"C": 32}, {"C": 96}, {"C": 4160}):
        assert fn(*args(**kw)) == EINVAL, kw
    if bwd:
        for nparts in (0, -1):
            assert fn(*args(nparts=nparts)) == EINVAL
    assert fn(*args(total_T=1 << 31)) == EUNSUPPORTED                         # cu_seqlens is int32
    for NS, m in ((2, P), (3, None), (5, None), (4, P), (0, None)):           # the (NS, m) pairs of the dense kernels, no others
        kw = dict(NS=NS, m=m) | ({"dm": P} if bwd and m else {})
        assert fn(*args(**kw)) == EUNSUPPORTED, (NS, m)
    required = ["cu", "x", "maa", "dout", "dx", "part"] if bwd else ["cu", "x", "maa", "out"]
    base = dict(NS=5, m=P) | ({"dm": P} if bwd else {})
    for p in required:
        assert fn(*args(**(base | {p: None}))) == ENULL, p
    if bwd:
        assert fn(*args(NS=5, m=P, dm=None)) == ENULL


def test_python_wrappers_refuse_what_a_packed_call_cannot_express():
    import torch
    from rwkv_lm_ext_amd import mix_op, wkv6_op
    x = torch.zeros(1, 8, 64)
    with pytest.raises(RuntimeError):
        mix_op.ddlerp(x, torch.zeros(1, 64), cu_seqlens=torch.tensor([0, 8], dtype=torch.int32), rev_n=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        wkv6_op.new_varlen_workspace(0, 1, 128, 2, "cpu")
    t = torch.zeros(8, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):                                          # no CPU path, and cu_seqlens must be int32
        wkv6_op.forward_varlen_ex(t, t, t, t, torch.zeros(2, 64, dtype=torch.bfloat16), 2, torch.tensor([0, 8]), 8)
    assert hasattr(torch.ops.wkv6, "forward_varlen") and hasattr(torch.ops.wkv6, "backward_varlen")


# ---- the preparation rules on the many-sequence sets (the GPU tier holds the device's arrays to this model) ---------------------------
def test_many_sequence_sets_are_what_the_gpu_tier_expects():
    from varlen_common import MANY_SETS, TIE_LENS
    n600, n257 = MANY_SETS["600"], MANY_SETS["257"]
    slots = lambda lens: sum((n + 63) // 64 for n in lens)
    assert (len(n600), sum(n600), n600.count(0), slots(n600), sum(n600) // 64 + 600) == (600, 22041, 56, 723, 944)
    assert (len(n257), sum(n257), n257.count(0), slots(n257), sum(n257) // 64 + 257) == (257, 9112, 26, 304, 399)
    assert MANY_SETS["256"] == n600[:256] and len(MANY_SETS["513"]) == 513          # one stream of draws
    assert len(TIE_LENS) == 300 and sorted(set(TIE_LENS)) == [0, 64] and TIE_LENS[:100] == TIE_LENS[200:] == [0] * 100


@pytest.mark.parametrize("cut", [None, 64], ids=["whole", "cut64"])
@pytest.mark.parametrize("name", ["256", "257", "513", "600", "ties"])
def test_preparation_model_invariants(name, cut):
    import numpy as np
    from varlen_common import MANY_SETS, cu_of, prepare_model
    given = MANY_SETS[name]
    n_seq, total = len(given), sum(given)
    max_seqlen = cut or max(given)
    ck_stride = total // 64 + n_seq
    lens, tok_off, ck_off, order = prepare_model(cu_of(given), total, max_seqlen, ck_stride)
    assert lens.tolist() == [min(n, max_seqlen) for n in given] and tok_off.tolist() == cu_of(given)[:-1].tolist()
    # the rows are inside the tensors and do not overlap
    assert (tok_off >= 0).all() and (tok_off + lens <= total).all() and (tok_off[1:] >= tok_off[:-1] + lens[:-1]).all()
    # checkpoint slots: back to back in sequence order, none shared, all below the host-side bound
    n_slots = (lens.astype(np.int64) + 63) // 64
    assert ck_off[0] == 0 and (ck_off[1:] == ck_off[:-1] + n_slots[:-1]).all()
    assert ck_off[-1] + n_slots[-1] == n_slots.sum() <= ck_stride
    # dispatch order: a permutation, longest first, ties by index
    assert sorted(order.tolist()) == list(range(n_seq))
    ranked = lens[order]
    assert (ranked[:-1] >= ranked[1:]).all()
    assert all(order[i] < order[i + 1] for i in range(n_seq - 1) if ranked[i] == ranked[i + 1])


def test_preparation_model_clamps_what_lies_outside():
    from varlen_common import prepare_model
    lens, tok_off, ck_off, order = prepare_model([37, 137, 437, 9999], 551, 128, 551 // 64 + 3)
    assert lens.tolist() == [100, 128, 114] and tok_off.tolist() == [37, 137, 437] and ck_off.tolist() == [0, 2, 4]
    assert order.tolist() == [1, 2, 0]
    lens, tok_off, ck_off, order = prepare_model([0, 0, 0, 0], 450, 450, 450 // 64 + 3)
    assert lens.tolist() == [0, 0, 0] and ck_off.tolist() == [0, 0, 0] and order.tolist() == [0, 1, 2]
    lens, *_ = prepare_model([0, 640, 1280], 1280, 640, 10)                  # a bound that is too small: the row that passes it gets length 0
    assert lens.tolist() == [640, 0]
