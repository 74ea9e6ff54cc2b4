"""CPU tier of the packed stateful inference entry points (include/wkv6_amd.h: rwkv6_forward_varlen_bf16 / _fp16 / _fp32): every
documented refusal returns its code before anything is launched, the workspace is the four prepared int32 arrays, and the Python
wrappers refuse what they can see is wrong before they call the library.

The pointers passed here are dummies (64: aligned, never dereferenced), as in test_varlen_abi_cpu.py."""
import pytest

EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4
P = 64
ALGO_SCAN = 16
NAMES = ("rwkv6_forward_varlen_bf16", "rwkv6_forward_varlen_fp16", "rwkv6_forward_varlen_fp32")
PTRS = ("cu", "state_slot", "state_pool", "r", "k", "v", "w", "u", "y")


@pytest.fixture(scope="module")
def lib():
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


def args(total_T=256, n_seq=3, max_seqlen=128, C=128, H=2, n_slots=8, ws=P, ws_bytes=1 << 40, flags=0, **ptrs):
    p = {n: ptrs.get(n, P) for n in PTRS}
    return (total_T, n_seq, max_seqlen, C, H, p["cu"], p["state_slot"], n_slots, p["state_pool"], p["r"], p["k"], p["v"], p["w"], p["u"],
            p["y"], ws, ws_bytes, flags, None)


@pytest.mark.parametrize("name", NAMES)
def test_bad_shapes_slots_and_flags(lib, name):
    fn = getattr(lib, name)
    for kw in ({"C": 96}, {"C": 128, "H": 3}, {"n_seq": 0}, {"n_seq": -2}, {"total_T": 0}, {"total_T": -7}, {"max_seqlen": 0},
               {"max_seqlen": -1}, {"H": 0, "C": 0}, {"n_slots": 0}, {"n_slots": -4}):
        assert fn(*args(**kw)) == EINVAL, kw
    # state_slot NULL: slot = sequence index, so the pool must hold n_seq slots
    assert fn(*args(state_slot=None, n_slots=2)) == EINVAL
    assert fn(*args(state_slot=None, n_slots=3, r=None)) == ENULL            # accepted: the next check reports the missing tensor
    assert fn(*args(n_slots=1, r=None)) == ENULL                            # with a state_slot array any pool of >= 1 slots will do
    for bit in (1, 2, 4, 8, 32, 64, 128, 256, 1 << 20, 1 << 31):            # WKV6_ALGO_SCAN is the only flag these calls know
        assert fn(*args(flags=bit)) == EINVAL, bit
        assert fn(*args(flags=ALGO_SCAN | bit)) == EINVAL, bit
    assert fn(*args(flags=ALGO_SCAN, r=None)) == ENULL


@pytest.mark.parametrize("name", NAMES)
def test_null_pointers(lib, name):
    fn = getattr(lib, name)
    for p in PTRS:
        if p != "state_slot":
            assert fn(*args(**{p: None})) == ENULL, p


@pytest.mark.parametrize("name", NAMES)
def test_short_workspace_and_misaligned_output(lib, name):
    fn = getattr(lib, name)
    need = lib.rwkv6_varlen_workspace_bytes(3)
    for short in (0, 1, need - 1):
        assert fn(*args(ws_bytes=short)) == EWORKSPACE, short
    for bad in (65, 66, 72):                                                # the gap rows of y are zeroed with 16-byte stores
        assert fn(*args(ws_bytes=need, y=bad)) == EINVAL, bad


def test_workspace_is_the_four_int_arrays(lib):
    f = lib.rwkv6_varlen_workspace_bytes
    assert f(0) == 0 and f(-3) == 0
    for n_seq in (1, 2, 16, 17, 64, 65, 1000, 1 << 16):
        assert f(n_seq) == (4 * n_seq * 4 + 255) // 256 * 256, n_seq
        # no checkpoint is kept: the int arrays of the packed training calls, nothing more
        assert f(n_seq) < lib.wkv6_varlen_workspace_bytes(64, n_seq, 128, 2)


def test_row_addressing_limits_follow_the_route(lib):
    """(max_seqlen + 64) * C < 2^30 where the chunked kernel may run (bf16, max_seqlen >= 32, no WKV6_ALGO_SCAN), < 2^31 on the scan route
    (fp16, fp32, WKV6_ALGO_SCAN).  An accepted shape is probed through the check behind the shape checks: a NULL tensor gives ENULL."""
    C, H = 4096, 64
    full, half = (1 << 31) // C - 64, (1 << 30) // C - 64
    bf16, fp16, fp32 = (getattr(lib, n) for n in NAMES)
    big = dict(total_T=full, C=C, H=H)
    assert bf16(*args(max_seqlen=half, **big)) == EUNSUPPORTED
    assert bf16(*args(max_seqlen=half - 1, r=None, **big)) == ENULL
    assert bf16(*args(max_seqlen=half, flags=ALGO_SCAN, r=None, **big)) == ENULL
    for fn in (fp16, fp32):
        assert fn(*args(max_seqlen=half, r=None, **big)) == ENULL
    for fn, fl in ((bf16, ALGO_SCAN), (fp16, 0), (fp32, 0), (fp32, ALGO_SCAN)):
        assert fn(*args(max_seqlen=full, flags=fl, **big)) == EUNSUPPORTED
        assert fn(*args(max_seqlen=full - 1, flags=fl, r=None, **big)) == ENULL
    assert bf16(*args(total_T=1 << 31, max_seqlen=512, C=C, H=H)) == EUNSUPPORTED     # cu_seqlens is int32
    total = (1 << 31) // C * 4                                                       # total_T * C = 2^33: the sequence origin is 64-bit
    assert bf16(*args(total_T=total, n_seq=total // 512, max_seqlen=512, C=C, H=H, n_slots=total // 512, r=None)) == ENULL


def test_python_wrappers_refuse_before_calling_the_library(monkeypatch):
    import torch
    from rwkv_lm_ext_amd import _lib, wkv6_op

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", no_library)
    bf = torch.bfloat16
    T, C, H = 8, 128, 2
    ok = dict(state_pool=torch.zeros(4, H, 64, 64), state_slot=torch.zeros(2, dtype=torch.int32), r=torch.zeros(T, C, dtype=bf),
              k=torch.zeros(T, C, dtype=bf), v=torch.zeros(T, C, dtype=bf), w=torch.zeros(T, C), u=torch.zeros(H, 64, dtype=bf),
              y=torch.zeros(T, C, dtype=bf), cu_seqlens=torch.tensor([0, 3, 8], dtype=torch.int32))
    order = ("state_pool", "state_slot", "r", "k", "v", "w", "u", "y", "cu_seqlens")

    def call(fn=wkv6_op.rwkv6.forward_varlen_bf16, max_seqlen=8, **over):
        a = dict(ok, **over)
        return fn(T, C, H, *(a[n] for n in order), max_seqlen)

    with pytest.raises(RuntimeError, match="must be on the GPU"):            # everything else is right: no CPU path
        call()
    for name, bad in (("state_pool", ok["state_pool"].double()), ("r", ok["r"].float()), ("k", ok["k"].half()), ("w", ok["w"].to(bf)),
                      ("u", ok["u"].float()), ("y", ok["y"].float())):
        with pytest.raises(RuntimeError, match=f"{name} must be torch"):
            call(**{name: bad})
    with pytest.raises(RuntimeError, match="must be torch.float16"):
        call(fn=wkv6_op.rwkv6.forward_varlen_fp16)
    with pytest.raises(RuntimeError, match="must be torch.float32"):
        call(fn=wkv6_op.rwkv6.forward_varlen_fp32)
    for bad in (ok["state_slot"].long(), ok["state_slot"].float(), torch.zeros(3, dtype=torch.int32), [0, 1]):
        with pytest.raises(RuntimeError, match="state_slot must be"):
            call(state_slot=bad)
    with pytest.raises(RuntimeError, match="cu_seqlens must be"):
        call(cu_seqlens=torch.tensor([0, 3, 8]))
    with pytest.raises(RuntimeError, match="state_pool has shape"):
        call(state_pool=torch.zeros(4, H, 64, 32))
    with pytest.raises(RuntimeError, match="slots for 2 sequences"):
        call(state_pool=torch.zeros(1, H, 64, 64), state_slot=None)
    with pytest.raises(RuntimeError, match="max_seqlen"):
        call(max_seqlen=0)
    with pytest.raises(RuntimeError, match="unknown algo"):
        wkv6_op.rwkv6.forward_varlen_bf16(T, C, H, *(ok[n] for n in order), 8, algo="chunk")
    if torch.cuda.is_available():                                           # a state_slot / cu_seqlens on another device than the tensors
        dev = {n: (t.cuda() if n not in ("state_slot",) else t) for n, t in ok.items()}
        with pytest.raises(RuntimeError, match="state_slot must be"):
            call(**dev)
    assert all(hasattr(torch.ops.rwkv6, n) for n in ("forward_varlen_bf16", "forward_varlen_fp16", "forward_varlen_fp32"))
