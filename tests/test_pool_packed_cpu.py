"""CPU tier of the packed pooling operator (include/wkv6_amd.h: wkv6_pool_packed_forward / _backward): the eager restatement
callers.pooling_packed against the fp64 statement of the header (tests/pool_common.py) under the suite's parity contract, the clamping rule,
the NaN and never-read rules, every refusal of the two C calls with its code and in its order (dummy pointers, nothing is launched), and
what mix_op.pool_packed refuses before it calls the library.

Contract: bf16 outputs under oracle.contract.bf16_ok on the sequences with a_s >= 1 (a_s == 0 is a NaN row by definition), "lasttoken"
bit-exact.  The dense callers.pooling is a second witness where it can be one: it meets the same contract for "weightedmean" and
"lasttoken"; its "avg" multiplies and sums in bf16 (two roundings) and is compared to within one bf16 ulp only."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle.contract import bf16_ok
from pool_common import KINDS, LENS, WIDTHS, cu_of, f64, pool_grad_ref, pool_ref, problem, spans
from rwkv_lm_ext_amd import callers

EINVAL, ENULL, EUNSUPPORTED = -1, -2, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows_with_a_sum(cu, actual, total, kind):
    return [s for s, (_, n, a) in enumerate(spans(cu, actual, total)) if n > 0 and (a >= 1 or kind == "lasttoken")]


def check_forward(out, x, cu, actual, kind):
    """out (bf16 [n_seq,C]) against fp64 under the contract; NaN rows and zero rows where the header says so."""
    ref = pool_ref(f64(x), cu.numpy(), None if actual is None else actual.numpy(), kind)
    got = f64(out)
    assert out.dtype == x.dtype if kind == "lasttoken" else out.dtype == torch.bfloat16
    for s, (_, n, a) in enumerate(spans(cu.numpy(), None if actual is None else actual.numpy(), x.shape[0])):
        if n == 0:
            assert (got[s] == 0).all() and not np.signbit(got[s]).any(), s
        elif a == 0 and kind != "lasttoken":
            assert np.isnan(got[s]).all(), s
    keep = rows_with_a_sum(cu.numpy(), None if actual is None else actual.numpy(), x.shape[0], kind)
    if kind == "lasttoken":
        assert np.array_equal(got[keep], ref[keep])
    else:
        ok, msg = bf16_ok(got[keep], ref[keep])
        assert ok, (kind, msg)


def check_backward(gx, gout, cu, actual, kind):
    total = gx.shape[0]
    ref, hit = pool_grad_ref(f64(gout), cu.numpy(), None if actual is None else actual.numpy(), kind, total)
    got = f64(gx)
    assert (got[~hit] == 0).all()
    nan = np.isnan(ref).any(1)
    assert np.isnan(got[nan]).all()
    sel = hit & ~nan
    if kind == "lasttoken":
        assert np.array_equal(got[sel], ref[sel])
    else:
        ok, msg = bf16_ok(got[sel], ref[sel])
        assert ok, (kind, msg)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", WIDTHS)
def test_eager_forward_and_gradient_against_fp64(C, kind):
    x, gout, cu = problem(C, seed=3 + C)
    actual = torch.tensor([0, 1, 40, 63, 64, 77, 0, 3, 299], dtype=torch.int32)
    for act in (None, actual):
        xr = x.clone().requires_grad_()
        out = callers.pooling_packed(xr, cu, act, kind)
        assert tuple(out.shape) == (len(LENS), C)
        check_forward(out.detach(), x, cu, act, kind)
        finite = rows_with_a_sum(cu.numpy(), None if act is None else act.numpy(), x.shape[0], kind)
        out[finite].backward(gout[finite].to(out.dtype))             # a NaN row's own gradient is NaN whatever flows into it
        g = gout.clone()
        g[[s for s in range(len(LENS)) if s not in finite]] = 0
        check_backward(xr.grad, g, cu, act, kind)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_eager_serves_fp32_and_fp16_and_the_3d_form(dtype):
    x, _, cu = problem(64, seed=9, dtype=dtype)
    for kind in KINDS:
        check_forward(callers.pooling_packed(x.unsqueeze(0), cu, None, kind), x, cu, None, kind)
        assert torch.equal(callers.pooling_packed(x, cu, None, kind, kernels=False)[1:], callers.pooling_packed(x.unsqueeze(0), cu, None, kind)[1:])


@pytest.mark.parametrize("kind", KINDS)
def test_the_clamping_rule(kind):
    """actual_len negative -> 0, equal to len_s (or beyond) -> len_s - 1, None -> len_s - 1; a cu_seqlens entry past total_T is clamped."""
    lens = [5, 9, 4, 6]
    x, _, cu = problem(64, seed=21, lens=lens)
    for actual in ([-1, 9, 2, 1 << 30], [4, -(1 << 31), 4, 6], [3, 8, 100, 5]):
        act = torch.tensor(actual, dtype=torch.int32)
        out = callers.pooling_packed(x, cu, act, kind)
        check_forward(out, x, cu, act, kind)
        clamped = torch.tensor([min(max(a, 0), n - 1) for a, n in zip(actual, lens)], dtype=torch.int32)
        assert torch.equal(out.isnan(), callers.pooling_packed(x, cu, clamped, kind).isnan())
        assert torch.equal(out.nan_to_num(7.0), callers.pooling_packed(x, cu, clamped, kind).nan_to_num(7.0))
    full = torch.tensor([n for n in lens], dtype=torch.int32)                # == len_s: the last token, as None
    assert torch.equal(callers.pooling_packed(x, cu, full, kind), callers.pooling_packed(x, cu, None, kind))
    over = cu.clone()
    over[-1] = x.shape[0] + 50
    assert torch.equal(callers.pooling_packed(x, over, None, kind), callers.pooling_packed(x, cu, None, kind))


def test_a_zero_gives_nan_for_the_means_and_leaves_the_neighbours_finite():
    lens = [6, 1, 8, 5]
    x, _, cu = problem(64, seed=22, lens=lens)
    act = torch.tensor([5, 0, 0, 4], dtype=torch.int32)
    for kind in ("weightedmean", "avg"):
        out = callers.pooling_packed(x, cu, act, kind)
        assert out[1].isnan().all() and out[2].isnan().all()
        assert out[0].isfinite().all() and out[3].isfinite().all()
        check_forward(out, x, cu, act, kind)
    last = callers.pooling_packed(x, cu, act, "lasttoken")
    assert torch.equal(last[1], x[6]) and torch.equal(last[2], x[7])


@pytest.mark.parametrize("kind", KINDS)
def test_nan_in_gap_rows_and_past_a_reaches_nothing(kind):
    lens = [7, 0, 12, 3]
    front, back = 3, 5
    x, gout, cu = problem(64, seed=23, lens=lens, front=front, back=back)
    act = torch.tensor([4, 0, 7, 2], dtype=torch.int32)
    clean = callers.pooling_packed(x, cu, act, kind)
    poisoned = x.clone()
    poisoned[:front] = float("nan")
    poisoned[-back:] = float("nan")
    for (start, n, a) in spans(cu.numpy(), act.numpy(), x.shape[0]):
        poisoned[start + a + 1:start + n] = float("nan")                      # past a_s (for "avg" row a_s itself is not summed either)
    xr = poisoned.clone().requires_grad_()
    out = callers.pooling_packed(xr, cu, act, kind)
    assert torch.equal(out, clean) and out.isfinite().all()
    out.backward(gout.to(out.dtype))
    gx, hit = pool_grad_ref(f64(gout), cu.numpy(), act.numpy(), kind, x.shape[0])
    assert xr.grad.isfinite().all() and (f64(xr.grad)[~hit] == 0).all()
    check_backward(xr.grad, gout, cu, act, kind)


def test_against_the_dense_function():
    """the padded rows through callers.pooling: the contract for weightedmean, bit-exact for lasttoken, one bf16 ulp for avg"""
    lens = [n for n in LENS if n >= 2]
    x, _, cu = problem(64, seed=24, lens=lens)
    T = max(lens)
    padded = torch.zeros(len(lens), T, 64, dtype=x.dtype)
    for s, n in enumerate(lens):
        padded[s, :n] = x[cu[s]:cu[s + 1]]
    a = torch.tensor([n - 1 for n in lens])
    for kind in KINDS:
        dense, packed = callers.pooling(padded, a, kind), callers.pooling_packed(x, cu, a.int(), kind)
        if kind == "lasttoken":
            assert torch.equal(dense, packed)
        elif kind == "weightedmean":
            ok, msg = bf16_ok(f64(dense), pool_ref(f64(x), cu.numpy(), a.numpy(), kind))
            assert ok, msg
        else:
            ulp = packed.float().abs().clamp_min(1e-30).log2().floor().exp2() * 2.0 ** -7
            assert ((dense.float() - packed.float()).abs() <= ulp).all()


# ---- the C ABI: dummy pointers (never dereferenced: every call below is refused before a launch)
X, OUT, P = 1 << 40, 2 << 40, 64


@pytest.fixture(scope="module")
def lib():
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


def args(total_T=100, n_seq=3, C=64, kind=0, cu=P, actual=P, x=X, out=OUT):
    return (total_T, n_seq, C, kind, cu, actual, x, out, None)


def test_symbols_and_signatures(lib):
    from rwkv_lm_ext_amd import _lib
    header = open(os.path.join(ROOT, "include", "wkv6_amd.h")).read()
    I, L, VP = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    common = ["long total_T", "int n_seq", "int C", "int kind", "const int* cu_seqlens", "const int* actual_len"]
    want = {"wkv6_pool_packed_forward": common + ["const void* x", "void* out", "void* stream"],
            "wkv6_pool_packed_backward": common + ["const void* gout", "void* gx", "void* stream"]}
    for name, params in want.items():
        res, table = _lib.SIGNATURES[name]
        assert res is I and list(table) == [L, I, I, I, VP, VP, VP, VP, VP]
        assert getattr(lib, name).restype is I and list(getattr(lib, name).argtypes) == list(table)
        decl = re.search("int " + name + r"\(([^;]*)\);", header).group(1)
        assert [" ".join(p.split()) for p in decl.split(",")] == params
    kinds = re.search(r"enum \{ WKV6_POOL_WEIGHTEDMEAN = (\d), WKV6_POOL_LASTTOKEN = (\d), WKV6_POOL_AVG = (\d) \};", header).groups()
    assert dict(zip(("weightedmean", "lasttoken", "avg"), map(int, kinds))) == _lib.POOL_KINDS


@pytest.mark.parametrize("name", ["wkv6_pool_packed_forward", "wkv6_pool_packed_backward"])
def test_refusals_and_their_order(lib, name):
    fn = getattr(lib, name)
    # (1) shapes and the kind, in front of everything
    for kw in ({"total_T": 0}, {"total_T": -5}, {"n_seq": 0}, {"n_seq": -1}, {"C": 0}, {"C": -8}, {"C": 4}, {"C": 12}, {"C": 63}, {"C": 2052},
               {"kind": 3}, {"kind": -1}, {"kind": 1 << 20}):
        assert fn(*args(**kw)) == EINVAL, kw
        assert fn(*args(**dict(kw, x=None))) == EINVAL, kw
        if "total_T" not in kw:
            assert fn(*args(**dict(kw, total_T=1 << 31))) == EINVAL, kw
    # (2) what int32 arrays and a 32-bit grid cannot hold
    assert fn(*args(total_T=1 << 31)) == EUNSUPPORTED
    assert fn(*args(total_T=1 << 31, cu=None)) == EUNSUPPORTED
    assert fn(*args(total_T=(1 << 31) - 1, cu=None)) == ENULL                 # INT_MAX itself goes on to the next check
    assert fn(*args(n_seq=(1 << 31) - 1, C=1024, out=None)) == EUNSUPPORTED    # n_seq * ceil(C / 512)
    assert fn(*args(n_seq=(1 << 31) - 1, C=512, out=None)) == ENULL
    # (3) NULL pointers (actual_len may be NULL), in front of alignment
    for p in ("cu", "x", "out"):
        assert fn(*args(**{p: None})) == ENULL, p
    assert fn(*args(x=None, out=OUT + 2)) == ENULL
    assert fn(*args(cu=None, actual=P + 1)) == ENULL
    assert fn(*args(actual=None, x=X + 8)) == EINVAL                           # a NULL actual_len is accepted: the next check speaks
    # (4) alignment: 16 bytes for the bf16 tensors, 4 for the int arrays
    for p, base in (("x", X), ("out", OUT)):
        for off in (1, 2, 4, 8, 12):
            assert fn(*args(**{p: base + off})) == EINVAL, (p, off)
    for p in ("cu", "actual"):
        for off in (1, 2, 3):
            assert fn(*args(**{p: P + off})) == EINVAL, (p, off)


def test_pool_packed_refuses_before_calling_the_library(monkeypatch):
    from rwkv_lm_ext_amd import _lib, mix_op

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", no_library)
    bf, i32 = torch.bfloat16, torch.int32
    good = dict(x=torch.zeros(1, 10, 64, dtype=bf), cu=torch.tensor([0, 4, 10], dtype=i32), actual=torch.tensor([3, 5], dtype=i32))

    def call(kind="weightedmean", **o):
        a = dict(good, **o)
        return mix_op.pool_packed(a["x"], a["cu"], a["actual"], kind)

    with pytest.raises(RuntimeError, match="must be on the GPU"):            # everything else is right: no CPU path
        call()
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        call(x=good["x"][0], actual=None)
    for bad in (good["x"].float(), good["x"].half(), torch.zeros(640, dtype=bf), None):
        with pytest.raises(RuntimeError, match="x must be"):
            call(x=bad)
    with pytest.raises(RuntimeError, match="a packed batch is"):
        call(x=torch.zeros(2, 10, 64, dtype=bf))
    for bad in (torch.zeros(1, 10, 12, dtype=bf), torch.zeros(1, 10, 4, dtype=bf), torch.zeros(1, 0, 64, dtype=bf)):
        with pytest.raises(RuntimeError, match="multiple of 8"):
            call(x=bad)
    with pytest.raises(RuntimeError, match="kind must be one of"):
        call(kind="max")
    for bad in (good["cu"].long(), torch.zeros(1, dtype=i32), torch.zeros(6, dtype=i32)[::2], [0, 4, 10], None):
        with pytest.raises(RuntimeError, match="cu_seqlens must be"):
            call(cu=bad)
    for bad in (good["actual"].long(), torch.zeros(3, dtype=i32), torch.zeros(4, dtype=i32)[::2], [3, 5]):
        with pytest.raises(RuntimeError, match="actual_len must be"):
            call(actual=bad)
    # callers.pooling_packed: kernels=True asks for the kernels and gets their refusal; None and False take the eager path on the CPU
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        callers.pooling_packed(good["x"], good["cu"], good["actual"], kernels=True)
    assert torch.equal(callers.pooling_packed(good["x"], good["cu"], good["actual"]),
                       callers.pooling_packed(good["x"], good["cu"], good["actual"], kernels=False))
    with pytest.raises(ValueError):
        callers.pooling_packed(good["x"], good["cu"], good["actual"], "max")
