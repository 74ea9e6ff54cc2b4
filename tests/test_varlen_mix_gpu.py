"""The token-shift / lerp kernels on a packed variable-length batch (wkv6_ddlerp_varlen_forward / _backward, mix_op.ddlerp(cu_seqlens=)):
the token in front of the first token of sequence s is shifted0[s] (or zero), never the last token of sequence s - 1.

Reference: the formulas in fp64 torch on the same bf16 inputs, computed per sequence (every sequence's first token takes its own front
row, nothing is handed across a boundary).  Metric and bounds are those of tests/test_mix_kernels_gpu.py for the dense kernels, imported
from it: outputs within 1.01 bf16 ulp of RNE_bf16(fp64) (rel-rms <= 2e-3), dx within 1.5, the fp32 partial rows of dmaa summed in fp64
within K_PART 2^-24 sum|terms| per channel; outputs are poisoned with NaN first and none may be left; calls repeat bit for bit."""
import pytest
import torch

from test_mix_kernels_gpu import INST, check_detectable, check_partials, close, no_nan, poisoned, ptr, rnd, same, stream
from varlen_common import EDGE_LENS, bench_lens, cu_of

pytestmark = pytest.mark.gpu
bf, f32, f64 = torch.bfloat16, torch.float32, torch.float64


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


def packed_ref(x, maa, m, s0, lens, dout):
    """fp64, sequence by sequence: out [NS,T,C], dx [T,C], dm (= the dmaa terms) [NS,T,C], d shifted0 [n_seq,C]."""
    T, C = x.shape
    NS = maa.shape[0]
    xd = x.double()
    out = torch.empty(NS, T, C, dtype=f64, device="cuda")
    dx = torch.empty(T, C, dtype=f64, device="cuda")
    dm = torch.empty(NS, T, C, dtype=f64, device="cuda")
    ds0 = torch.zeros(len(lens), C, dtype=f64, device="cuda")
    t0 = 0
    for s, n in enumerate(lens):
        if n == 0:
            continue
        sl = slice(t0, t0 + n)
        front = torch.zeros(1, C, dtype=f64, device="cuda") if s0 is None else s0[s:s + 1].double()
        xs = xd[sl]
        xx = torch.cat([front, xs[:-1]], 0) - xs
        c = maa.double().view(NS, 1, C) + (0.0 if m is None else m[:, sl].double())
        out[:, sl] = xs + xx * c
        d = dout[:, sl].double()
        g = (d * (1.0 - c)).sum(0)
        hand = (d * c).sum(0)                        # what token t hands to token t - 1 of the SAME sequence
        g[:-1] += hand[1:]
        ds0[s] = hand[0]
        dx[sl] = g
        dm[:, sl] = d * xx
        t0 += n
    assert t0 == T
    return out, dx, dm, ds0


def fwd_abi(lib, x, maa, m, s0, cu):
    T, C = x.shape
    out = poisoned(maa.shape[0], T, C)
    rc = lib.wkv6_ddlerp_varlen_forward(T, cu.numel() - 1, C, maa.shape[0], ptr(cu), ptr(x), ptr(s0), ptr(m), ptr(maa), ptr(out), stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out


def bwd_abi(lib, x, maa, m, s0, cu, dout, nparts):
    T, C = x.shape
    NS = maa.shape[0]
    dx, dm, part = poisoned(T, C), (None if m is None else poisoned(NS, T, C)), poisoned(nparts, NS, C, dtype=f32)
    rc = lib.wkv6_ddlerp_varlen_backward(T, cu.numel() - 1, C, NS, ptr(cu), ptr(x), ptr(s0), ptr(m), ptr(maa), ptr(dout), ptr(dx),
                                         ptr(dm), ptr(part), nparts, stream())
    assert rc == 0
    torch.cuda.synchronize()
    return dx, dm, part


def inputs(T, n_seq, C, NS, has_m, with_s0, seed):
    x = rnd(T, C, seed=seed)
    maa = rnd(NS, C, scale=0.5, seed=seed + 1)
    m = rnd(NS, T, C, scale=0.3, seed=seed + 2) if has_m else None
    s0 = rnd(n_seq, C, seed=seed + 3) if with_s0 else None
    dout = rnd(NS, T, C, seed=seed + 4)
    return x, maa, m, s0, dout


def run_case(lib, lens, C, ns, has_m, with_s0, nparts_list, what):
    T = sum(lens)
    cu = torch.from_numpy(cu_of(lens)).cuda()
    x, maa, m, s0, dout = inputs(T, len(lens), C, ns, has_m, with_s0, seed=10 * ns + has_m)
    out_ref, dx_ref, dm_ref, ds0_ref = packed_ref(x, maa, m, s0, lens, dout)
    terms = dm_ref.permute(1, 0, 2).contiguous()                        # [rows, NS, C]
    out = fwd_abi(lib, x, maa, m, s0, cu)
    no_nan(what + " out", out)
    assert same(out, fwd_abi(lib, x, maa, m, s0, cu)), what + ": forward not repeatable"
    close(out, out_ref, what + " out")
    first = None
    for nparts in nparts_list:
        tag = f"{what} nparts={nparts}"
        dx, dm, part = bwd_abi(lib, x, maa, m, s0, cu, dout, nparts)
        no_nan(tag, dx, dm, part)
        dx2, dm2, part2 = bwd_abi(lib, x, maa, m, s0, cu, dout, nparts)
        assert same(dx, dx2) and same(part, part2) and (m is None or same(dm, dm2)), tag + ": backward not repeatable"
        close(dx, dx_ref, tag + " dx", ulps=1.5)
        if m is not None:
            close(dm, dm_ref, tag + " dm")
        per = -(-T // nparts)
        bound = check_partials(part, terms, tag + " dmaa", [p for p in range(nparts) if p * per >= T])
        if first is None:
            first = (dx, dm)
        else:   # every row's dx / dm is formed by the same operations whichever workgroup serves it
            assert same(dx, first[0]) and (m is None or same(dm, first[1])), tag + ": depends on the run split"
    check_detectable(terms, bound, what)
    # the autograd wrapper: x [1,T,C]; d shifted0 of an empty sequence is 0
    from rwkv_lm_ext_amd import mix_op
    xl, maal = x.view(1, T, C).clone().requires_grad_(True), maa.clone().requires_grad_(True)
    ml = None if m is None else m.view(ns, 1, T, C).clone().requires_grad_(True)
    sl = None if s0 is None else s0.clone().requires_grad_(True)
    o = mix_op.ddlerp(xl, maal, ml, sl, cu_seqlens=cu)
    assert same(o.view(ns, T, C), out)
    o.backward(dout.view(ns, 1, T, C))
    torch.cuda.synchronize()
    close(xl.grad.view(T, C), dx_ref, what + " autograd dx", ulps=1.5)
    close(maal.grad, terms.sum(0), what + " autograd dmaa")
    if sl is not None:
        close(sl.grad, ds0_ref, what + " autograd dshifted0", ulps=1.5)
        assert not bool(sl.grad[[i for i, n in enumerate(lens) if n == 0]].any())


IDS = [f"NS{n}{'m' if h else ''}" for n, h in INST]


@pytest.mark.parametrize("with_s0", [False, True], ids=["zero-front", "shifted0"])
@pytest.mark.parametrize("ns,has_m", INST, ids=IDS)
def test_ddlerp_varlen_edge_lengths(lib, ns, has_m, with_s0):
    assert EDGE_LENS == [1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 0, 330]
    T = sum(EDGE_LENS)
    run_case(lib, EDGE_LENS, 256, ns, has_m, with_s0, [1, 7, 1024, T, T + 5], f"varlen edges NS={ns} m={has_m} s0={with_s0}")


@pytest.mark.parametrize("with_s0", [False, True], ids=["zero-front", "shifted0"])
@pytest.mark.parametrize("ns,has_m", INST, ids=IDS)
def test_ddlerp_varlen_training_rows(lib, ns, has_m, with_s0):
    """total_T >= 2^17 rows of C = 2048 channels, lengths as bench.py draws them (plus empty sequences at both ends and in the middle)."""
    lens = bench_lens(480, device="cuda")
    lens = [0] + lens[:200] + [0, 0] + lens[200:] + [0]
    assert sum(lens) >= 1 << 17
    run_case(lib, lens, 2048, ns, has_m, with_s0, [1024], f"varlen training rows NS={ns} m={has_m} s0={with_s0}")


def test_one_sequence_is_the_dense_kernel(lib):
    """cu_seqlens = [0, T]: bit for bit the dense kernels on [1,T,C]."""
    T, C = 1000, 512
    x, maa, m, s0, dout = inputs(T, 1, C, 5, True, True, seed=77)
    cu = torch.tensor([0, T], dtype=torch.int32, device="cuda")
    out = fwd_abi(lib, x, maa, m, s0, cu)
    dense = poisoned(5, T, C)
    assert lib.wkv6_ddlerp_forward(1, T, C, 5, ptr(x), ptr(s0), ptr(m), ptr(maa), ptr(dense), stream()) == 0
    dx, dm, part = bwd_abi(lib, x, maa, m, s0, cu, dout, 64)
    dx2, dm2, part2 = poisoned(T, C), poisoned(5, T, C), poisoned(64, 5, C, dtype=f32)
    assert lib.wkv6_ddlerp_backward(1, T, C, 5, ptr(x), ptr(s0), ptr(m), ptr(maa), ptr(dout), ptr(dx2), ptr(dm2), ptr(part2), 64,
                                    stream()) == 0
    torch.cuda.synchronize()
    assert same(out, dense) and same(dx, dx2) and same(dm, dm2) and same(part, part2)
