"""The packed variable-length ("varlen") WKV6 operator on the GPU: wkv6_op.forward_varlen_ex / backward_varlen_ex, wkv.WKV_6_VARLEN /
WKV_6STATE_VARLEN and callers.Tmix_x060(cu_seqlens=...).

Expectation of a packed call: the CPU oracle on every sequence alone (B = 1, T = len_s), concatenated (varlen_common.oracle_packed).
Tolerances are the suite's (oracle/contract.py): fp32 max_norm_err <= F32_TOL; bf16: rel-rms <= 1e-3, <= 2 ulp, >= 95 % correctly
rounded; gw with floor 0.1 and >= 90 % (its last bit depends on the order of a suffix sum: tests/test_bwd_unsplit_gpu.py).  Per-sequence
gu / gs are fp32 partials (WKV6_PARTIALS_F32): max_norm_err <= 1e-3 on the bf16 path as tests/test_bench_shapes_gpu.py holds them.

Rows are independent workgroups that run the dense kernels' arithmetic, so beyond parity every tensor of a packed bf16 call equals BIT FOR
BIT the dense call on each sequence alone; neighbours filled with NaN change nothing; checkpoints kept from the forward give the backward
that rebuilds them; two calls agree bit for bit; and a captured graph replays the eager result."""
import numpy as np
import pytest
import torch

from conftest import max_norm_err
from oracle.contract import F32_TOL, bf16_report
from varlen_common import EDGE_LENS, LONG_LENS, bench_lens, cu_of, oracle_packed

pytestmark = pytest.mark.gpu
bf, f32 = torch.bfloat16, torch.float32
GRADS = ("gr", "gk", "gv", "gw")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "the gpu suite needs a GPU"
    from rwkv_lm_ext_amd import wkv6_op
    return wkv6_op


def host(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def check_bf16(out, ref, what):
    gw = what.split()[-1].startswith("gw")
    rms, off, ulps = bf16_report(out, ref, floor=0.1 if gw else 1e-3)
    print(f"{what}: bf16 rel-rms {rms:.2e}, max {ulps:.2f} ulp, {off * 100:.1f}% not correctly rounded")
    assert rms <= 1e-3 and ulps <= 2.0 and off <= 1 - (0.90 if gw else 0.95), what


def check_f32(out, ref, what):
    e = max_norm_err(out, ref)
    print(f"{what}: fp32 max_norm_err {e:.2e}")
    assert e <= F32_TOL, (what, e)


def make(lens, H, io, seed=0, ramp=False):
    """Packed inputs in the I/O type: r, k, v, raw w, u, gy (+ cu_seqlens on the device)."""
    total, C = sum(lens), 64 * H
    g = torch.Generator(device="cuda").manual_seed(seed)
    r, k, v = (torch.randn(total, C, device="cuda", generator=g).mul_(0.5).to(io) for _ in range(3))
    if ramp:    # bench.py's init-ramp decays
        base = torch.tensor([-6 + 5 * (n / (C - 1)) ** (0.7 + 1.3 * 0.5) for n in range(C)], device="cuda").view(1, C)
        w = (base + 0.1 * torch.randn(total, C, device="cuda", generator=g)).to(io)
    else:
        w = (-1 + 0.5 * torch.randn(total, C, device="cuda", generator=g)).to(io)
    u = (torch.randn(H, 64, device="cuda", generator=g) * 0.3).to(io)
    gy = torch.randn(total, C, device="cuda", generator=g).to(io)
    cu = torch.from_numpy(cu_of(lens)).cuda()
    return dict(r=r, k=k, v=v, w=w, u=u, gy=gy, cu=cu, lens=list(lens), H=H, max_seqlen=max(max(lens), 1))


def run(ops, d, ew=False, algo=None, s0=None, want_state=False, keep=True):
    """Forward + backward of the packed op.  ew: the decay goes in as fp32 ew = -exp(w).  keep: the forward's workspace carries the
    checkpoints to the backward."""
    w = (-torch.exp(d["w"].float())).contiguous() if ew else d["w"]
    H, n_seq = d["H"], len(d["lens"])
    total, C = d["r"].shape
    ws = ops.new_varlen_workspace(total, n_seq, C, H, "cuda") if keep else None
    s_out = torch.full((n_seq, H, 64, 64), float("nan"), device="cuda", dtype=d["r"].dtype) if want_state else None
    y = ops.forward_varlen_ex(d["r"], d["k"], d["v"], w, d["u"], H, d["cu"], d["max_seqlen"], s0=s0, s_out=s_out, w_is_ew=ew,
                              algo=algo, ws=ws)
    g = ops.backward_varlen_ex(d["r"], d["k"], d["v"], w, d["u"], d["gy"], H, d["cu"], d["max_seqlen"], s0=s0, w_is_ew=ew,
                               want_gs=s0 is not None, algo=algo, ws=ws, ckpt_valid=keep)
    torch.cuda.synchronize()
    out = dict(y=y, gr=g[0], gk=g[1], gv=g[2], gw=g[3], gu=g[4])
    if s0 is not None:
        out["gs"] = g[5]
    if want_state:
        out["s_out"] = s_out
    return out


def oracle_of(oracle, d, s0=None, heads=None):
    f = lambda t: host(t)
    return oracle_packed(oracle, f(d["r"]), f(d["k"]), f(d["v"]), f(d["w"]), f(d["u"]), f(d["gy"]), d["lens"],
                         s0=None if s0 is None else f(s0), heads=heads)


def compare(got, want, io, what, cols=slice(None), rows=slice(None), seqs=slice(None)):
    for n in ("y",) + GRADS:
        a = host(got[n])[rows, cols]
        (check_bf16 if io == bf else check_f32)(a, want[n][rows], f"{what} {n}")
    gu = host(got["gu"])[seqs, cols]
    e = max_norm_err(gu, want["gu"][seqs])
    print(f"{what} gu (fp32 per-sequence partials): {e:.2e}")
    assert e <= (1e-3 if io == bf else F32_TOL), (what, e)


CASES = {"edges": EDGE_LENS, "long": LONG_LENS}
assert EDGE_LENS == [1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 0, 330] and sorted(LONG_LENS) == [1] * 15 + [4096]


@pytest.mark.parametrize("ew", [False, True], ids=["w_raw", "ew_f32"])
@pytest.mark.parametrize("path", ["chunk_bf16", "scan_f32"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_oracle_parity(ops, oracle, case, path, ew):
    io = bf if path == "chunk_bf16" else f32
    # (the long case takes bench.py's init-ramp decays, as the suite's other T = 4096 parity test does -- tests/test_bench_shapes_gpu.py:
    # synth.  With the N(-1, 0.5) decays of the short cases the chunked gw of the 4096-token row measured 3.75 ulp against the oracle
    # (rel-rms 9.1e-4): the dense kernel's own figure on that row -- the packed row is bit-identical to it, see
    # test_same_arithmetic_as_the_dense_op_on_each_sequence_alone -- not an effect of packing.)
    d = make(CASES[case], 2, io, seed=3, ramp=case == "long")
    got = run(ops, d, ew=ew)
    compare(got, oracle_of(oracle, d), io, f"{case} {path} {'ew' if ew else 'raw'}")
    # the scan kernels on bf16 I/O serve packed rows too (WKV6_ALGO_SCAN)
    if path == "chunk_bf16" and not ew:
        compare(run(ops, d, algo="scan"), oracle_of(oracle, d), bf, f"{case} scan_bf16 raw")


@pytest.mark.parametrize("ew", [False, True], ids=["w_raw", "ew_f32"])
@pytest.mark.parametrize("path", ["chunk_bf16", "scan_f32"])
def test_oracle_parity_at_the_bench_shape(ops, oracle, path, ew):
    """48 lengths drawn as bench.py's ragged config draws them, H = 32, C = 2048: five (sequence, head) slices against the oracle."""
    io = bf if path == "chunk_bf16" else f32
    lens = bench_lens(48, device="cuda")
    assert len(lens) == 48 and 64 <= min(lens) and max(lens) <= 512
    d = make(lens, 32, io, seed=4, ramp=True)
    got = run(ops, d, ew=ew)
    cu = cu_of(lens)
    longest, shortest = int(np.argmax(lens)), int(np.argmin(lens))
    for s, h in ((0, 0), (47, 31), (longest, 16), (shortest, 17), (23, 9)):
        rows, cols = slice(int(cu[s]), int(cu[s + 1])), slice(64 * h, 64 * h + 64)
        one = {n: (t[rows, cols].contiguous() if n in ("r", "k", "v", "w", "gy") else t) for n, t in d.items()}
        one["u"], one["lens"] = d["u"][h:h + 1], [lens[s]]
        want = oracle_of(oracle, one)
        sub = {n: got[n][rows] for n in ("y",) + GRADS}
        sub["gu"] = got["gu"][s:s + 1]
        compare(sub, want, io, f"bench ({s},{h}) {path} {'ew' if ew else 'raw'}", cols=cols)


@pytest.mark.parametrize("path", ["chunk_bf16", "scan_f32"])
def test_per_sequence_states(ops, oracle, path):
    """WKV6_S0_PER_BATCH: s0, s_out, gs are [n_seq,H,N,N]; an empty sequence hands its s0 on and has zero gu / gs."""
    io = bf if path == "chunk_bf16" else f32
    d = make(EDGE_LENS, 2, io, seed=5)
    g = torch.Generator(device="cuda").manual_seed(6)
    s0 = (torch.randn(len(EDGE_LENS), 2, 64, 64, device="cuda", generator=g) * 0.3).to(io)
    got = run(ops, d, s0=s0, want_state=True)
    want = oracle_of(oracle, d, s0=s0)
    compare(got, want, io, f"per-sequence state {path}")
    for n in ("s_out", "gs"):
        a = host(got[n])
        if io == bf and n == "s_out":
            check_bf16(a, want[n], f"per-sequence state {path} {n}")
        else:   # gs: fp32 partials
            e = max_norm_err(a, want[n])
            print(f"per-sequence state {path} {n}: {e:.2e}")
            assert e <= (1e-3 if io == bf else F32_TOL), (n, e)
    empty = EDGE_LENS.index(0)
    assert same(got["s_out"][empty], s0[empty]) and not bool(got["gu"][empty].any()) and not bool(got["gs"][empty].any())
    # a shared [H,N,N] state: every sequence starts from it
    shared = s0[0].contiguous()
    got2 = run(ops, d, s0=shared, want_state=True)
    want2 = oracle_of(oracle, d, s0=shared)
    compare(got2, want2, io, f"shared state {path}")
    e = max_norm_err(host(got2["gs"]).sum(0), want2["gs"].sum(0))
    assert e <= (1e-3 if io == bf else F32_TOL), e


@pytest.mark.parametrize("ew", [False, True], ids=["w_raw", "ew_f32"])
@pytest.mark.parametrize("case", ["edges", "bench"])
def test_same_arithmetic_as_the_dense_op_on_each_sequence_alone(ops, case, ew):
    """dispatch(split=0, tsplit=0): one workgroup per (batch, head) and one scan level in the dense calls, as every packed row runs."""
    lens = EDGE_LENS if case == "edges" else bench_lens(48, device="cuda")[:12]
    H = 2 if case == "edges" else 32
    d = make(lens, H, bf, seed=7)
    got = run(ops, d, ew=ew, want_state=True)
    got_nockpt = run(ops, d, ew=ew, want_state=True, keep=False)
    cu = cu_of(lens)
    wfull = (-torch.exp(d["w"].float())).contiguous() if ew else d["w"]
    with ops.dispatch(split=0, tsplit=0):
        for s, n in enumerate(lens):
            if n == 0:
                continue
            rows = slice(int(cu[s]), int(cu[s + 1]))
            r, k, v, w, gy = (t[rows].unsqueeze(0).contiguous() for t in (d["r"], d["k"], d["v"], wfull, d["gy"]))
            s_out = torch.empty(1, H, 64, 64, device="cuda", dtype=bf)
            y = ops.forward_ex(r, k, v, w, d["u"], H, s_out=s_out, w_is_ew=ew)
            gr, gk, gv, gw, gu, _ = ops.backward_ex(r, k, v, w, d["u"], gy, H, w_is_ew=ew)
            for res in (got, got_nockpt):
                for name, t in (("y", y), ("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw)):
                    assert same(res[name][rows], t[0]), (case, s, n, name)
                assert same(res["gu"][s], gu[0]), (case, s, n, "gu")
                assert same(res["s_out"][s], s_out[0]), (case, s, n, "s_out")


@pytest.mark.parametrize("ew", [False, True], ids=["w_raw", "ew_f32"])
def test_kept_checkpoints_give_the_self_contained_backward(ops, ew):
    for lens, H in ((EDGE_LENS, 2), (LONG_LENS, 2), (bench_lens(48, device="cuda"), 32)):
        d = make(lens, H, bf, seed=8)
        a, b = run(ops, d, ew=ew, keep=True), run(ops, d, ew=ew, keep=False)
        for n in ("y",) + GRADS + ("gu",):
            assert same(a[n], b[n]), (len(lens), n)


@pytest.mark.parametrize("path", ["chunk_bf16", "scan_f32"])
def test_nan_in_one_sequence_stays_there(ops, path):
    io = bf if path == "chunk_bf16" else f32
    lens = EDGE_LENS
    d = make(lens, 2, io, seed=9)
    clean = run(ops, d)
    cu = cu_of(lens)
    for s in range(len(lens)):
        if lens[s] == 0:
            continue
        rows = slice(int(cu[s]), int(cu[s + 1]))
        p = dict(d)
        for n in ("r", "k", "v", "w", "gy"):
            p[n] = d[n].clone()
            p[n][rows] = float("nan")
        got = run(ops, p)
        keep = torch.ones(sum(lens), dtype=torch.bool, device="cuda")
        keep[rows] = False
        for n in ("y",) + GRADS:
            assert bool(torch.isfinite(got[n][keep]).all()), (s, n)
            assert same(got[n][keep], clean[n][keep]), (s, n)
        others = [i for i in range(len(lens)) if i != s]
        assert bool(torch.isfinite(got["gu"][others]).all()) and same(got["gu"][others], clean["gu"][others]), s


@pytest.mark.parametrize("path", ["chunk_bf16", "scan_f32"])
def test_two_calls_are_bit_identical(ops, path):
    io = bf if path == "chunk_bf16" else f32
    d = make(bench_lens(48, device="cuda"), 4, io, seed=10)
    s0 = (torch.randn(4, 64, 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 0.3).to(io)
    a, b = run(ops, d, s0=s0, want_state=True), run(ops, d, s0=s0, want_state=True)
    for n in a:
        assert same(a[n], b[n]), n


def test_clamping_and_garbage_boundaries_are_safe(ops):
    """Lengths are clamped on the device: max_seqlen cuts a sequence, and a sequence never reaches past total_T."""
    lens = [100, 300, 50]
    d = make(lens, 2, bf, seed=11)
    full = run(ops, d)
    cut = dict(d, max_seqlen=128)
    got = run(ops, cut)                                              # sequence 1 is served for its first 128 tokens only
    assert same(got["y"][:100], full["y"][:100]) and same(got["y"][100:228], full["y"][100:228]) and same(got["y"][400:], full["y"][400:])
    for n in ("y",) + GRADS:                                         # what max_seqlen cut off belongs to no sequence: +0 (include/wkv6_amd.h)
        assert not bool(bits(got[n][228:400]).any()), n
    over = dict(d, cu=torch.tensor([0, 100, 400, 9999], dtype=torch.int32, device="cuda"), max_seqlen=20000)
    got = run(ops, over)                                             # the last boundary lies past total_T: clamped to it
    for n in ("y",) + GRADS:
        assert same(got[n], full[n]), n


def test_forward_and_backward_replay_from_a_graph(ops):
    lens = EDGE_LENS
    d = make(lens, 2, bf, seed=12)
    H, n_seq = 2, len(lens)
    total, C = d["r"].shape
    ws = ops.new_varlen_workspace(total, n_seq, C, H, "cuda")            # caller-owned: nothing is allocated for the kernels while capturing
    ref = run(ops, d)
    y = torch.empty_like(d["r"])
    outs = {}

    def step():
        ops.forward_varlen_ex(d["r"], d["k"], d["v"], d["w"], d["u"], H, d["cu"], d["max_seqlen"], y=y, ws=ws)
        outs["g"] = ops.backward_varlen_ex(d["r"], d["k"], d["v"], d["w"], d["u"], d["gy"], H, d["cu"], d["max_seqlen"], ws=ws,
                                           ckpt_valid=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.current_stream().wait_stream(side)
    captured = outs["g"]
    y.zero_()
    for t in captured[:5]:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same(y, ref["y"])
    for n, t in zip(GRADS + ("gu",), captured):
        assert same(t, ref[n]), n
    # other boundaries in the same buffers: the graph reads cu_seqlens on the device at replay time
    lens2 = [330, 0, 200, 129, 128, 127, 65, 64, 63, 3, 2, 1]
    assert sum(lens2) == total
    d2 = dict(d, lens=lens2, cu=torch.from_numpy(cu_of(lens2)).cuda())
    ref2 = run(ops, d2)
    d["cu"].copy_(d2["cu"])
    graph.replay()
    torch.cuda.synchronize()
    assert same(y, ref2["y"]) and same(captured[3], ref2["gw"])


def test_autograd_functions(ops, oracle):
    """wkv.WKV_6_VARLEN / WKV_6STATE_VARLEN and the torch.ops registration: gu / gs summed over the sequences and rounded once."""
    from rwkv_lm_ext_amd.wkv import RUN_CUDA_RWKV6_VARLEN, RUN_CUDA_RWKV6_STATE_VARLEN
    lens = EDGE_LENS
    d = make(lens, 2, bf, seed=13)
    total, C = d["r"].shape
    want = oracle_of(oracle, d)
    leaves = [d[n].clone().view(1, total, C).requires_grad_(True) for n in ("r", "k", "v", "w")] + [d["u"].clone().requires_grad_(True)]
    y = RUN_CUDA_RWKV6_VARLEN(total, C, 2, *leaves, d["cu"], max(lens))
    assert y.shape == (1, total, C)
    y.backward(d["gy"].view(1, total, C))
    torch.cuda.synchronize()
    check_bf16(host(y[0]), want["y"], "autograd y")
    for t, n in zip(leaves, GRADS):
        check_bf16(host(t.grad[0]), want[n], f"autograd {n}")
    check_bf16(host(leaves[4].grad).reshape(-1), want["gu"].astype(np.float64).sum(0), "autograd gu")
    # learnable shared state
    g = torch.Generator(device="cuda").manual_seed(2)
    s = (torch.randn(2, 64, 64, device="cuda", generator=g) * 0.3).to(bf)
    want = oracle_of(oracle, d, s0=s)
    leaves = [d[n].clone().requires_grad_(True) for n in ("r", "k", "v", "w", "u")] + [s.clone().requires_grad_(True)]
    y = RUN_CUDA_RWKV6_STATE_VARLEN(total, C, 2, *leaves, d["cu"], max(lens))
    y.backward(d["gy"])
    torch.cuda.synchronize()
    check_bf16(host(y), want["y"], "state autograd y")
    check_bf16(host(leaves[5].grad), want["gs"].astype(np.float64).sum(0), "state autograd gs")
    check_bf16(host(leaves[4].grad).reshape(-1), want["gu"].astype(np.float64).sum(0), "state autograd gu")
    # torch.ops.wkv6.forward_varlen writes the caller's buffer
    y2 = torch.empty_like(d["r"])
    torch.ops.wkv6.forward_varlen(total, C, 2, d["r"], d["k"], d["v"], d["w"], d["u"], d["cu"], max(lens), y2)
    assert same(y2, run(ops, d)["y"])


def test_time_mix_module_on_a_packed_batch():
    """Tmix_x060(cu_seqlens=...) on the HIP path (varlen shift kernels + varlen operator) against the same module on the HIP path run
    on every sequence alone.  Bound: OP_TOL of tests/test_callers_gpu.py, which that file holds between its HIP module and the same
    module with the operator swapped."""
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import callers
    from test_callers_gpu import OP_TOL
    from varlen_common import CALLER_LENS
    tm = callers.Tmix_x060(cw.N_EMBD, cw.DIM_ATT)
    tm.load_state_dict(cw.tmix_weights(torch.Generator().manual_seed(11), layer_id=1), strict=True)
    tm = tm.cuda().to(bf)
    cm = callers.CMix_x060(cw.N_EMBD, cw.DIM_FFN)
    cm.load_state_dict(cw.cmix_weights(torch.Generator().manual_seed(12)), strict=True)
    cm = cm.cuda().to(bf)
    lens = CALLER_LENS
    x = torch.randn(1, sum(lens), cw.N_EMBD, generator=torch.Generator().manual_seed(5)).cuda().to(bf)
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(6)).cuda().to(bf)
    cu = torch.from_numpy(cu_of(lens)).cuda()
    for mod, name in ((tm, "time-mix"), (cm, "channel-mix")):
        assert mod._use_fused(x)
        parts, t0 = [], 0
        for n in lens:
            if n:
                parts.append(mod(x[:, t0:t0 + n].contiguous()))
            t0 += n
        want = torch.cat(parts, 1)
        mod.zero_grad()
        want.backward(gy)
        gwant = {n: p.grad.clone() for n, p in mod.named_parameters()}
        got = mod(x, cu_seqlens=cu, max_seqlen=max(lens))
        mod.zero_grad()
        got.backward(gy)
        torch.cuda.synchronize()
        e = max_norm_err(host(got), host(want))
        print(f"{name} packed vs per sequence: {e:.2e}")
        assert e <= OP_TOL, (name, e)
        for n, p in mod.named_parameters():
            eg = max_norm_err(host(p.grad), host(gwant[n]))
            print(f"  grad {n}: {eg:.2e}")
            assert eg <= 2 * OP_TOL, (name, n, eg)       # (3e-2: the bound test_callers_gpu.py holds parameter gradients to with the operator swapped)
        with torch.no_grad():                            # the dense module on the packed tensor leaks across the boundaries
            leak = mod(x)
        first = [int(cu[s]) for s in range(1, len(lens)) if lens[s]]
        assert all(float((leak[0, t].float() - want[0, t].float()).abs().max()) > 0 for t in first)
