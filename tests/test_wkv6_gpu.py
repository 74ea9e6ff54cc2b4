"""GPU parity suite (run with -m gpu on an MI355X).  Every call goes through the C ABI of
librwkv6_amd.so; expected values come from the CPU oracle (oracle/wkv6_oracle.c) and the golden vectors
that oracle/gen_golden.py captured from the reference's own CPU paths.

Tolerances (stated once, used everywhere):
  * fp32 I/O mode:   max|out - ref| / max|ref| <= 1e-5                       (north star: 1e-5 fp32)
  * bf16 I/O mode:   against RNE_bf16(ref): rms(out - RNE(ref)) / rms(ref) <= 1e-3, at most 2 bf16 ulps
                     off anywhere, and >= 95 % of the elements equal to the correctly rounded value
                     (north star: 1e-3 bf16; the reference rounds its fp32 result to bf16 the same way)
"""
import numpy as np
import pytest
import torch

from conftest import bf16_report, load_golden, load_golden_mid, max_norm_err

pytestmark = pytest.mark.gpu

F32_TOL = 1e-5
PART_TOL = 1e-3      # gu / gs per-batch partial sums with bf16 I/O: fp32 (WKV6_PARTIALS_F32) from fp32-accurate kernels
BF16_RMS, BF16_ULPS, BF16_EXACT = 1e-3, 2.0, 0.95


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "the gpu suite needs a GPU"
    from rwkv_lm_ext_amd import wkv6_op
    assert wkv6_op.selftest() == 0, "cross-lane primitive self-test failed"
    return wkv6_op


def dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dtype).contiguous()


def host(t):
    return t.detach().float().cpu().numpy()


def check(out, ref, io, what):
    out = host(out)
    if io == torch.float32:
        # gw is a difference of O(1) suffix sums (a_s - b_s); when the true value is ~0 (T <= 2: exactly 0)
        # the fp32 cancellation residue must be measured against those terms, not against max|ref| = 0
        e = max_norm_err(out, ref, floor=0.1 if what.endswith("gw") else 1e-3)
        assert e <= F32_TOL, f"{what}: fp32 max-normalised error {e:.2e} > {F32_TOL}"
    else:
        rms, off, ulps = bf16_report(out, ref, floor=0.1 if what.split()[-1].startswith("gw") or " gw" in what else 1e-3)
        assert rms <= BF16_RMS and ulps <= BF16_ULPS and off <= 1 - BF16_EXACT, \
            f"{what}: bf16 rel-rms {rms:.2e}, max {ulps:.2f} ulp, {off * 100:.1f}% not correctly rounded"


def rand_inputs(seed, B, T, H, kind="stress"):
    g = torch.Generator().manual_seed(seed)
    C = H * 64
    bf = lambda x: x.to(torch.bfloat16).float().numpy()
    r, k, v = (bf(torch.randn(B, T, C, generator=g) * 0.5) for _ in range(3))
    if kind == "init":
        ramp = torch.tensor([-6 + 5 * (n / (C - 1)) ** (0.7 + 1.3 * 0.5) for n in range(C)])
        w = bf(ramp.view(1, 1, C) + 0.1 * torch.randn(B, T, C, generator=g))
    else:
        w = bf(-1.0 + 0.5 * torch.randn(B, T, C, generator=g))
    u = bf(torch.randn(H, 64, generator=g) * 0.3)
    gy = bf(torch.randn(B, T, C, generator=g))
    return r, k, v, w, u, gy


IOS = [torch.float32, torch.bfloat16]
PLAIN = ["wkv6_init", "wkv6_stress", "wkv6_extreme", "wkv6_T1", "wkv6_T2", "wkv6_T3"]


@pytest.mark.parametrize("io", IOS, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", PLAIN)
def test_golden_plain(ops, name, io):
    g = load_golden(name)
    H = g["u"].shape[0]
    r, k, v, w, u, gy = (dev(g[n], io) for n in ("r", "k", "v", "w", "u", "gy"))
    check(ops.forward_ex(r, k, v, w, u, H), g["y"], io, name + " y")
    gr, gk, gv, gw, gu, _ = ops.backward_ex(r, k, v, w, u, gy, H)
    for n, t in (("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw)):
        check(t, g[n], io, f"{name} {n}")
    # gu: [B,C] per-batch partials, fp32 through the *_ex path (the reference-signature symbols round them to bf16)
    e = max_norm_err(host(gu).sum(0).reshape(H, 64), g["gu"])
    assert e <= (F32_TOL if io == torch.float32 else PART_TOL), f"{name} gu: {e:.2e}"


def test_reference_signature_entry_points(ops):
    """wkv6_cuda.forward/backward with the reference's dtypes: fp32 ew = -exp(w), bf16 everything else
    (cuda/wkv6_op.cpp:8-13), also through torch.ops.wkv6.*"""
    g = load_golden("wkv6_stress")
    B, T, C = g["r"].shape
    H = g["u"].shape[0]
    bf = torch.bfloat16
    r, k, v, u, gy = (dev(g[n], bf) for n in ("r", "k", "v", "u", "gy"))
    ew = (-torch.exp(dev(g["w"], bf).float())).contiguous()          # src/model.py:210
    y = torch.empty(B, T, C, device="cuda", dtype=bf)
    ops.wkv6_cuda.forward(B, T, C, H, r, k, v, ew, u, y)
    check(y, g["y"], bf, "wkv6_cuda.forward")
    y2 = torch.empty_like(y)
    torch.ops.wkv6.forward(B, T, C, H, r, k, v, ew, u, y2)
    assert torch.equal(y, y2)
    gr, gk, gv, gw = (torch.empty_like(y) for _ in range(4))
    gu = torch.empty(B, C, device="cuda", dtype=bf)
    ops.wkv6_cuda.backward(B, T, C, H, r, k, v, ew, u, gy, gr, gk, gv, gw, gu)
    for n, t in (("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw)):
        check(t, g[n], bf, "wkv6_cuda.backward " + n)
    with pytest.raises(RuntimeError):                               # stricter than the reference: shape check
        ops.wkv6_cuda.forward(B, T, C, H + 1, r, k, v, ew, u, y)


@pytest.mark.parametrize("io", IOS, ids=["f32", "bf16"])
def test_golden_state(ops, io):
    g = load_golden("wkv6_state")
    H = g["u"].shape[0]
    r, k, v, w, u, gy, s = (dev(g[n], io) for n in ("r", "k", "v", "w", "u", "gy", "s"))
    check(ops.forward_ex(r, k, v, w, u, H, s0=s), g["y"], io, "state y")
    gr, gk, gv, gw, gu, gs = ops.backward_ex(r, k, v, w, u, gy, H, s0=s, want_gs=True)
    for n, t in (("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw)):
        check(t, g[n], io, "state " + n)
    tol = F32_TOL if io == torch.float32 else PART_TOL
    assert max_norm_err(host(gs).sum(0), g["gs"]) <= tol
    assert max_norm_err(host(gu).sum(0).reshape(H, 64), g["gu"]) <= tol
    if io == torch.bfloat16:     # the reference-signature module object
        B, T, C = g["r"].shape
        y = torch.empty(B, T, C, device="cuda", dtype=io)
        ops.wkv6state_cuda.forward(B, T, C, H, r, k, v, w, u, s, y)
        check(y, g["y"], io, "wkv6state_cuda.forward")


@pytest.mark.parametrize("io", IOS, ids=["f32", "bf16"])
def test_golden_infctx(ops, io):
    g = load_golden("wkv6_infctx")
    B, T, C = g["r"].shape
    H = g["u"].shape[0]
    r, k, v, w, u, gy, s = (dev(g[n], io) for n in ("r", "k", "v", "w", "u", "gy", "s"))
    s_out = torch.empty_like(s)
    check(ops.forward_ex(r, k, v, w, u, H, s0=s, s_out=s_out), g["y"], io, "infctx y")
    check(s_out, g["s_final"], io, "infctx final state")
    gr, gk, gv, gw, gu, gs = ops.backward_ex(r, k, v, w, u, gy, H, s0=s, want_gs=True)
    for n, t in (("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw), ("gs", gs.to(io))):     # gs: fp32 partial, rounded once here
        check(t, g[n], io, "infctx " + n)
    if io == torch.float32:
        # carried state: 3 chunks of 16 with the state handed on == one 48-token call (fp32 carry is exact)
        st = s.clone()
        ys = []
        for c in range(3):
            sl = slice(16 * c, 16 * c + 16)
            ys.append(ops.forward_ex(r[:, sl].contiguous(), k[:, sl].contiguous(), v[:, sl].contiguous(),
                                     w[:, sl].contiguous(), u, H, s0=st, s_out=st))
        check(torch.cat(ys, 1), g["y"], io, "infctx chunked y")
        check(st, g["s_final"], io, "infctx chunked final state")
    else:
        s2 = s.clone()                                              # in-place reference ABI
        y = torch.empty(B, T, C, device="cuda", dtype=io)
        ops.wkv6infctx_cuda.forward(B, T, C, H, r, k, v, w, u, s2, y)
        check(y, g["y"], io, "wkv6infctx_cuda.forward")
        check(s2, g["s_final"], io, "wkv6infctx_cuda.forward state")


@pytest.mark.parametrize("io", IOS, ids=["f32", "bf16"])
def test_golden_bi(ops, io):
    g = load_golden("wkv6_bi")
    H = g["u"].shape[0]
    r, k, v, w, u, gy = (dev(g[n], io) for n in ("r", "k", "v", "w", "u", "gy"))
    mask = torch.from_numpy(g["mask"]).to("cuda", torch.int32)
    y = ops.bi_forward_ex(mask, r, k, v, w, u, H)
    check(y, g["y"], io, "bi y")         # the two halves are summed in fp32 and rounded once
    yh = host(y)
    assert np.all(yh[0, 31:] == 0) and np.all(yh[1, 18:] == 0) and np.all(yh[2, 1:] == 0)   # Q2: zero-filled
    gr, gk, gv, gw, gu = ops.bi_backward_ex(mask, r, k, v, w, u, gy, H)
    for n, t in (("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw)):
        # the adjoints of the two scans are summed in fp32 (side buffers) and rounded once: the suite's bf16 contract
        # (the reference accumulates `_gr[t] += F(gr)` in bf16, cuda/wkv6_bi_cuda.cu:199-200)
        check(t, g[n], io, "bi " + n)
        assert np.all(host(t)[1, 18:] == 0)
    assert max_norm_err(host(gu).sum(0).reshape(H, 64), g["gu"]) <= (F32_TOL if io == torch.float32 else PART_TOL)


@pytest.mark.parametrize("bwd", ["auto", "12k"], ids=["auto", "unsplit"])
@pytest.mark.parametrize("io", IOS, ids=["f32", "bf16"])
def test_golden_medium(ops, io, bwd):
    """Reference-generated vectors at T = 160 (oracle/gen_golden_medium.py): every block, stage, group and checkpoint boundary of
    the chunked kernels meets values that came out of the reference's own recurrence -- plain, per-sample state with gs and
    final state, ragged wkv6_bi; fp32 I/O (scan kernels) and bf16 I/O through either chunked backward."""
    if bwd != "auto" and io == torch.float32:
        pytest.skip("the backward switch only concerns the chunked bf16 kernels")
    # auto: the small grid runs two workgroups per (batch, head); 12k: one workgroup per pair, as at the benched shapes
    with ops.dispatch(split=0 if bwd != "auto" else None):
        tol = F32_TOL if io == torch.float32 else PART_TOL
        g = load_golden_mid("wkv6_mid")
        H = g["u"].shape[0]
        B, T, C = g["r"].shape
        r, k, v, w, u, gy = (dev(g[n], io) for n in ("r", "k", "v", "w", "u", "gy"))
        ck = ops.new_checkpoint(B, T, C, H, "cuda") if io == torch.bfloat16 else None
        check(ops.forward_ex(r, k, v, w, u, H, ckpt=ck), g["y"], io, "mid y")
        gr, gk, gv, gw, gu, _ = ops.backward_ex(r, k, v, w, u, gy, H, ckpt=ck)
        for n, t in (("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw)):
            check(t, g[n], io, "mid " + n)
        assert max_norm_err(host(gu).sum(0).reshape(H, 64), g["gu"]) <= tol
        g = load_golden_mid("wkv6_mid_state")
        H = g["u"].shape[0]
        r, k, v, w, u, gy, s = (dev(g[n], io) for n in ("r", "k", "v", "w", "u", "gy", "s"))
        s_out = torch.empty_like(s)
        check(ops.forward_ex(r, k, v, w, u, H, s0=s, s_out=s_out), g["y"], io, "mid state y")
        check(s_out, g["s_final"], io, "mid final state")
        gr, gk, gv, gw, gu, gs = ops.backward_ex(r, k, v, w, u, gy, H, s0=s, want_gs=True)
        for n, t in (("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw), ("gs", gs.to(io))):
            check(t, g[n], io, "mid state " + n)
        assert max_norm_err(host(gu).sum(0).reshape(H, 64), g["gu"]) <= tol
        g = load_golden_mid("wkv6_mid_bi")
        H = g["u"].shape[0]
        r, k, v, w, u, gy = (dev(g[n], io) for n in ("r", "k", "v", "w", "u", "gy"))
        mask = torch.from_numpy(g["mask"].astype(np.int32)).cuda()
        check(ops.bi_forward_ex(mask, r, k, v, w, u, H), g["y"], io, "mid bi y")
        gr, gk, gv, gw, gu = ops.bi_backward_ex(mask, r, k, v, w, u, gy, H)
        for n, t in (("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw)):
            check(t, g[n], io, "mid bi " + n)
            assert np.all(host(t)[2, 33:] == 0) and np.all(host(t)[1, 97:] == 0)
        assert max_norm_err(host(gu).sum(0).reshape(H, 64), g["gu"]) <= tol


@pytest.mark.parametrize("io", IOS, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 300, 3, "stress"), (1, 1000, 2, "init"), (3, 17, 1, "stress")],
                         ids=["B2T300H3", "B1T1000H2", "B3T17H1"])
def test_random_vs_oracle(ops, oracle, shape, io):
    """Ragged lengths (T not a multiple of the 16-token staging batch), several heads/batches."""
    B, T, H, kind = shape
    r, k, v, w, u, gy = rand_inputs(100 + T, B, T, H, kind)
    d = [dev(x, io) for x in (r, k, v, w, u, gy)]
    check(ops.forward_ex(*d[:5], H), oracle.forward(r, k, v, w, u), io, "y")
    og = oracle.backward(r, k, v, w, u, gy)
    gr, gk, gv, gw, gu, _ = ops.backward_ex(*d[:5], d[5], H)
    for n, t in (("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw)):
        check(t, og[n], io, n)
    assert max_norm_err(host(gu), og["gu_b"]) <= (F32_TOL if io == torch.float32 else PART_TOL)


@pytest.mark.parametrize("T", [15, 16, 17, 31, 32, 33, 49])
def test_exact_kernels_at_staging_batch_boundaries(ops, oracle, T):
    """The exact kernels in fp32 I/O around the 16-token staging batch: one batch short of full, full and one over, an even and an odd
    number of batches (the descending sweep then starts in either LDS buffer), with a per-sample initial state carried to s_out and gs."""
    B, H = 2, 1
    r, k, v, w, u, gy = rand_inputs(400 + T, B, T, H, "stress")
    g = torch.Generator().manual_seed(T + 2)
    s0 = (torch.randn(B, H, 64, 64, generator=g) * 0.5).to(torch.bfloat16).float().numpy()
    f32 = torch.float32
    d = [dev(x, f32) for x in (r, k, v, w, u, gy)]
    s, s_out = dev(s0, f32), torch.empty(B, H, 64, 64, device="cuda")
    yo, so = oracle.forward(r, k, v, w, u, s0, return_state=True)
    check(ops.forward_ex(*d[:5], H, s0=s, s_out=s_out, algo="scan"), yo, f32, "y")
    check(s_out, so, f32, "s_out")
    og = oracle.backward(r, k, v, w, u, gy, s0)
    gr, gk, gv, gw, gu, gs = ops.backward_ex(*d, H, s0=s, want_gs=True, algo="scan")
    for n, t in (("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw), ("gs", gs)):
        check(t, og["gs_b" if n == "gs" else n], f32, n)
    assert max_norm_err(host(gu), og["gu_b"]) <= F32_TOL


def test_autograd_surface(ops, oracle):
    """WKV_6.apply / RUN_CUDA_RWKV6 / WKV_6STATE / infctx / WKV_6_BI: gradient tuple order and values."""
    from rwkv_lm_ext_amd.wkv import (RUN_CUDA_RWKV6, RUN_CUDA_RWKV6_BI, RUN_CUDA_RWKV6_INFCTX,
                                     RUN_CUDA_RWKV6_STATE)
    bf = torch.bfloat16
    B, T, H = 2, 64, 2
    C = H * 64
    r, k, v, w, u, gy = rand_inputs(5, B, T, H)
    leaves = [dev(x, bf).requires_grad_(True) for x in (r, k, v, w, u)]
    y = RUN_CUDA_RWKV6(B, T, C, H, *leaves)
    y.backward(dev(gy, bf))
    og = oracle.backward(r, k, v, w, u, gy)
    check(y, oracle.forward(r, k, v, w, u), bf, "RUN_CUDA_RWKV6 y")
    for t, n in zip(leaves, ("gr", "gk", "gv", "gw")):
        check(t.grad, og[n], bf, "autograd " + n)
    assert leaves[4].grad.shape == (H, 64) and leaves[4].grad.dtype == bf
    check(leaves[4].grad, og["gu"], bf, "autograd gu (fp32 partials, rounded once)")

    g = torch.Generator().manual_seed(9)
    s = (torch.randn(H, 64, 64, generator=g) * 0.5).to(bf).float().numpy()
    leaves = [dev(x, bf).requires_grad_(True) for x in (r, k, v, w, u, s)]
    y = RUN_CUDA_RWKV6_STATE(B, T, C, H, *leaves)
    y.backward(dev(gy, bf))
    og = oracle.backward(r, k, v, w, u, gy, s)
    check(y, oracle.forward(r, k, v, w, u, s), bf, "states y")
    assert leaves[5].grad.shape == (H, 64, 64)
    check(leaves[5].grad, og["gs"], bf, "autograd gs (fp32 partials, rounded once)")

    sb = (torch.randn(B, H, 64, 64, generator=g) * 0.5).to(bf).float().numpy()
    leaves = [dev(x, bf).requires_grad_(True) for x in (r, k, v, w, u)]
    st = dev(sb, bf)
    y, st2 = RUN_CUDA_RWKV6_INFCTX(B, T, C, H, *leaves, st)
    assert st2 is st                                                    # updated in place, returned
    yo, so = oracle.forward(r, k, v, w, u, sb, return_state=True)
    check(y, yo, bf, "infctx y")
    check(st, so, bf, "infctx state")
    y.backward(dev(gy, bf))
    check(leaves[0].grad, oracle.backward(r, k, v, w, u, gy, sb)["gr"], bf, "infctx gr (initial state kept, Q6)")

    mask = torch.ones(B, T, dtype=torch.int32)
    mask[0, 40:] = 0
    leaves = [dev(x, bf).requires_grad_(True) for x in (r, k, v, w, u)]
    y = RUN_CUDA_RWKV6_BI(B, T, C, H, mask.cuda(), *leaves)
    y.backward(dev(gy, bf))
    check(y, oracle.bi_forward(mask.numpy(), r, k, v, w, u), bf, "WKV_6_BI y")
    ob = oracle.bi_backward(mask.numpy(), r, k, v, w, u, gy)
    check(leaves[1].grad, ob["gk"], bf, "WKV_6_BI gk")


def test_two_workgroups_per_head_is_the_same_arithmetic(ops):
    """Few (batch, head) pairs (B*H <= half the CUs) run as two workgroups per pair -- forward: two consumer waves each, backward:
    row role / column role, each with its own producers and its own copy of G -- with the same per-wave arithmetic: every output is
    bit-identical to the one-workgroup launch (dispatch(split=) forces either mode; the default picks by grid size, so the suite's small
    cases run split and the full-size ones not)."""
    bf = torch.bfloat16
    B, T, H = 3, 200, 2
    r, k, v, w, u, gy = rand_inputs(11, B, T, H)
    g = torch.Generator().manual_seed(3)
    s0 = dev((torch.randn(B, H, 64, 64, generator=g) * 0.5).numpy(), bf)
    d = [dev(x, bf) for x in (r, k, v, w, u)]
    res = []
    for split in ("0", "1"):
        with ops.dispatch(split=int(split)):
            s_out = torch.empty_like(s0)
            ck = ops.new_checkpoint(B, T, 64 * H, H, s0.device)
            y = ops.forward_ex(*d, H, s0=s0, s_out=s_out, ckpt=ck)
            grads = ops.backward_ex(*d, dev(gy, bf), H, s0=s0, want_gs=True, ckpt=ck)
            grads2 = ops.backward_ex(*d, dev(gy, bf), H, s0=s0, want_gs=True)          # own state pass
            res.append([y, s_out] + list(grads) + list(grads2))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("segments", [2, 4, 8])
def test_two_level_scan_forward_for_few_long_sequences(ops, oracle, segments):
    """Forward-only calls on few long sequences are cut into segments that run as extra workgroups (state pass per segment, a
    chaining kernel, then the ordinary forward from each segment's entry state; wkv6_tsplit.hip: chunk_forward).  dispatch(tsplit=) forces
    the segment count: y and the final state against the oracle (bf16 contract) and against the one-pass kernel (1 ulp)."""
    bf = torch.bfloat16
    B, T, H = 1, 1024, 2
    r, k, v, w, u, _ = rand_inputs(77, B, T, H, "init")
    g = torch.Generator().manual_seed(5)
    s0 = (torch.randn(B, H, 64, 64, generator=g) * 0.5).to(bf).float().numpy()
    d = [dev(x, bf) for x in (r, k, v, w, u)]
    out = {}
    for split in (0, segments):
        with ops.dispatch(tsplit=split):
            s_out = torch.empty(B, H, 64, 64, device="cuda", dtype=bf)
            out[split] = (ops.forward_ex(*d, H, s0=dev(s0, bf), s_out=s_out), s_out)
    yo, so = oracle.forward(r, k, v, w, u, s0, return_state=True)
    check(out[segments][0], yo, bf, f"{segments}-segment forward y")
    check(out[segments][1], so, bf, f"{segments}-segment forward final state")
    for a, b, n in ((out[0][0], out[segments][0], "y"), (out[0][1], out[segments][1], "state")):
        a, b = host(a), host(b)
        assert float(np.abs(a - b).max()) <= 2.0 ** -8 * float(np.abs(a).max()), n
    # training forward: the segments' checkpoints land in the whole sequence's slots and feed the ordinary backward
    with ops.dispatch(tsplit=segments):
        gy = rand_inputs(78, B, T, H, "init")[5]
        ck = ops.new_checkpoint(B, T, 64 * H, H, "cuda")
        y_ck = ops.forward_ex(*d, H, s0=dev(s0, bf), ckpt=ck)
        assert torch.equal(y_ck, out[segments][0])
        grads = ops.backward_ex(*d, dev(gy, bf), H, s0=dev(s0, bf), want_gs=True, ckpt=ck)
        og = oracle.backward(r, k, v, w, u, gy, s0)
        for n, t in zip(("gr", "gk", "gv", "gw"), grads[:4]):
            check(t, og[n], bf, f"{segments}-segment forward checkpoints -> backward {n}")
    # the stateful inference operator (fp32 state in place, decay given as exp(-exp(w))) takes the same path for a prefill
    from rwkv_lm_ext_amd.wkv6_op import rwkv6
    decay = torch.exp(-torch.exp(torch.from_numpy(w))).cuda().contiguous()
    res = []
    for split in (0, segments):
        with ops.dispatch(tsplit=split):
            state = torch.from_numpy(s0).cuda().contiguous()
            y = torch.empty(B, T, 64 * H, device="cuda", dtype=bf)
            rwkv6.forward_bf16(B, T, 64 * H, H, state, d[0], d[1], d[2], decay, d[4], y)
            res.append((y, state))
    check(res[1][0], yo, bf, "rwkv6 prefill y")
    assert max_norm_err(host(res[1][1]), so) <= 1e-3
    assert float((res[0][0].float() - res[1][0].float()).abs().max()) <= 2.0 ** -8 * float(res[0][0].float().abs().max())


@pytest.mark.parametrize("segments", [2, 4, 8])
def test_two_level_scan_backward_for_few_long_sequences(ops, oracle, segments):
    """The backward of few long sequences as a two-level scan over T (wkv6_tsplit.hip: chunk_backward): every segment runs as its own
    workgroup from the adjoint state entering it from the future (reversed state-only pass with k := r, v := gy, chained last to
    first) and from the gw suffix sum beyond its end (Phi = sum_j G S at the boundary); gu sums over the segments, gs is the adjoint
    state at the sequence start.  dispatch(tsplit=) forces the segment count: every gradient against the oracle (bf16 contract, fp32
    partials) and against the one-pass backward, with the forward's checkpoints and self-contained."""
    bf = torch.bfloat16
    B, T, H = 2, 1024, 2
    r, k, v, w, u, gy = rand_inputs(177, B, T, H, "init")
    g = torch.Generator().manual_seed(15)
    s0 = (torch.randn(B, H, 64, 64, generator=g) * 0.5).to(bf).float().numpy()
    d = [dev(x, bf) for x in (r, k, v, w, u, gy)]
    og = oracle.backward(r, k, v, w, u, gy, s0)
    res = {}
    for split in (0, segments):
        with ops.dispatch(tsplit=split):
            ck = ops.new_checkpoint(B, T, 64 * H, H, "cuda")
            ops.forward_ex(*d[:5], H, s0=dev(s0, bf), ckpt=ck)
            res[split] = (ops.backward_ex(*d, H, s0=dev(s0, bf), want_gs=True, ckpt=ck),          # the forward's checkpoints
                          ops.backward_ex(*d, H, s0=dev(s0, bf), want_gs=True))                    # self-contained
    for kept, grads in zip(("kept checkpoints", "self-contained"), res[segments]):
        for n, t in zip(("gr", "gk", "gv", "gw"), grads[:4]):
            check(t, og[n], bf, f"{segments}-segment backward ({kept}) {n}")
        assert max_norm_err(host(grads[4]), og["gu_b"]) <= PART_TOL, kept
        assert max_norm_err(host(grads[5]), og["gs_b"]) <= PART_TOL, kept
        for n, a_, b_ in zip(("gr", "gk", "gv", "gw", "gu", "gs"), res[0][0], grads):
            a_, b_ = host(a_), host(b_)
            scale = max(float(np.abs(a_).max()), 1e-3)
            assert float(np.abs(a_ - b_).max()) <= (4.0 if n in ("gw", "gu", "gs") else 2.0) * 2.0 ** -8 * scale, (kept, n)


def test_checkpoint_opt_out_gives_identical_gradients(ops, monkeypatch):
    """RWKV_AMD_NO_CKPT=1: nothing is kept from forward to backward, the backward rebuilds the state checkpoints itself --
    same kernels on the same numbers, so every gradient is bit-identical (WKV_6 and WKV_6_BI)."""
    from rwkv_lm_ext_amd.wkv import RUN_CUDA_RWKV6, RUN_CUDA_RWKV6_BI
    bf = torch.bfloat16
    B, T, H = 2, 96, 2
    C = H * 64
    r, k, v, w, u, gy = rand_inputs(7, B, T, H)
    mask = torch.ones(B, T, dtype=torch.int32)
    mask[1, 50:] = 0
    res = []
    for no_ckpt in ("0", "1"):
        monkeypatch.setenv("RWKV_AMD_NO_CKPT", no_ckpt)
        out = []
        for bi in (False, True):
            leaves = [dev(x, bf).requires_grad_(True) for x in (r, k, v, w, u)]
            y = RUN_CUDA_RWKV6_BI(B, T, C, H, mask.cuda(), *leaves) if bi else RUN_CUDA_RWKV6(B, T, C, H, *leaves)
            y.backward(dev(gy, bf))
            out += [y.detach()] + [t.grad for t in leaves]
        res.append(out)
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_full_size_properties(ops):
    """BASELINE config 2 (B=8,T=4096,C=2048,H=32), where the CPU oracle would take minutes: properties
    that do not depend on size.  (a) splitting the sequence and carrying the fp32 state reproduces the
    single call; (b) y is linear in v; (c) the oracle on one (b,h) slice of the big problem."""
    from oracle import wkv6_oracle as orc
    B, T, H = 8, 4096, 32
    C = H * 64
    g = torch.Generator(device="cuda").manual_seed(0)
    f32 = torch.float32
    r, k, v = (torch.randn(B, T, C, device="cuda", generator=g).mul_(0.5).to(torch.bfloat16).to(f32) for _ in range(3))
    ramp = torch.tensor([-6 + 5 * (n / (C - 1)) ** (0.7 + 1.3 * 0.5) for n in range(C)], device="cuda")
    w = (ramp.view(1, 1, C) + 0.1 * torch.randn(B, T, C, device="cuda", generator=g)).to(torch.bfloat16).to(f32)
    u = (torch.randn(H, 64, device="cuda", generator=g) * 0.3).to(torch.bfloat16).to(f32)
    y = ops.forward_ex(r, k, v, w, u, H)
    # (a) 2 x 2048 with carried state
    st = torch.zeros(B, H, 64, 64, device="cuda")
    parts = []
    for c in range(2):
        sl = slice(2048 * c, 2048 * (c + 1))
        parts.append(ops.forward_ex(*(x[:, sl].contiguous() for x in (r, k, v, w)), u, H, s0=st, s_out=st))
    assert max_norm_err(host(torch.cat(parts, 1)), host(y)) <= F32_TOL
    # (b) linearity in v
    v2 = torch.randn(B, T, C, device="cuda", generator=g).to(torch.bfloat16).to(f32)
    y2 = ops.forward_ex(r, k, v2, w, u, H)
    y12 = ops.forward_ex(r, k, v + 2 * v2, w, u, H)
    assert max_norm_err(host(y12), host(y + 2 * y2)) <= F32_TOL
    # (c) one head of one batch row against the oracle (fwd + bwd), full length
    b, h = 5, 17
    sl = (slice(b, b + 1), slice(None), slice(64 * h, 64 * h + 64))
    rs, ks, vs, ws = (host(x[sl]) for x in (r, k, v, w))
    us = host(u[h:h + 1])
    assert max_norm_err(host(y[sl]), orc.forward(rs, ks, vs, ws, us)) <= F32_TOL
    gy = torch.randn(B, T, C, device="cuda", generator=g).to(torch.bfloat16).to(f32)
    gr, gk, gv, gw, gu, _ = ops.backward_ex(r, k, v, w, u, gy, H)
    og = orc.backward(rs, ks, vs, ws, us, host(gy[sl]))
    for n, t in (("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw)):
        e = max_norm_err(host(t[sl]), og[n])
        assert e <= (5e-5 if n == "gw" else F32_TOL), (n, e)       # gw: 4096-term suffix sums in fp32
    assert max_norm_err(host(gu[b, 64 * h:64 * h + 64]), og["gu_b"][0]) <= 5e-5


# ---- chunked MFMA forward (the default bf16 path) --------------------------------------------------
@pytest.mark.parametrize("name", PLAIN + ["wkv6_state", "wkv6_infctx"])
def test_chunk_forward_golden(ops, name):
    """Default bf16 forward = chunked MFMA kernel; `algo="scan"` = exact kernel.  Both must meet the bf16
    tolerance against the reference vectors; state variants also check the final state."""
    g = load_golden(name)
    H = g["u"].shape[0]
    bf = torch.bfloat16
    r, k, v, w, u = (dev(g[n], bf) for n in ("r", "k", "v", "w", "u"))
    s0 = dev(g["s"], bf) if "s" in g else None
    for algo in (None, "scan"):
        s_out = torch.empty(r.shape[0], H, 64, 64, device="cuda", dtype=bf) if "s_final" in g else None
        y = ops.forward_ex(r, k, v, w, u, H, s0=s0, s_out=s_out, algo=algo)
        check(y, g["y"], bf, f"{name} y ({algo or 'chunk'})")
        if s_out is not None:
            check(s_out, g["s_final"], bf, f"{name} final state ({algo or 'chunk'})")
    # reference ABI (fp32 ew) goes through the chunked kernel as well
    if s0 is None:
        B, T, C = g["r"].shape
        ew = (-torch.exp(w.float())).contiguous()
        y = torch.empty(B, T, C, device="cuda", dtype=bf)
        ops.wkv6_cuda.forward(B, T, C, H, r, k, v, ew, u, y)
        check(y, g["y"], bf, name + " y (chunk, fp32 ew)")


@pytest.mark.parametrize("shape", [(2, 300, 3, "stress"), (1, 1000, 2, "init"), (3, 17, 1, "stress"),
                                   (2, 64, 2, "init"), (1, 129, 1, "stress")],
                         ids=["B2T300H3", "B1T1000H2", "B3T17H1", "B2T64H2", "B1T129H1"])
def test_chunk_forward_random_vs_oracle(ops, oracle, shape):
    B, T, H, kind = shape
    r, k, v, w, u, gy = rand_inputs(200 + T, B, T, H, kind)
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(T)
    s0 = (torch.randn(B, H, 64, 64, generator=g) * 0.5).to(bf).float().numpy()
    d = [dev(t, bf) for t in (r, k, v, w, u)]
    yo, so = oracle.forward(r, k, v, w, u, s0, return_state=True)
    s_out = torch.empty(B, H, 64, 64, device="cuda", dtype=bf)
    y = ops.forward_ex(*d, H, s0=dev(s0, bf), s_out=s_out)
    check(y, yo, bf, "chunk y")
    check(s_out, so, bf, "chunk final state")


def test_chunk_forward_accuracy_report(ops, oracle):
    """How close the chunked kernel is to the exact result BEFORE the bf16 rounding hides it: run both
    kernels on the same inputs and compare their bf16 outputs; they must agree on >= 97 % of the significant
    elements and never differ by more than one bf16 ulp (2^-7 relative)."""
    B, T, H = 2, 512, 4
    r, k, v, w, u, _ = rand_inputs(77, B, T, H, "init")
    bf = torch.bfloat16
    d = [dev(t, bf) for t in (r, k, v, w, u)]
    yc = host(ops.forward_ex(*d, H))
    ys = host(ops.forward_ex(*d, H, algo="scan"))
    big = np.abs(ys) >= 1e-2 * np.abs(ys).max()
    same = float(np.mean(yc[big] == ys[big]))
    rel = float((np.abs(yc - ys)[big] / np.abs(ys[big])).max())
    assert same >= 0.97 and rel <= 2.0 ** -7 * 1.01, (same, rel)


# ---- chunked MFMA backward (the default bf16 path) -------------------------------------------------
@pytest.mark.parametrize("algo", [None, "scan"], ids=["chunk", "scan"])
@pytest.mark.parametrize("shape", [(2, 300, 3, "stress"), (1, 1000, 2, "init"), (3, 17, 1, "stress"),
                                   (2, 64, 2, "init"), (1, 129, 1, "stress")],
                         ids=["B2T300H3", "B1T1000H2", "B3T17H1", "B2T64H2", "B1T129H1"])
def test_backward_random_vs_oracle_with_state(ops, oracle, shape, algo):
    """bf16 backward of both kernels against the oracle, with a per-sample initial state (gs checked)."""
    B, T, H, kind = shape
    r, k, v, w, u, gy = rand_inputs(300 + T, B, T, H, kind)
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(T + 1)
    s0 = (torch.randn(B, H, 64, 64, generator=g) * 0.5).to(bf).float().numpy()
    d = [dev(t, bf) for t in (r, k, v, w, u, gy)]
    og = oracle.backward(r, k, v, w, u, gy, s0)
    gr, gk, gv, gw, gu, gs = ops.backward_ex(*d, H, s0=dev(s0, bf), want_gs=True, algo=algo)
    for n, t in (("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw), ("gs_b", gs.to(bf))):
        check(t, og[n], bf, f"{n} ({algo or 'chunk'})")
    assert max_norm_err(host(gu), og["gu_b"]) <= PART_TOL


def test_chunk_backward_agrees_with_scan(ops):
    """Same inputs through both backward implementations: bf16 outputs identical on >= 97 % of the significant
    elements, never more than one bf16 ulp apart (gw: two, it is a 512-term suffix sum)."""
    B, T, H = 2, 512, 4
    r, k, v, w, u, gy = rand_inputs(78, B, T, H, "init")
    bf = torch.bfloat16
    d = [dev(t, bf) for t in (r, k, v, w, u, gy)]
    oc = ops.backward_ex(*d, H)
    osn = ops.backward_ex(*d, H, algo="scan")
    for n, c, s_ in zip(("gr", "gk", "gv", "gw"), oc, osn):
        c, s_ = host(c), host(s_)
        big = np.abs(s_) >= 1e-2 * np.abs(s_).max()
        same = float(np.mean(c[big] == s_[big]))
        rel = float((np.abs(c - s_)[big] / np.abs(s_[big])).max())
        assert same >= 0.97 and rel <= 2.0 ** -7 * (2.02 if n == "gw" else 1.01), (n, same, rel)


@pytest.mark.parametrize("T", [1, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65, 95, 97, 129])
def test_chunked_kernels_at_block_and_stage_boundaries(ops, T):
    """Sequence lengths around the 16-token block, 32-token stage and 64-token group boundaries, with an initial state:
    the chunked forward / backward (checkpoint path included) against the exact scan kernels on the same inputs."""
    B, H = 2, 2
    r, k, v, w, u, gy = rand_inputs(300 + T, B, T, H, "init")
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(T)
    s0 = dev((torch.randn(H, 64, 64, generator=g) * 0.5).numpy(), bf)
    d = [dev(t, bf) for t in (r, k, v, w, u, gy)]
    ck = ops.new_checkpoint(B, T, H * 64, H, "cuda")
    yc = ops.forward_ex(*d[:5], H, s0=s0, ckpt=ck)
    ys = ops.forward_ex(*d[:5], H, s0=s0, algo="scan")
    oc = ops.backward_ex(*d, H, s0=s0, want_gs=True, ckpt=ck)
    osn = ops.backward_ex(*d, H, s0=s0, want_gs=True, algo="scan")
    for n, c, s_ in zip(("y", "gr", "gk", "gv", "gw", "gu", "gs"), (yc,) + tuple(oc), (ys,) + tuple(osn)):
        c, s_ = host(c), host(s_)
        scale = max(float(np.abs(s_).max()), 1e-3)
        assert float(np.abs(c - s_).max()) <= (4.0 if n in ("gw", "gu", "gs") else 2.0) * 2.0 ** -8 * scale, (n, T)


def test_fuzz_chunked_against_scan_kernels(ops):
    """Seeded random shapes, lengths and decay regimes: the chunked kernels (plain, with state, wkv6_bi with ragged masks that
    include one-token and full-length rows) against the exact scan kernels on the device, same inputs, both bf16."""
    bf = torch.bfloat16
    rng = np.random.default_rng(2024)

    def agree(tag, names, got, ref):
        for n, c, s_ in zip(names, got, ref):
            c, s_ = host(c), host(s_)
            # gw_t = lw_t (sum of r dq - k dk terms that cancel): for very short sequences the true value is ~0 and what is left
            # is the 2^-16 operand error of the split-bf16 products times the size of the cancelling terms (O(1..10)), hence
            # the absolute floor for gw
            scale = max(float(np.abs(s_).max()), 1e-2 if n == "gw" else 1e-3)
            assert float(np.abs(c - s_).max()) <= (4.0 if n in ("gw", "gu", "gs") else 2.0) * 2.0 ** -8 * scale, (tag, n)

    for case in range(24):
        B, H = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        T = int(rng.choice([1, 2, 3, 15, 16, 17, 31, 33, 47, 64, 65, 95, 96, 97, 130, 191]))
        regime = ("init", "stress")[case % 2]
        r, k, v, w, u, gy = rand_inputs(5000 + case, B, T, H, regime)
        d = [dev(t, bf) for t in (r, k, v, w, u, gy)]
        tag = (case, B, T, H, regime)
        if case % 3 == 2:       # wkv6_bi with ragged masks
            mask = torch.ones(B, T, dtype=torch.int32)
            for b in range(B):
                cut = int(rng.integers(0, T + 1))          # 0: the first token is already masked; T: no zero in the row
                if cut < T:
                    mask[b, cut:] = 0
            m = mask.cuda()
            yc, ys = ops.bi_forward_ex(m, *d[:5], H), ops.bi_forward_ex(m, *d[:5], H, algo="scan")
            agree(tag, ("y",), (yc,), (ys,))
            agree(tag, ("gr", "gk", "gv", "gw", "gu"), ops.bi_backward_ex(m, *d, H), ops.bi_backward_ex(m, *d, H, algo="scan"))
        else:
            g = torch.Generator().manual_seed(case)
            s0 = dev((torch.randn(B, H, 64, 64, generator=g) * 0.5).numpy(), bf) if case % 3 == 1 else None
            ck = ops.new_checkpoint(B, T, H * 64, H, "cuda")
            yc = ops.forward_ex(*d[:5], H, s0=s0, ckpt=ck)
            ys = ops.forward_ex(*d[:5], H, s0=s0, algo="scan")
            agree(tag, ("y",), (yc,), (ys,))
            names = ("gr", "gk", "gv", "gw", "gu", "gs")
            oc = ops.backward_ex(*d, H, s0=s0, want_gs=s0 is not None, ckpt=ck)
            osn = ops.backward_ex(*d, H, s0=s0, want_gs=s0 is not None, algo="scan")
            n = 6 if s0 is not None else 5
            agree(tag, names[:n], oc[:n], osn[:n])


def test_forward_checkpoints_feed_backward(ops, oracle):
    """Training path: forward_ex(ckpt=) stores the per-group states, backward_ex(ckpt=) consumes them; results
    must be identical (bitwise) to the self-contained backward that recomputes them with its own state pass."""
    B, T, H = 2, 333, 2
    r, k, v, w, u, gy = rand_inputs(91, B, T, H, "stress")
    bf = torch.bfloat16
    d = [dev(t, bf) for t in (r, k, v, w, u, gy)]
    ck = ops.new_checkpoint(B, T, H * 64, H, "cuda")
    y1 = ops.forward_ex(*d[:5], H, ckpt=ck)
    y0 = ops.forward_ex(*d[:5], H)
    assert torch.equal(y0, y1)
    g1 = ops.backward_ex(*d, H, ckpt=ck)
    g0 = ops.backward_ex(*d, H)
    for a_, b_ in zip(g0[:5], g1[:5]):
        assert torch.equal(a_, b_)
    check(g1[3], oracle.backward(r, k, v, w, u, gy)["gw"], bf, "ckpt path gw")


@pytest.mark.parametrize("io", IOS, ids=["f32", "bf16"])
def test_rwkv6_stateful_inference_kernel(ops, oracle, io):
    """cuda/rwkv6.cu: fp32 state in/out, decay already exponentiated; two consecutive calls continue the sequence."""
    from rwkv_lm_ext_amd.wkv import RUN_RWKV_6
    B, T, H = 1, 50, 2
    C = H * 64
    r, k, v, w, u, _ = rand_inputs(55, B, T, H)
    g = torch.Generator().manual_seed(56)
    s0 = (torch.randn(H, 64, 64, generator=g) * 0.5).numpy()
    yo, so = oracle.forward(r, k, v, w, u, s0, return_state=True)
    d = [dev(t, io) for t in (r, k, v, w, u)]
    state = dev(s0, torch.float32)
    y1, st = RUN_RWKV_6(B, 30, C, H, state, *(t[:, :30].contiguous() for t in d[:4]), d[4])
    assert st.data_ptr() == state.data_ptr()                                  # updated in place and returned
    y2, _ = RUN_RWKV_6(B, 20, C, H, state, *(t[:, 30:].contiguous() for t in d[:4]), d[4])
    check(torch.cat([y1, y2], 1), yo, io, "rwkv6 y")
    assert max_norm_err(host(state), so[0]) <= F32_TOL                       # fp32 state: exact carry
    # B > 1 (the reference kernel is wrong there): one state per row
    B2 = 3
    r, k, v, w, u, _ = rand_inputs(57, B2, 20, H)
    sb = (torch.randn(B2, H, 64, 64, generator=g) * 0.5).numpy()
    yo, so = oracle.forward(r, k, v, w, u, sb, return_state=True)
    stb = dev(sb, torch.float32)
    y, _ = RUN_RWKV_6(B2, 20, C, H, stb, *(dev(t, io) for t in (r, k, v, w, u)))
    check(y, yo, io, "rwkv6 batched y")
    assert max_norm_err(host(stb), so) <= F32_TOL
    # prefill-sized call: bf16 goes through the chunked MFMA kernel (state stays fp32), then a short decode continues it
    Tp = 300
    r, k, v, w, u, _ = rand_inputs(58, 2, Tp + 3, H)
    sb = (torch.randn(2, H, 64, 64, generator=g) * 0.5).numpy()
    yo, so = oracle.forward(r, k, v, w, u, sb, return_state=True)
    d = [dev(t, io) for t in (r, k, v, w, u)]
    st2 = dev(sb, torch.float32)
    y1, _ = RUN_RWKV_6(2, Tp, C, H, st2, *(t[:, :Tp].contiguous() for t in d[:4]), d[4])
    y2, _ = RUN_RWKV_6(2, 3, C, H, st2, *(t[:, Tp:].contiguous() for t in d[:4]), d[4])
    check(torch.cat([y1, y2], 1), yo, io, "rwkv6 prefill + decode y")
    assert max_norm_err(host(st2), so) <= (F32_TOL if io == torch.float32 else 2e-4)   # chunked path: split-bf16 products


def test_rwkv6_fp16_symbol_widens_in_the_kernel(ops, oracle):
    """rwkv6_cuda_forward_fp16 (cuda/rwkv6_op.cpp:9, 16-19): fp16 r, k, v, u, y with the fp32 state and decay of the other flavours;
    inputs are widened in the kernel (no fp32 copies on the host side), y is rounded to fp16 once.  Checked against the oracle on
    the fp16-rounded inputs, and bit for bit against the fp32 flavour rounded to fp16."""
    B, T, H = 2, 41, 2
    C = H * 64
    h16 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float16)
    r, k, v, w, u, _ = rand_inputs(77, B, T, H)
    r16, k16, v16, u16 = (h16(t) for t in (r, k, v, u))
    g = torch.Generator().manual_seed(78)
    s0 = (torch.randn(B, H, 64, 64, generator=g) * 0.5).numpy()
    yo, so = oracle.forward(r16.float().numpy(), k16.float().numpy(), v16.float().numpy(), w, u16.float().numpy(), s0, return_state=True)
    decay = torch.exp(-torch.exp(torch.from_numpy(w).float())).cuda().contiguous()       # src/model_run.py:64
    st16, st32 = dev(s0, torch.float32), dev(s0, torch.float32)
    y16 = torch.empty(B, T, C, dtype=torch.float16, device="cuda")
    ops.rwkv6.forward_fp16(B, T, C, H, st16, r16.cuda(), k16.cuda(), v16.cuda(), decay, u16.cuda(), y16)
    assert max_norm_err(host(y16), yo) <= 1e-3                        # fp16 output rounding: 2^-11 relative
    assert max_norm_err(host(st16), so) <= F32_TOL
    y32 = torch.empty(B, T, C, dtype=torch.float32, device="cuda")
    ops.rwkv6.forward_fp32(B, T, C, H, st32, r16.cuda().float(), k16.cuda().float(), v16.cuda().float(), decay, u16.cuda().float(), y32)
    assert torch.equal(y16, y32.to(torch.float16)) and torch.equal(st16, st32)
