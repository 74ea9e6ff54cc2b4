"""The WKV5 (RWKV-5, static decay) operator on the GPU: every public surface against the pinned fp64 WKV6 oracle with the decay
broadcast over batch and time and gw summed over time (the identity tests/test_wkv5_cpu.py pins), the fp32 flavour, the headline
shape, equivalence with the existing WKV6 scan kernels, bit-reproducibility, graph capture and the time-mix caller."""
import numpy as np
import pytest
import torch

import wkv5_numpy as w5
from conftest import max_norm_err
from oracle.contract import F32_TOL, bf16_ok, bf16_report_torch, BF16_RMS, BF16_ULPS, BF16_EXACT

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
# floors of the bf16 contract: what tests/test_wkv6_gpu.py's check and __graft_entry__.smoke() use for the same tensors.  gw [H,N]
# and gw [B,C] keep gw's 0.1: they are sums of the WKV6 gw over tokens (and batch), never smaller in scale than a single token's.
FLOOR = dict(y=1e-3, gr=1e-3, gk=1e-3, gv=1e-3, gu=1e-3, gu_b=1e-3, gw=0.1, gw_b=0.1)


def dev(a, dtype=bf):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def host(t):
    return t.detach().float().cpu().numpy()


def contract(out, ref, name, what):
    ok, msg = bf16_ok(host(out).reshape(np.shape(ref)), ref, floor=FLOOR[name])
    print(f"{what} {name}: {msg}")
    assert ok, (what, name, msg)


def decay_pair(w):
    """ew, eew as the reference's WKV_5.forward builds them (src/model.py:260-261): fp32 [H,N]."""
    ew = (-torch.exp(w.float())).contiguous()
    return torch.exp(ew).contiguous(), ew


def reference_style(mod, B, T, C, H, t):
    """forward + backward through a module object with the reference's positional signatures (src/model.py:264, 282)."""
    eew, ew = decay_pair(t["w"])
    y = torch.empty_like(t["r"])
    mod.forward(B, T, C, H, t["r"], t["k"], t["v"], eew, t["u"], y)
    gr, gk, gv = (torch.empty_like(t["r"]) for _ in range(3))
    gw, gu = (torch.empty(B, C, dtype=bf, device="cuda") for _ in range(2))
    mod.backward(B, T, C, H, t["r"], t["k"], t["v"], eew, ew, t["u"], t["gy"], gr, gk, gv, gw, gu)
    return dict(y=y, gr=gr, gk=gk, gv=gv, gw_b=gw, gu_b=gu)


@pytest.fixture(scope="module")
def shim():
    from rwkv_lm_ext_amd import torch_shim
    return torch_shim.load(prefix="shim")


# T in {1, 2, 3, 15, 16, 17, 64, 160, 1000}; B*H from 1 to 288 (> 256 CUs); H = 32 twice
SHAPES = [(1, 1, 1), (2, 2, 2), (1, 3, 2), (3, 15, 2), (2, 16, 1), (2, 17, 3), (1, 64, 32), (5, 160, 2), (2, 1000, 2), (9, 16, 32)]


@pytest.mark.parametrize("decay_set", ["ramp", "stress"])
@pytest.mark.parametrize("B,T,H", SHAPES)
def test_parity_bf16_every_surface(oracle, shim, B, T, H, decay_set):
    from rwkv_lm_ext_amd import wkv6_op
    from rwkv_lm_ext_amd.wkv import WKV_5
    C = 64 * H
    p = w5.problem(B, T, H, seed=100 + T + H, decay_set=decay_set)
    yo, go = w5.oracle_pair(oracle, **p)
    ref = dict(go, y=yo)
    t = {n: dev(a) for n, a in p.items()}

    class TorchOps:
        forward, backward = torch.ops.wkv5.forward, torch.ops.wkv5.backward

    surfaces = {"ctypes": wkv6_op.wkv5, "torch.ops": TorchOps, "shim": shim.wkv5}
    got = {}
    for what, mod in surfaces.items():
        got[what] = reference_style(mod, B, T, C, H, t)
        for n in ("y", "gr", "gk", "gv", "gw_b", "gu_b"):
            contract(got[what][n], ref[n], n, f"{what} B{B} T{T} H{H} {decay_set}")
    for what in ("torch.ops", "shim"):                                   # the same library underneath
        for n, a in got[what].items():
            assert torch.equal(a, got["ctypes"][n]), (what, n)
    if T <= 2:
        assert not got["ctypes"]["gw_b"].float().abs().any()            # exactly zero (cuda/wkv5_cuda.cu:119: empty loop)
    # the autograd function: raw bf16 w, [H,N] parameter gradients
    leaves = [t[n].clone().requires_grad_(True) for n in ("r", "k", "v", "w", "u")]
    y = WKV_5.apply(B, T, C, H, *leaves)
    y.backward(t["gy"])
    contract(y, ref["y"], "y", "WKV_5")
    for leaf, n in zip(leaves, ("gr", "gk", "gv", "gw", "gu")):
        assert leaf.grad.shape == leaf.shape and leaf.grad.dtype == bf
        contract(leaf.grad, ref[n], n, f"WKV_5 B{B} T{T} H{H} {decay_set}")


@pytest.mark.parametrize("decay_set", ["ramp", "stress"])
@pytest.mark.parametrize("B,T,H", [(2, 1, 2), (1, 2, 1), (2, 17, 2), (3, 160, 2), (2, 1000, 2), (5, 64, 32),
                                   (2, 16, 1), (1, 32, 1), (1, 33, 1)])      # one full staging batch, an even and an odd number of batches
def test_fp32_flavour_vs_oracle(oracle, B, T, H, decay_set):
    from rwkv_lm_ext_amd import wkv6_op
    p = w5.problem(B, T, H, seed=7 + T, decay_set=decay_set)
    yo, go = w5.oracle_pair(oracle, **p)
    t = {n: dev(a, torch.float32) for n, a in p.items()}
    y = wkv6_op.wkv5_forward_ex(t["r"], t["k"], t["v"], t["w"], t["u"], H)
    gr, gk, gv, gw, gu = wkv6_op.wkv5_backward_ex(t["r"], t["k"], t["v"], t["w"], t["u"], t["gy"], H)
    errs = {"y": max_norm_err(host(y), yo)}
    for n, a in (("gr", gr), ("gk", gk), ("gv", gv), ("gw_b", gw), ("gu_b", gu)):
        errs[n] = max_norm_err(host(a), go[n])
    print(f"fp32 B{B} T{T} H{H} {decay_set}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert all(e <= F32_TOL for e in errs.values()), errs
    if T <= 2:
        assert not gw.abs().any()


def test_equivalence_with_wkv6_scan_kernels_on_broadcast_decay():
    """WKV5(r,k,v,w,u) == WKV6(r,k,v,broadcast(w),u): the new kernels against the existing exact scan kernels (fp32 I/O)."""
    from rwkv_lm_ext_amd import wkv6_op
    for (B, T, H), decay_set in (((2, 160, 2), "ramp"), ((3, 200, 3), "stress"), ((1, 1000, 2), "ramp")):
        C = 64 * H
        p = w5.problem(B, T, H, seed=31 + T, decay_set=decay_set)
        t = {n: dev(a, torch.float32) for n, a in p.items()}
        wb = t["w"].view(1, 1, C).expand(B, T, C).contiguous()
        y6 = wkv6_op.forward_ex(t["r"], t["k"], t["v"], wb, t["u"], H, algo="scan")
        g6 = wkv6_op.backward_ex(t["r"], t["k"], t["v"], wb, t["u"], t["gy"], H, algo="scan")
        y5 = wkv6_op.wkv5_forward_ex(t["r"], t["k"], t["v"], t["w"], t["u"], H)
        g5 = wkv6_op.wkv5_backward_ex(t["r"], t["k"], t["v"], t["w"], t["u"], t["gy"], H)
        errs = {"y": max_norm_err(host(y5), host(y6))}
        for i, n in enumerate(("gr", "gk", "gv")):
            errs[n] = max_norm_err(host(g5[i]), host(g6[i]))
        errs["gu_b"] = max_norm_err(host(g5[4]), host(g6[4]))
        print(f"wkv5 vs wkv6 scan B{B} T{T} H{H} {decay_set}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
        assert all(e <= F32_TOL for e in errs.values()), errs


def _headline():
    B, T, H = 8, 4096, 32
    C = 64 * H
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g, device="cuda") * scale).to(bf)
    r, k, v = (rnd(B, T, C, scale=0.5) for _ in range(3))
    gy = rnd(B, T, C)
    u = rnd(H, 64, scale=0.3)
    n = torch.arange(C, dtype=torch.float32, device="cuda")
    w = (-6 + 5 * (n / (C - 1)) ** 0.7).view(H, 64).to(bf)
    return B, T, C, H, dict(r=r, k=k, v=v, w=w, u=u, gy=gy)


def test_headline_shape_vs_oracle_slices_and_scan_partials(oracle):
    """B=8, T=4096, C=2048, H=32.  y, gr, gk, gv and the [B,C] partials of a handful of (b, h) pairs against the oracle on that
    pair's slice (every pair is an independent recurrence); all of gw, gu against the WKV6 scan kernels' fp32 result on the
    broadcast decay, reduced in fp64 on the device.

    Bound of that second comparison, PART_TOL = 1e-4 of max|ref|: both sides are fp32 accumulations of T = 4096 terms per
    channel in different orders (the WKV6 path forms gw_t from running suffix sums, then is summed over t here; WKV5 adds
    r_t (gy_t . D_t) token by token).  The worst case of a length-T fp32 sum is T 2^-24 = 2.4e-4 of sum|terms|, a random walk
    gives sqrt(T) 2^-24 = 4e-6; 1e-4 sits between the two and is 50 times tighter than the bf16 half-ulp (2^-9) that the
    [H,N] contract resolves."""
    from rwkv_lm_ext_amd import wkv6_op
    from rwkv_lm_ext_amd.wkv import WKV_5
    PART_TOL = 1e-4
    B, T, C, H, t = _headline()
    y = wkv6_op.wkv5_forward_ex(t["r"], t["k"], t["v"], t["w"], t["u"], H)
    gr, gk, gv, gw_b, gu_b = wkv6_op.wkv5_backward_ex(t["r"], t["k"], t["v"], t["w"], t["u"], t["gy"], H)
    torch.cuda.synchronize()
    for b, h in ((0, 0), (3, 17), (7, 31), (5, 8)):
        sl = (slice(b, b + 1), slice(None), slice(64 * h, 64 * h + 64))
        p = {n: host(t[n][sl]) for n in ("r", "k", "v", "gy")}
        p["w"], p["u"] = host(t["w"][h:h + 1]), host(t["u"][h:h + 1])
        yo, go = w5.oracle_pair(oracle, **p)
        contract(y[sl], yo, "y", f"headline ({b},{h})")
        for n, a in (("gr", gr), ("gk", gk), ("gv", gv)):
            contract(a[sl], go[n], n, f"headline ({b},{h})")
        csl = (slice(b, b + 1), slice(64 * h, 64 * h + 64))
        e_w, e_u = max_norm_err(host(gw_b[csl]), go["gw_b"]), max_norm_err(host(gu_b[csl]), go["gu_b"])
        print(f"headline ({b},{h}) fp32 partials vs oracle: gw {e_w:.2e}, gu {e_u:.2e}")
        assert e_w <= PART_TOL and e_u <= PART_TOL, (b, h, e_w, e_u)
    # every channel: the WKV6 scan path in fp32 I/O on the broadcast decay, gw summed over t in fp64 on the device
    f = {n: a.float() for n, a in t.items()}
    wb = f["w"].view(1, 1, C).expand(B, T, C).contiguous()
    g6 = wkv6_op.backward_ex(f["r"], f["k"], f["v"], wb, f["u"], f["gy"], H, algo="scan")
    gw6_b, gu6_b = g6[3].double().sum(1), g6[4].double()
    del g6, wb, f
    e_w = float((gw_b.double() - gw6_b).abs().max() / gw6_b.abs().max())
    e_u = float((gu_b.double() - gu6_b).abs().max() / gu6_b.abs().max())
    print(f"headline fp32 partials vs WKV6 scan: gw {e_w:.2e}, gu {e_u:.2e}")
    assert e_w <= PART_TOL and e_u <= PART_TOL, (e_w, e_u)
    # WKV_5's [H,N] gradients: the bf16 contract against the same reference summed over the batch
    leaves = [t[n].clone().requires_grad_(True) for n in ("r", "k", "v", "w", "u")]
    WKV_5.apply(B, T, C, H, *leaves).backward(t["gy"])
    for leaf, ref, n in ((leaves[3], gw6_b.sum(0), "gw"), (leaves[4], gu6_b.sum(0), "gu")):
        rms, off, ulps = bf16_report_torch(leaf.grad.view(-1), ref.view(-1), FLOOR[n])
        print(f"headline WKV_5 {n} [H,N]: bf16 rel-rms {rms:.2e}, max {ulps:.2f} ulp, {off * 100:.1f}% not correctly rounded")
        assert rms <= BF16_RMS and ulps <= BF16_ULPS and off <= 1 - BF16_EXACT, (n, rms, off, ulps)
    assert torch.equal(leaves[0].grad, gr) and torch.equal(leaves[1].grad, gk) and torch.equal(leaves[2].grad, gv)


def test_two_calls_are_bit_identical():
    from rwkv_lm_ext_amd import wkv6_op
    B, T, H = 5, 1000, 13
    p = w5.problem(B, T, H, seed=77, decay_set="ramp")
    t = {n: dev(a) for n, a in p.items()}
    run = lambda: (wkv6_op.wkv5_forward_ex(t["r"], t["k"], t["v"], t["w"], t["u"], H),) + \
        wkv6_op.wkv5_backward_ex(t["r"], t["k"], t["v"], t["w"], t["u"], t["gy"], H)
    first, second = run(), run()
    for n, a, b in zip(("y", "gr", "gk", "gv", "gw", "gu"), first, second):
        assert torch.equal(a, b), n


def test_drop_in_pair_and_ex_pair_agree_bit_for_bit():
    """wkv5_cuda_* is wkv5_*_ex with flags = 0 (fp32 decay + ew, bf16 partials); WKV6_PARTIALS_F32 changes nothing but the
    element type of gw, gu (their bf16 rounding is the drop-in's value); the raw-w flag forms the same decay in the kernel."""
    from rwkv_lm_ext_amd import _lib, wkv6_op
    lib = _lib.load()
    B, T, H = 3, 130, 2
    C = 64 * H
    p = w5.problem(B, T, H, seed=9)
    t = {n: dev(a) for n, a in p.items()}
    ref = reference_style(wkv6_op.wkv5, B, T, C, H, t)
    eew, ew = decay_pair(t["w"])
    st = torch.cuda.current_stream().cuda_stream
    P = lambda x: x.data_ptr()
    for flags, part_dt in ((0, bf), (_lib.PARTIALS_F32, torch.float32)):
        y, gr, gk, gv = (torch.empty_like(t["r"]) for _ in range(4))
        gw, gu = (torch.empty(B, C, dtype=part_dt, device="cuda") for _ in range(2))
        assert lib.wkv5_forward_ex(B, T, C, H, P(t["r"]), P(t["k"]), P(t["v"]), P(eew), P(t["u"]), P(y), flags, st) == 0
        assert lib.wkv5_backward_ex(B, T, C, H, P(t["r"]), P(t["k"]), P(t["v"]), P(eew), P(ew), P(t["u"]), P(t["gy"]), P(gr), P(gk),
                                    P(gv), P(gw), P(gu), flags, st) == 0
        torch.cuda.synchronize()
        for n, a in (("y", y), ("gr", gr), ("gk", gk), ("gv", gv), ("gw_b", gw.to(bf)), ("gu_b", gu.to(bf))):
            assert torch.equal(a, ref[n]), (flags, n)
    # gw, gu may be NULL
    gr2, gk2, gv2 = (torch.empty_like(t["r"]) for _ in range(3))
    assert lib.wkv5_backward_ex(B, T, C, H, P(t["r"]), P(t["k"]), P(t["v"]), P(eew), None, P(t["u"]), P(t["gy"]), P(gr2), P(gk2),
                                P(gv2), None, None, 0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(gr2, ref["gr"]) and torch.equal(gk2, ref["gk"]) and torch.equal(gv2, ref["gv"])


def test_the_op_replays_from_a_graph():
    from rwkv_lm_ext_amd import wkv6_op
    B, T, H = 2, 200, 2
    p = w5.problem(B, T, H, seed=21)
    t = {n: dev(a) for n, a in p.items()}
    y_ref = wkv6_op.wkv5_forward_ex(t["r"], t["k"], t["v"], t["w"], t["u"], H)
    g_ref = wkv6_op.wkv5_backward_ex(t["r"], t["k"], t["v"], t["w"], t["u"], t["gy"], H)
    y = torch.empty_like(t["r"])
    outs = {}

    def step():
        wkv6_op.wkv5_forward_ex(t["r"], t["k"], t["v"], t["w"], t["u"], H, y=y)
        outs["g"] = wkv6_op.wkv5_backward_ex(t["r"], t["k"], t["v"], t["w"], t["u"], t["gy"], H)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                     # warm-up on the capture stream: library load, self-test, attribute calls
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.current_stream().wait_stream(side)
    captured = outs["g"]
    y.zero_()
    for a in captured:
        a.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, y_ref)
    for n, a, b in zip("gr gk gv gw gu".split(), captured, g_ref):
        assert torch.equal(a, b), n
    t["r"].copy_(dev(w5.problem(B, T, H, seed=22)["r"]))
    y2 = wkv6_op.wkv5_forward_ex(t["r"], t["k"], t["v"], t["w"], t["u"], H)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, y2)


def test_tmix_x052_forward_and_backward_vs_fp32_cpu_module():
    """The bf16 GPU module (HIP operator) against the same module in fp32 on the CPU with the numpy restatement as its operator,
    by max_norm_err, with the bounds tests/test_callers_gpu.py holds a bf16 GPU module to against its fp32 self: outputs TOL = 3e-2
    (its yardstick (1)), gradients 6e-2 (test_bi_encoder_training_step_gradients: `e_ref <= 6e-2`, "against fp32: the bf16 model's
    own precision"; its 3e-2 is the bound of another comparison, the operator swapped inside one GPU pipeline).
    Measured on MI355X: out 1.6e-2; gradients between 5e-3 and 5.7e-2, the largest on the tensors behind the operator's
    (v_t . gy_t) terms (time_faaaa 5.7e-2, dx 5.0e-2, key.weight 3.6e-2, receptance.weight 3.1e-2); the operator itself on
    such data is inside the bf16 contract (<= 1 ulp).
    The module writes its GroupNorm out: torch's group_norm backward returned wrong weight / bias gradients for [B*T, C] rows on
    this GPU stack (fp32 too, against the CPU: 0.86 / 1.0 by this metric), which is how this test first failed."""
    import copy
    from rwkv_lm_ext_amd.callers import RWKV_Tmix_x052
    TOL, GRAD_TOL = 3e-2, 6e-2
    n_embd, B, T = 256, 3, 96
    torch.manual_seed(4)
    cpu = RWKV_Tmix_x052(n_embd, n_embd, wkv=w5.numpy_wkv5).init_like_reference(layer_id=1, n_layer=4)
    with torch.no_grad():
        for lin in (cpu.receptance, cpu.key, cpu.value, cpu.gate, cpu.output):
            lin.weight.normal_(0, n_embd ** -0.5)
        for prm in cpu.parameters():
            prm.copy_(prm.to(bf).float())                                # both copies start from the same bf16 values
    gpu = copy.deepcopy(cpu)
    gpu.wkv = RWKV_Tmix_x052(64, 64).wkv                                 # the default: the HIP operator
    gpu = gpu.cuda().to(bf)
    x = torch.randn(B, T, n_embd).to(bf)
    probe = torch.randn(B, T, n_embd).to(bf)
    xc = x.float().requires_grad_(True)
    xg = x.cuda().requires_grad_(True)
    out_c = cpu(xc)
    out_c.backward(probe.float())
    out_g = gpu(xg)
    assert out_g.dtype == bf
    out_g.backward(probe.cuda())
    errs = {"out": max_norm_err(host(out_g), host(out_c)), "dx": max_norm_err(host(xg.grad), host(xc.grad))}
    for (n, pc), (_, pg) in zip(cpu.named_parameters(), gpu.named_parameters()):
        errs[n] = max_norm_err(host(pg.grad), host(pc.grad))
    print("tmix x052 bf16 GPU vs fp32 CPU: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert errs["out"] <= TOL and all(e <= GRAD_TOL for n, e in errs.items() if n != "out"), errs
