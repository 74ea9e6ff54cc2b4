"""CPU tier of the LM-head cross-entropy (include/wkv6_amd.h: wkv6_ce_rows_*): the six symbols against the header and _lib, every refusal
of the C calls with its code and in its order (dummy pointers, nothing is launched), what mix_op.ce_rows refuses before it calls the
library, the eager branch of callers.lm_loss against the reference's three lines (restated here from src/model.py:960-974, 1249-1269),
callers.head_loss against lm_loss on the unchunked logits, and train_dp.CausalLM packed against padded."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ce_common import IGNORE, ce_ref, f64
from rwkv_lm_ext_amd import callers, train_dp

EINVAL, ENULL, EUNSUPPORTED = -1, -2, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ("bf16", "fp16", "fp32")
FWD_PARAMS = ["long n_rows", "int V", "long ld", "const void* logits", "const long long* targets", "float* loss_row", "float* lse",
              "float* zmax", "int* imax", "const float* ce_scale", "const float* l2_scale", "void* glogits", "long ld_g", "void* stream"]
BWD_PARAMS = ["long n_rows", "int V", "long ld", "const void* logits", "const long long* targets", "const float* lse", "const float* zmax",
              "const int* imax", "const float* ce_scale", "const float* l2_scale", "void* glogits", "long ld_g", "void* stream"]


@pytest.fixture(scope="module")
def lib():
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


def test_symbols_and_signatures(lib):
    from rwkv_lm_ext_amd import _lib
    header = open(os.path.join(ROOT, "include", "wkv6_amd.h")).read()
    I, L, VP = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    for way, params in (("forward", FWD_PARAMS), ("backward", BWD_PARAMS)):
        types = [{"long": L, "int": I}.get(p.rsplit(" ", 1)[0], VP) for p in params]
        for io in TYPES:
            name = f"wkv6_ce_rows_{way}_{io}"
            res, table = _lib.SIGNATURES[name]
            assert res is I and list(table) == types, name
            assert getattr(lib, name).restype is I and list(getattr(lib, name).argtypes) == types
            decl = re.search("int " + name + r"\(([^;]*)\);", header).group(1)
            assert [" ".join(p.split()) for p in decl.split(",")] == params, name


# ---- the C ABI: dummy pointers (never dereferenced: every call below is refused before a launch)
Z, G, P = 1 << 40, 2 << 40, 1 << 30


def fwd_args(n_rows=10, V=100, ld=104, logits=Z, targets=P, loss=P, lse=P, zmax=P, imax=P, ce=P, l2=P, g=G, ld_g=104):
    return (n_rows, V, ld, logits, targets, loss, lse, zmax, imax, ce, l2, g, ld_g, None)


def bwd_args(n_rows=10, V=100, ld=104, logits=Z, targets=P, loss=None, lse=P, zmax=P, imax=P, ce=P, l2=P, g=G, ld_g=104):
    return (n_rows, V, ld, logits, targets, lse, zmax, imax, ce, l2, g, ld_g, None)


@pytest.mark.parametrize("io", TYPES)
@pytest.mark.parametrize("way", ["forward", "backward"])
def test_refusals_and_their_order(lib, way, io):
    fn, args = getattr(lib, f"wkv6_ce_rows_{way}_{io}"), fwd_args if way == "forward" else bwd_args
    es = 4 if io == "fp32" else 2
    # (1) sizes, in front of everything
    for kw in ({"n_rows": 0}, {"n_rows": -3}, {"V": 0}, {"V": -1}, {"ld": 96}, {"ld": 100}, {"ld": 108}, {"ld_g": 96}, {"ld_g": 100},
               {"ld_g": 108}, {"ld_g": 0}):
        assert fn(*args(**kw)) == EINVAL, kw
        assert fn(*args(**dict(kw, logits=None))) == EINVAL, kw
        if "n_rows" not in kw:
            assert fn(*args(**dict(kw, n_rows=1 << 31))) == EINVAL, kw
    # (2) the grid
    assert fn(*args(n_rows=1 << 31)) == EUNSUPPORTED
    assert fn(*args(n_rows=1 << 31, targets=None)) == EUNSUPPORTED
    assert fn(*args(n_rows=(1 << 31) - 1, targets=None)) == ENULL
    # (3) NULL pointers, in front of alignment
    for p in ("logits", "targets", "lse", "zmax", "imax", "ce", "l2") + (("loss",) if way == "forward" else ("g",)):
        assert fn(*args(**{p: None})) == ENULL, p
        assert fn(*args(**{p: None, "logits" if p != "logits" else "targets": Z + 2})) == ENULL, p
    # (4) alignment: 16 bytes for the two row tensors, 8 for the targets, 4 for the rest; then the overlap
    for p, base in (("logits", Z), ("g", G)):
        for off in (1, 2, 4, 8, 12):
            assert fn(*args(**{p: base + off})) == EINVAL, (p, off)
    for off in (1, 2, 4, 6):
        assert fn(*args(targets=P + off)) == EINVAL, off
    for p in ("lse", "zmax", "imax", "ce", "l2") + (("loss",) if way == "forward" else ()):
        for off in (1, 2, 3):
            assert fn(*args(**{p: P + off})) == EINVAL, (p, off)
    assert fn(*args(g=Z, ld_g=112)) == EINVAL                                  # the same buffer with another row stride is no in-place use
    assert fn(*args(g=Z + 16)) == EINVAL
    assert fn(*args(g=Z + 10 * 104 * es - 16)) == EINVAL
    assert fn(*args(logits=G + 10 * 104 * es - 16)) == EINVAL


def test_statistics_only_forward_looks_at_no_gradient_argument(lib):
    """glogits == NULL: ce_scale, l2_scale and ld_g are not judged; what is refused is still refused in order"""
    for io in TYPES:
        fn = getattr(lib, f"wkv6_ce_rows_forward_{io}")
        assert fn(*fwd_args(g=None, ce=None, l2=None, ld_g=0, loss=None)) == ENULL
        assert fn(*fwd_args(g=None, ce=None, l2=None, ld_g=-5, lse=P + 2)) == EINVAL       # the outputs' 4-byte rule, not ld_g
        assert fn(*fwd_args(g=None, ce=P + 1, l2=P + 3, ld_g=-5, targets=None)) == ENULL     # misaligned scales are not what is refused
        assert fn(*fwd_args(g=None, ce=None, l2=None, ld_g=3, n_rows=0)) == EINVAL


def test_ce_rows_refuses_before_calling_the_library(monkeypatch):
    from rwkv_lm_ext_amd import _lib, mix_op

    def no_library(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(mix_op, "_call", no_library)
    good = dict(logits=torch.zeros(6, 16, dtype=torch.bfloat16), targets=torch.zeros(6, dtype=torch.int64), l2=torch.zeros(6))

    def call(**o):
        a = dict(good, **o)
        return mix_op.ce_rows(a["logits"], a["targets"], a["l2"])

    with pytest.raises(RuntimeError, match="must be on the GPU"):                # everything else is right: no CPU path
        call()
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        call(logits=torch.zeros(6, 24)[:, :13], l2=None)                         # a view of a padded tensor is a good shape
    for bad in (good["logits"].double(), good["logits"].to(torch.int32), torch.zeros(96, dtype=torch.bfloat16),
                torch.zeros(2, 3, 16, dtype=torch.bfloat16), torch.zeros(6, 32, dtype=torch.bfloat16)[:, ::2], torch.zeros(0, 16), None):
        with pytest.raises(RuntimeError, match="logits must be"):
            call(logits=bad)
    for bad in (torch.zeros(6, 13), torch.zeros(6, 20), torch.zeros(5 * 16 + 13).as_strided((6, 13), (16, 1))):       # the last row ends short of its ld
        with pytest.raises(RuntimeError, match="multiple of 8"):
            call(logits=bad)
    for bad in (good["targets"].int(), torch.zeros(5, dtype=torch.int64), torch.zeros(12, dtype=torch.int64)[::2], [0] * 6, None):
        with pytest.raises(RuntimeError, match="targets must be"):
            call(targets=bad)
    for bad in (good["l2"].double(), torch.zeros(5), torch.zeros(12)[::2], 0.1):
        with pytest.raises(RuntimeError, match="l2_scale must be"):
            call(l2=bad)
    with pytest.raises(RuntimeError, match="ce_scale must be"):
        mix_op.ce_rows_grad_(good["logits"], good["targets"], torch.zeros(5), good["l2"])
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        mix_op.ce_rows_grad_(good["logits"], good["targets"], good["l2"], good["l2"])
    # callers.lm_loss: kernels=True asks for the kernels and gets their refusal; None and False take the eager path on the CPU
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        callers.lm_loss(good["logits"], good["targets"], kernels=True)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        callers.head_loss(torch.zeros(6, 8), torch.zeros(16, 8), good["targets"], kernels=True)
    assert torch.equal(callers.lm_loss(good["logits"].float(), good["targets"]), callers.lm_loss(good["logits"].float(), good["targets"], kernels=False))


# ---- the eager branch of lm_loss against the reference's three lines
class RefL2Wrap(torch.autograd.Function):
    """src/model.py:960-974; with token_amount src/model.py:937-958 (without WN_FIX_L2WRAP)"""

    @staticmethod
    def forward(ctx, loss, y, token_amount=None):
        ctx.save_for_backward(y)
        ctx.token_amount = token_amount
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        y = ctx.saved_tensors[0]
        factor = 1e-4 / (y.shape[0] * y.shape[1] if ctx.token_amount is None else ctx.token_amount)
        maxx, ids = torch.max(y, -1, keepdim=True)
        gy = torch.zeros_like(y)
        gy.scatter_(-1, ids, maxx * factor)
        return (grad_output, gy, None)


def reference_training_step(logits, targets, mask=None, token_amount=None):
    """src/model.py:1249-1269"""
    if mask is None:
        loss = F.cross_entropy(logits.view(-1, logits.size(-1)), targets.view(-1))
    else:
        mask = mask.view(-1)
        sum_mask = torch.sum(mask).item()
        loss = F.cross_entropy(logits.view(-1, logits.size(-1)), targets.view(-1), reduction="none")
        loss = torch.sum(loss * mask) / sum_mask
    return RefL2Wrap.apply(loss, logits, token_amount)


def lm_problem(B=3, T=11, V=37, seed=0):
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, T, V, generator=gen) * 4
    top = torch.randint(0, V, (B, T, 1), generator=gen)
    logits.scatter_(-1, top, 30.0 + torch.rand(B, T, 1, generator=gen))          # a unique maximum in every row: the tie rule cannot matter
    targets = torch.randint(0, V, (B, T), generator=gen)
    mask = (torch.rand(B, T, generator=gen) < 0.5).float()
    return logits, targets, mask


@pytest.mark.parametrize("form", ["plain", "ignore", "mask", "token_amount", "mask_and_ignore"])
def test_eager_lm_loss_equals_the_reference_three_lines(form):
    logits, targets, mask = lm_problem()
    kw = {}
    if "ignore" in form:
        targets[0, 2:6] = IGNORE
        targets[2, -1] = IGNORE
    if "mask" in form:
        kw["mask"] = mask
    if form == "token_amount":
        kw["token_amount"] = 29
    a, b = logits.clone().requires_grad_(), logits.clone().requires_grad_()
    got, want = callers.lm_loss(a, targets, kernels=False, **kw), reference_training_step(b, targets, **kw)
    assert torch.equal(got, want)
    (got * 0.5).backward()
    (want * 0.5).backward()                                                      # the L2 term is not scaled by the incoming gradient
    assert torch.equal(a.grad, b.grad) and a.grad.abs().sum() > 0
    # a packed [total_T, V] tensor is B = 1: the same rows, the same loss
    c = logits.clone().reshape(-1, logits.shape[-1]).requires_grad_()
    packed_kw = dict(kw, mask=kw["mask"].reshape(-1)) if "mask" in kw else kw
    assert torch.equal(callers.lm_loss(c, targets.reshape(-1), kernels=False, **packed_kw), want)


def test_eager_lm_loss_l2_switches_and_device_counts():
    logits, targets, _ = lm_problem(seed=1)
    grads = {}
    for name, kw in (("on", {}), ("off", {"l2wrap": 0.0}), ("tensor", {"token_amount": torch.tensor(29)}), ("int", {"token_amount": 29}),
                     ("zero", {"token_amount": 0})):
        z = logits.clone().requires_grad_()
        callers.lm_loss(z, targets, kernels=False, **kw).backward()
        grads[name] = z.grad
    assert torch.equal(grads["tensor"], grads["int"]) and torch.equal(grads["zero"], grads["off"])
    assert not torch.equal(grads["on"], grads["off"]) and not torch.equal(grads["on"], grads["int"])
    rows = torch.zeros(logits.shape[:2])
    rows[1] = 1
    z = logits.clone().requires_grad_()
    callers.lm_loss(z, targets, kernels=False, l2_rows=rows).backward()
    assert torch.equal(z.grad[1], grads["on"][1]) and torch.equal(z.grad[0], grads["off"][0]) and torch.equal(z.grad[2], grads["off"][2])


def test_eager_chunk_step_against_fp64():
    """callers._ce_rows_grad_eager restates the fused kernel: judged by the oracle that judges the kernel"""
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(9, 50, generator=gen) * 4
    t = torch.randint(0, 50, (9,), generator=gen)
    t[4] = IGNORE
    ce, l2 = torch.rand(9, generator=gen) + 0.5, torch.rand(9, generator=gen) * 1e-2
    loss, g = callers._ce_rows_grad_eager(z, t, ce, l2)
    ref = ce_ref(f64(z), t.numpy(), ce.numpy(), l2.numpy())
    assert np.abs(f64(loss) - ref["loss"]).max() <= 1e-5
    assert (np.abs(f64(g) - ref["g"]) <= 2e-5 * np.abs(ref["g"]) + 1e-7 * f64(ce)[:, None]).all()


# ---- head_loss: the chunked head against lm_loss on the unchunked logits
@pytest.mark.parametrize("chunk_rows", [7, 30, 4096])
@pytest.mark.parametrize("form", ["plain", "mask", "token_amount", "no_l2"])
def test_head_loss_equals_lm_loss_on_the_logits(form, chunk_rows):
    gen = torch.Generator().manual_seed(11)
    rows, C, V = 30, 16, 37                                                      # V no multiple of 8: the buffer's rows are padded
    x, W = torch.randn(rows, C, generator=gen), torch.randn(V, C, generator=gen) * 0.5
    targets = torch.randint(0, V, (rows,), generator=gen)
    targets[3] = IGNORE
    kw = {"mask": {"mask": (torch.rand(rows, generator=gen) < 0.5).float()}, "token_amount": {"token_amount": 19}, "no_l2": {"l2wrap": 0.0}}.get(form, {})
    if form == "plain":
        kw = {"l2wrap": 0.05}                                                    # large enough to show in the gradients
    xa, Wa = x.clone().requires_grad_(), W.clone().requires_grad_()
    got = callers.head_loss(xa, Wa, targets, chunk_rows=chunk_rows, kernels=False, **kw)
    got.backward()
    xb, Wb = x.clone().requires_grad_(), W.clone().requires_grad_()
    want = callers.lm_loss(xb @ Wb.t(), targets, kernels=False, **kw)
    want.backward()
    assert abs(float(got.detach()) - float(want.detach())) <= 1e-6 * abs(float(want.detach()))
    assert (xa.grad - xb.grad).abs().max() <= 1e-6 * xb.grad.abs().max()
    assert (Wa.grad - Wb.grad).abs().max() <= 1e-6 * Wb.grad.abs().max()


def test_head_loss_skips_the_weight_gemm_for_a_frozen_head_and_scales_by_the_incoming_gradient(monkeypatch):
    calls = []
    gemm = callers._gw_gemm
    monkeypatch.setattr(callers, "_gw_gemm", lambda g, x, out: calls.append(g.shape) or gemm(g, x, out))
    gen = torch.Generator().manual_seed(12)
    x, W = torch.randn(3, 10, 16, generator=gen), torch.randn(24, 16, generator=gen)
    targets = torch.randint(0, 24, (3, 10), generator=gen)
    xa = x.clone().requires_grad_()
    callers.head_loss(xa, W, targets, chunk_rows=8, kernels=False).backward()
    assert calls == [] and xa.grad.shape == x.shape
    xb, Wb = x.clone().requires_grad_(), W.clone().requires_grad_()
    (callers.head_loss(xb, Wb, targets, chunk_rows=8, kernels=False, l2wrap=0.0) * 3.0).backward()
    assert len(calls) == 4                                                       # 30 rows in chunks of 8
    xc = x.clone().requires_grad_()
    callers.head_loss(xc, W, targets, chunk_rows=8, kernels=False, l2wrap=0.0).backward()
    assert torch.allclose(xb.grad, 3.0 * xc.grad, rtol=1e-6, atol=0) and Wb.grad is not None
    # a trainable head behind a hidden state that takes no gradient
    Wd = W.clone().requires_grad_()
    callers.head_loss(x, Wd, targets, chunk_rows=8, kernels=False, l2wrap=0.0).backward()
    assert torch.allclose(Wd.grad * 3.0, Wb.grad, rtol=1e-5, atol=1e-7)
    with pytest.raises(RuntimeError, match="weight must be"):
        callers.head_loss(x, W.double(), targets)
    with pytest.raises(RuntimeError, match="one entry per row"):
        callers.head_loss(x, W, targets[:, :5])


# ---- CausalLM on the CPU route: packed against padded
def lm_batch(V=64, T=24, lengths=(24, 9, 17), seed=0):
    gen = torch.Generator().manual_seed(seed)
    idx = torch.randint(2, V, (len(lengths), T), generator=gen)
    targets = torch.randint(0, V, (len(lengths), T), generator=gen)
    for b, n in enumerate(lengths):
        idx[b, n:] = 0
        targets[b, n:] = IGNORE
    return idx, targets, torch.tensor(lengths)


def test_pack_lm_rows():
    idx, targets, lengths = lm_batch()
    pidx, ptgt, cu, max_seqlen = train_dp.pack_lm_rows(idx, targets, lengths, total_multiple=16)
    assert pidx.shape == ptgt.shape == (1, 64) and cu.dtype == torch.int32 and cu.tolist() == [0, 24, 33, 50] and max_seqlen == 24
    assert torch.equal(pidx[0, 24:33], idx[1, :9]) and torch.equal(ptgt[0, 33:50], targets[2, :17])
    assert (ptgt[0, 50:] == IGNORE).all() and (pidx[0, 50:] == 0).all()
    assert train_dp.pack_lm_rows(idx, targets, lengths)[0].shape == (1, 50)


def test_causal_lm_packed_against_padded_on_the_cpu_route():
    """At l2wrap = 0 the packed loss is the padded loss (the padded rows are ignored, the operator is causal).  With L2Wrap on, the two
    differ by design: the dense form regularises the pad rows too and divides by B * T, the packed form by the tokens that exist."""
    from test_train_dp_cpu import _naive_wkv as eager_wkv
    from test_train_packed_cpu import _naive_wkv_varlen as eager_wkv_varlen
    torch.manual_seed(0)
    V = 64
    model = train_dp.CausalLM(V, 64, 2, wkv=eager_wkv, wkv_varlen=eager_wkv_varlen)
    with torch.no_grad():                       # non-trivial time-mix parameters (the module zero-initialises them)
        for n, p in model.named_parameters():
            if "time_" in n or "ln_x" in n:
                p.copy_(torch.randn_like(p) * 0.1)
            if "time_decay" in n and p.dim() == 3:
                p.sub_(3.0)
    idx, targets, lengths = lm_batch(V)
    pidx, ptgt, cu, max_seqlen = train_dp.pack_lm_rows(idx, targets, lengths, total_multiple=8)
    grads = {}
    for l2wrap in (0.0, 1e-2):
        for route in ("padded", "packed"):
            model.zero_grad(set_to_none=True)
            if route == "padded":
                loss = train_dp.lm_training_loss(model, idx, targets, chunk_rows=20, l2wrap=l2wrap)
            else:
                loss = train_dp.lm_training_loss(model, pidx, ptgt, cu_seqlens=cu, max_seqlen=max_seqlen, chunk_rows=20, l2wrap=l2wrap)
            loss.backward()
            grads[l2wrap, route] = (loss.detach(), model.head.weight.grad.clone(), model.emb.weight.grad.clone())
    a, b = grads[0.0, "padded"], grads[0.0, "packed"]
    assert abs(float(a[0]) - float(b[0])) <= 1e-5 * abs(float(a[0]))
    for ga, gb in zip(a[1:], b[1:]):
        assert (ga - gb).abs().max() <= 1e-4 * ga.abs().max()
    # L2Wrap leaves the loss alone and moves the gradients, differently on the two routes
    c, d = grads[1e-2, "padded"], grads[1e-2, "packed"]
    assert torch.equal(c[0], a[0]) and torch.equal(d[0], b[0])
    assert (c[1] - a[1]).abs().max() > 1e-6 and (d[1] - b[1]).abs().max() > 1e-6
    assert (c[1] - d[1]).abs().max() > 1e-3 * (c[1] - a[1]).abs().max()
