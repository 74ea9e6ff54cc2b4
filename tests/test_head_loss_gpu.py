"""The chunked LM head on the HIP path (callers.head_loss over mix_op.ce_rows_grad_) and train_dp.CausalLM through it.

head_loss at rows = 300, C = 128, V = 1000 with chunk_rows 64 (a last chunk of 44 rows), 300 and 4096 against callers.lm_loss on the
unchunked logits: the loss to 1e-5 relative against the kernels' own lm_loss, x.grad and W.grad to 2^-7 of the largest reference entry
(bf16 rounding of a 300-term sum) against the eager three lines.  The eager lines are given the bf16 logits of the same GEMM held in fp32:
on bf16 tensors they round the log-softmax to bf16, percents of p, which is their error and not the head's.
CausalLM (2 layers, C = 128, V = 512) packed against padded at l2wrap = 0: losses within 2e-3 relative (bf16 through two blocks)."""
import pytest
import torch

from ce_common import IGNORE
from rwkv_lm_ext_amd import callers, train_dp

pytestmark = pytest.mark.gpu

ROWS, C, V = 300, 128, 1000
BF = torch.bfloat16


@pytest.fixture(scope="module")
def head():
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(ROWS, C, generator=gen).to(BF).cuda()
    W = (torch.randn(V, C, generator=gen) * 0.3).to(BF).cuda()
    targets = torch.randint(0, V, (ROWS,), generator=gen).cuda()
    targets[5::17] = IGNORE
    mask = (torch.rand(ROWS, generator=gen) < 0.7).float().cuda()
    return x, W, targets, mask


@pytest.fixture(scope="module")
def eager(head):
    """{form: (loss, x.grad, W.grad)} of the eager three lines on the unchunked logits, computed once"""
    x, W, targets, mask = head
    out = {}
    for form, kw in (("plain", {}), ("mask", {"mask": mask})):
        xr, Wr = x.clone().requires_grad_(), W.clone().requires_grad_()
        loss = callers.lm_loss((xr @ Wr.t()).float(), targets, kernels=False, **kw)
        loss.backward()
        out[form] = (float(loss.detach()), xr.grad.float(), Wr.grad.float())
    return out


@pytest.mark.parametrize("chunk_rows", [64, 300, 4096])
@pytest.mark.parametrize("form", ["plain", "mask"])
def test_head_loss_against_the_unchunked_logits(head, eager, form, chunk_rows):
    x, W, targets, mask = head
    kw = {"mask": mask} if form == "mask" else {}
    xr, Wr = x.clone().requires_grad_(), W.clone().requires_grad_()
    loss = callers.head_loss(xr, Wr, targets, chunk_rows=chunk_rows, kernels=True, **kw)
    loss.backward()
    unchunked = float(callers.lm_loss(x @ W.t(), targets, kernels=True, **kw))
    want, gx, gW = eager[form]
    print(f"loss {float(loss.detach()):.7f}, unchunked kernels {unchunked:.7f}, eager {want:.7f}; "
          f"x.grad {float((xr.grad.float() - gx).abs().max() / gx.abs().max()):.2e}, "
          f"W.grad {float((Wr.grad.float() - gW).abs().max() / gW.abs().max()):.2e} of the largest entry")
    assert abs(float(loss.detach()) - unchunked) <= 1e-5 * abs(unchunked)
    assert abs(float(loss.detach()) - want) <= 1e-5 * abs(want)
    assert (xr.grad.float() - gx).abs().max() <= 2.0 ** -7 * gx.abs().max()
    assert (Wr.grad.float() - gW).abs().max() <= 2.0 ** -7 * gW.abs().max()
    assert xr.grad.dtype == BF and Wr.grad.dtype == BF and xr.grad.shape == x.shape and Wr.grad.shape == W.shape


def test_a_frozen_head_takes_no_gradient_and_runs_no_weight_gemm(head, monkeypatch):
    x, W, targets, _ = head
    calls = []
    gemm = callers._gw_gemm
    monkeypatch.setattr(callers, "_gw_gemm", lambda g, xc, out: calls.append(tuple(g.shape)) or gemm(g, xc, out))
    xr, Wf = x.clone().requires_grad_(), W.clone()
    callers.head_loss(xr, Wf, targets, chunk_rows=64, kernels=True).backward()
    assert Wf.grad is None and calls == [] and xr.grad.isfinite().all()
    Wr = W.clone().requires_grad_()
    xt = x.clone().requires_grad_()
    callers.head_loss(xt, Wr, targets, chunk_rows=64, kernels=True).backward()
    assert calls == [(64, V)] * 4 + [(44, V)]                                    # the non-dividing last chunk
    assert torch.equal(xt.grad, xr.grad)


def test_kernels_none_is_eager_where_the_kernels_do_not_apply(head):
    """a GPU tensor in a type the kernels do not serve takes the eager chunk step under None, and the kernels' refusal under True"""
    x, W, targets, _ = head
    x64, W64 = x.double(), W.double()
    assert torch.equal(callers.head_loss(x64, W64, targets, chunk_rows=64), callers.head_loss(x64, W64, targets, chunk_rows=64, kernels=False))
    with pytest.raises(RuntimeError, match="logits must be"):
        callers.head_loss(x64, W64, targets, chunk_rows=64, kernels=True)
    z = x64 @ W64.t()
    assert torch.equal(callers.lm_loss(z, targets), callers.lm_loss(z, targets, kernels=False))


# ---- CausalLM
N_LAYER, VOCAB, T, LENGTHS = 2, 512, 64, (64, 23, 40, 7)


def _lm():
    torch.manual_seed(77)
    m = train_dp.CausalLM(VOCAB, C, N_LAYER)
    with torch.no_grad():                       # non-trivial time-mix parameters (the module zero-initialises them)
        for n, p in m.named_parameters():
            if "time_" in n or "ln_x" in n:
                p.copy_(torch.randn_like(p) * 0.1)
            if "time_decay" in n and p.dim() == 3:
                p.sub_(3.0)
    return m.to("cuda", BF)


def _lm_batch():
    gen = torch.Generator().manual_seed(78)
    idx = torch.randint(2, VOCAB, (len(LENGTHS), T), generator=gen)
    targets = torch.randint(0, VOCAB, (len(LENGTHS), T), generator=gen)
    for b, n in enumerate(LENGTHS):
        idx[b, n:] = 0
        targets[b, n:] = IGNORE
    return idx, targets


def test_causal_lm_packed_against_padded():
    model = _lm()
    for blk in model.blocks:
        assert blk.att.wkv_varlen is callers._default_wkv_varlen and blk.att.wkv is callers._default_wkv
    idx, targets = _lm_batch()
    pidx, ptgt, cu, max_seqlen = train_dp.pack_lm_rows(idx, targets, LENGTHS, total_multiple=64)
    assert int(cu[-1]) < pidx.shape[1]                                           # rows behind the last sequence
    dense = train_dp.lm_training_loss(model, idx.cuda(), targets.cuda(), chunk_rows=100, l2wrap=0.0)
    packed = train_dp.lm_training_loss(model, pidx.cuda(), ptgt.cuda(), cu_seqlens=cu.cuda(), max_seqlen=max_seqlen, chunk_rows=100, l2wrap=0.0)
    dense, packed = dense.detach(), packed.detach()
    print(f"dense {float(dense):.5f}, packed {float(packed):.5f}")
    assert dense.isfinite() and abs(float(packed) - float(dense)) <= 2e-3 * abs(float(dense))


def test_one_optimizer_step_runs_and_its_gradients_are_finite():
    model = _lm()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    idx, targets = _lm_batch()
    pidx, ptgt, cu, max_seqlen = train_dp.pack_lm_rows(idx, targets, LENGTHS, total_multiple=64)
    before = model.head.weight.detach().clone()
    loss = train_dp.lm_training_loss(model, pidx.cuda(), ptgt.cuda(), cu_seqlens=cu.cuda(), max_seqlen=max_seqlen, chunk_rows=100)
    loss.backward()
    grads = {n: p.grad for n, p in model.named_parameters()}
    assert loss.isfinite() and all(g is not None and g.isfinite().all() for g in grads.values()), [n for n, g in grads.items() if g is None]
    assert grads["head.weight"].abs().sum() > 0 and grads["emb.weight"].abs().sum() > 0
    opt.step()
    assert not torch.equal(model.head.weight, before) and model.head.weight.isfinite().all()
