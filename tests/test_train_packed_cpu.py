"""The packed route through the LoRA sentence-embedding model (train_dp.pack_rows, Block / SequenceEmbedder with cu_seqlens,
batches(packed=True), training_loss on a packed batch), CPU tier: the 2-layer fp32 model of test_train_dp_cpu.py, the token shift and the
pooling on their eager paths, and the pure-PyTorch port of the reference's CPU recurrence (oracle/, test infrastructure) standing in for
the operator through both hooks of the time-mix.  Expectation: the dense step on the same rows -- what the packed step leaves out is
padding behind the emb_id token, which the causal model never lets reach the pooled vector."""
import numpy as np
import pytest
import torch

from oracle.contract import F32_TOL, max_norm_err
from rwkv_lm_ext_amd import train_dp
from rwkv_lm_ext_amd.dp import BucketBatchSampler
from test_train_dp_cpu import BS, T, VOCAB, N_LAYER, _model, _naive_wkv


def _naive_wkv_varlen(total_T, C, H, r, k, v, w, u, cu_seqlens, max_seqlen):
    """every sequence alone through the naive operator; rows behind the last sequence (a total_multiple gap) come back zero, as the HIP
    operator writes them"""
    cu = cu_seqlens.tolist()
    assert cu[0] == 0 and cu[-1] <= total_T and max_seqlen == max(b - a for a, b in zip(cu, cu[1:]))
    parts = [_naive_wkv(1, b - a, C, H, *(t[:, a:b] for t in (r, k, v, w)), u) for a, b in zip(cu, cu[1:]) if b > a]
    return torch.cat(parts + [r.new_zeros(1, total_T - cu[-1], C)], 1)


def packed_model(**kw):
    m = _model()
    for blk in m.blocks:
        blk.att.wkv_varlen = _naive_wkv_varlen
    for k_, v_ in kw.items():
        setattr(m, k_, v_)
    return m


def sampler():
    return BucketBatchSampler([4 * BS], [BS], 0, 1)


def step(model, batch):
    model.zero_grad()
    loss = train_dp.training_loss(model, batch) if "idx" in batch else train_dp.training_loss(model, batch["query"], batch["positive"],
                                                                                              batch["negative"])
    loss.backward()
    return loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.requires_grad}


@pytest.fixture(scope="module")
def dense():
    return step(packed_model(), next(iter(train_dp.batches(sampler(), T, VOCAB))))


def test_pack_rows():
    idx = torch.tensor([[5, 6, 1, 0, 0, 0],        # ordinary: tokens, emb_id, padding
                        [1, 9, 9, 0, 0, 0],        # emb_id at position 0: one token
                        [5, 6, 7, 8, 9, 4],        # no emb_id: argmax gives 0, one token
                        [2, 3, 4, 5, 6, 1],        # a full row
                        [7, 1, 8, 1, 0, 0]])       # two emb_id: the first counts
    flat, cu, max_seqlen, actual = train_dp.pack_rows(idx, emb_id=1)
    assert flat.tolist() == [[5, 6, 1, 1, 5, 2, 3, 4, 5, 6, 1, 7, 1]] and flat.dtype == idx.dtype
    assert cu.tolist() == [0, 3, 4, 5, 11, 13] and cu.dtype == torch.int32
    assert actual.tolist() == [2, 0, 0, 5, 1] and actual.dtype == torch.int32
    assert max_seqlen == 6 and isinstance(max_seqlen, int)
    for mult, total in ((1, 13), (13, 13), (4, 16), (64, 64)):
        f, c, m, a = train_dp.pack_rows(idx, emb_id=1, total_multiple=mult, pad_id=0)
        assert f.shape == (1, total) and f[0, :13].tolist() == flat[0].tolist() and (f[0, 13:] == 0).all()
        assert c.tolist() == cu.tolist() and a.tolist() == actual.tolist() and m == 6         # the gap belongs to no sequence
    f, _, _, _ = train_dp.pack_rows(idx, emb_id=1, total_multiple=8, pad_id=3)
    assert f[0, 13:].tolist() == [3, 3, 3]
    f, c, m, a = train_dp.pack_rows(idx, emb_id=4)                                             # another marker
    assert c.tolist() == [0, 1, 2, 8, 11, 12] and a.tolist() == [0, 0, 5, 2, 0] and m == 6


def test_packed_batches_hold_the_dense_batches_rows():
    d = next(iter(train_dp.batches(sampler(), T, VOCAB)))
    p = next(iter(train_dp.batches(sampler(), T, VOCAB, packed=True)))
    rows = torch.cat([d["query"], d["positive"], d["negative"]])
    assert p["bs"] == BS and p["cu_seqlens"].numel() == 3 * BS + 1 and p["idx"].shape == (1, int(p["cu_seqlens"][-1]))
    assert p["max_seqlen"] == int((p["cu_seqlens"][1:] - p["cu_seqlens"][:-1]).max()) <= T
    for s in range(3 * BS):
        a, b = int(p["cu_seqlens"][s]), int(p["cu_seqlens"][s + 1])
        assert torch.equal(p["idx"][0, a:b], rows[s, :b - a]) and rows[s, b - a - 1] == 1 and int(p["actual_len"][s]) == b - a - 1
    p64 = next(iter(train_dp.batches(sampler(), T, VOCAB, packed=True, total_multiple=64)))
    assert p64["idx"].shape[1] % 64 == 0 and torch.equal(p64["cu_seqlens"], p["cu_seqlens"])
    assert int(p64["cu_seqlens"][-1]) < p64["idx"].shape[1]                                   # this batch does leave a gap


@pytest.mark.parametrize("total_multiple", [1, 64])
def test_packed_step_equals_the_dense_step(dense, total_multiple):
    loss_d, g_d = dense
    batch = next(iter(train_dp.batches(sampler(), T, VOCAB, packed=True, total_multiple=total_multiple)))
    loss_p, g_p = step(packed_model(), batch)
    assert abs(float(loss_p) - float(loss_d)) <= F32_TOL * max(1.0, abs(float(loss_d))), (float(loss_p), float(loss_d))
    assert sorted(g_p) == sorted(g_d) and len(g_p) >= 2 * 3 * N_LAYER + 2
    for n in g_d:
        assert float(g_d[n].abs().max()) > 0, n
        assert max_norm_err(g_p[n].numpy(), g_d[n].numpy(), floor=0.0) <= F32_TOL, (n, max_norm_err(g_p[n].numpy(), g_d[n].numpy(), floor=0.0))


def test_checkpointing_passes_the_packed_arguments_through():
    batch = next(iter(train_dp.batches(sampler(), T, VOCAB, packed=True, total_multiple=64)))
    loss_a, g_a = step(packed_model(grad_cp=False), batch)
    m = packed_model(grad_cp=True)
    assert m.training
    loss_b, g_b = step(m, batch)
    assert torch.equal(loss_a, loss_b)
    for n in g_a:
        assert torch.equal(g_a[n], g_b[n]), n


def test_ddp_takes_the_packed_shape_and_the_keyword_arguments(tmp_path):
    """a one-rank gloo group in this process (file store, no port): DDP forwards the packed batch's keyword arguments, its hooks run through
    the [1,total_T,C] LoRA layers, and the reduced gradients are the un-wrapped step's"""
    import torch.distributed as dist
    batch = next(iter(train_dp.batches(sampler(), T, VOCAB, packed=True, total_multiple=64)))
    loss_a, g_a = step(packed_model(), batch)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0, world_size=1)
    try:
        m = packed_model()
        loss_b = train_dp.training_loss(train_dp.wrap_ddp(m), batch)
        loss_b.backward()
        assert torch.equal(loss_a, loss_b.detach())
        for n, p in m.named_parameters():
            if p.requires_grad:
                assert torch.equal(g_a[n], p.grad), n
    finally:
        dist.destroy_process_group()


def test_train_steps_takes_packed_batches_and_the_dense_path_is_untouched():
    m = packed_model()
    opt = torch.optim.SGD(train_dp.trainable_parameters(m), lr=0.0)
    losses = train_dp.train_steps(m, opt, train_dp.batches(sampler(), T, VOCAB, packed=True), "cpu", 2)
    want = train_dp.train_steps(m, opt, train_dp.batches(sampler(), T, VOCAB), "cpu", 2)
    assert len(losses) == 2
    for a, b in zip(losses, want):
        assert abs(float(a) - float(b)) <= F32_TOL * max(1.0, abs(float(b)))
    idx = next(iter(train_dp.batches(sampler(), T, VOCAB)))["query"]
    with torch.no_grad():
        assert torch.equal(m(idx), m(idx, cu_seqlens=None, max_seqlen=None, actual_len=None))
        x = m.emb(idx)
        assert torch.equal(m.blocks[0](x), m.blocks[0](x, None, None))
