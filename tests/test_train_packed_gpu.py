"""The packed training step on the HIP path: the 2-layer bf16 LoRA model of test_train_dp_gpu.py fed one packed batch
(train_dp.batches(packed=True)) -- packed WKV6 operator, packed token-shift kernels, packed pooling kernels -- against the SAME bf16 model on
the CPU run DENSE on the padded rows (eager torch, the pure-PyTorch port of the reference's CPU recurrence as the operator), which is the
reference test_train_dp_gpu.py uses, with that file's tolerances: loss 1e-2 absolute, every trainable gradient 4e-2 max-normalised.

Measured on an MI355X, the same figures for total_multiple 1, 64 and 64 with checkpointing (the rows behind the last sequence and the
recomputation change no bit of the result): packed against the CPU reference, loss 9.5e-3 off and the worst gradient 1.9e-2; packed against
the dense step on the HIP path, loss 3.5e-3 off and the worst gradient 1.0e-2 -- the size of the dense HIP step's own distance from the
reference (4e-3 / 2.2e-2, test_train_dp_gpu.py): the two HIP steps run their GEMMs and LayerNorms on different row counts, so rocBLAS sums
in another order and a 2-layer bf16 network's roundings fall differently; nothing is systematically off.  The loss sits close to its bound;
each case prints its figures."""
import pytest
import torch

from rwkv_lm_ext_amd import callers, train_dp
from rwkv_lm_ext_amd.dp import BucketBatchSampler
from test_train_dp_cpu import BS, T, VOCAB, N_LAYER, _model, _naive_wkv

pytestmark = pytest.mark.gpu


def _sampler():
    return BucketBatchSampler([4 * BS], [BS], 0, 1)


def _step(model, batch, device):
    batch = train_dp.to_device(batch, device)
    loss = train_dp.training_loss(model, batch) if "idx" in batch else train_dp.training_loss(model, batch["query"], batch["positive"],
                                                                                              batch["negative"])
    loss.backward()
    return float(loss.detach()), {n: p.grad.float().cpu() for n, p in model.named_parameters() if p.requires_grad}


def _hip_model(grad_cp=False):
    m = _model()                                                            # same seed -> same weights
    for blk in m.blocks:                                                    # the HIP operators and the fused kernels
        blk.att.wkv = callers._default_wkv
    m.grad_cp = grad_cp
    return m.to("cuda", torch.bfloat16)


@pytest.fixture(scope="module")
def reference():
    """the bf16 CPU model, dense, on the padded rows (computed once)"""
    ref_model = _model().to(torch.bfloat16)
    for m in ref_model.modules():                                           # torch's CPU norms take bf16 inputs with fp32 parameters only
        if isinstance(m, (torch.nn.GroupNorm, torch.nn.LayerNorm)):
            m.float()
    for blk in ref_model.blocks:                                            # the operator returns y in the I/O type (bf16), as the HIP one does
        blk.att.wkv = lambda *a: _naive_wkv(*a).to(torch.bfloat16)
    return _step(ref_model, next(iter(train_dp.batches(_sampler(), T, VOCAB))), "cpu")


@pytest.fixture(scope="module")
def dense_hip():
    return _step(_hip_model(), next(iter(train_dp.batches(_sampler(), T, VOCAB))), "cuda")


@pytest.mark.parametrize("total_multiple,grad_cp", [(1, False), (64, False), (64, True)])
def test_packed_training_step_on_the_hip_path(reference, dense_hip, total_multiple, grad_cp):
    assert torch.cuda.is_available()
    loss_ref, g_ref = reference
    model = _hip_model(grad_cp)
    assert model.training
    for blk in model.blocks:                                                # the packed operator is the HIP default, nothing stands in for it
        assert blk.att.wkv_varlen is callers._default_wkv_varlen and blk.att.wkv is callers._default_wkv
        assert blk.att._use_fused(torch.empty(1, 8, 128, device="cuda", dtype=torch.bfloat16))
    batch = next(iter(train_dp.batches(_sampler(), T, VOCAB, packed=True, total_multiple=total_multiple)))
    assert (int(batch["cu_seqlens"][-1]) < batch["idx"].shape[1]) == (total_multiple > 1)
    loss, g = _step(model, batch, "cuda")
    loss_hip, g_hip = dense_hip
    worst_hip = max(float((g[n] - g_hip[n]).abs().max() / g_hip[n].abs().max()) for n in g_hip)
    print(f"packed vs dense HIP: loss {abs(loss - loss_hip):.2e}, worst gradient {worst_hip:.2e}; "
          f"packed vs CPU reference: loss {abs(loss - loss_ref):.2e}")
    assert abs(loss - loss_ref) <= 1e-2, (loss, loss_ref)
    names = sorted(g_ref)
    assert names == sorted(g) and len(names) >= 2 * 3 * N_LAYER + 2
    worst = {}
    for n in names:
        a, b = g[n], g_ref[n]
        assert float(b.abs().max()) > 0, n
        worst[n] = float((a - b).abs().max() / b.abs().max())
    print(f"packed vs CPU reference: worst gradient {max(worst.values()):.2e}")
    bad = {n: e for n, e in worst.items() if e > 4e-2}
    assert not bad, bad
