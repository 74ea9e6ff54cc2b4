"""Data-parallel LoRA training step of the sentence-embedding model around the WKV6 operator (BASELINE configs[3]).

What the reference runs (peft_train/peft_train_bi_encoder.py): RWKV-x060 backbone, LoRA r=8 alpha=32 injected into
`ffn.key / ffn.value / ffn.receptance` (:152-154, :252-264), `RwkvForSequenceEmbedding` on top
(src/model_ext.py:1690-1769: backbone -> ln_out -> pooling at the first `emb_id` -> optional dense+tanh), loss =
in-batch-negative InfoNCE over cat[query, positive, negative] (src/model_ext.py:1882-1911; negatives are per rank
only), Lightning + DeepSpeed ZeRO-2 for the gradient reduction over NCCL, and `MyBatchSampler` dealing rank-strided
slices of each length bucket (data/custom_datasets.py:19-74).

Here: the same modules restated on `callers.py`, `torch.nn.parallel.DistributedDataParallel` over the `nccl` backend
(= RCCL over xGMI on ROCm) for the one collective of the path -- the all-reduce of the trainable (LoRA / dense)
gradients, 13-28 MB per step for the 1B6 model, one or two buckets overlapped with the backward -- and
`dp.BucketBatchSampler` for the dealing.  Nothing else of the reference's trainer is rebuilt.
"""
import math
from typing import Iterable, List, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import callers
from .dp import BucketBatchSampler


class LoraLinear(nn.Module):
    """src/rwkvLinear.py:40-97: y = x W^T + (alpha / r) * dropout(x) A^T B^T with W frozen, B zero-initialised
    (peft's LoraLayer has the same forward; the reference injects it through peft, :252-264)."""

    def __init__(self, in_features: int, out_features: int, r: int = 8, alpha: float = 32.0, dropout: float = 0.0):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_features, in_features), requires_grad=False)
        self.lora_A = nn.Parameter(torch.empty(r, in_features))
        self.lora_B = nn.Parameter(torch.zeros(out_features, r))
        self.lora_dropout = nn.Dropout(dropout)
        self.scaling = alpha / r
        self.r = r
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        nn.init.kaiming_uniform_(self.lora_A, a=math.sqrt(5))

    @classmethod
    def from_linear(cls, lin: nn.Linear, r: int, alpha: float, dropout: float) -> "LoraLinear":
        assert lin.bias is None, "Biased LoraLinear not supported"          # src/rwkvLinear.py:46
        m = cls(lin.in_features, lin.out_features, r, alpha, dropout).to(lin.weight.device, lin.weight.dtype)
        with torch.no_grad():
            m.weight.copy_(lin.weight)
        return m

    def forward(self, x):
        # fused path: bf16 everywhere, no dropout, and a FROZEN base weight (the reference's trainer freezes it; a caller that trains
        # it gets the eager path, whose autograd produces the weight gradient the fused backward does not)
        if (x.is_cuda and self.lora_dropout.p == 0.0 and not self.weight.requires_grad
                and x.dtype == self.weight.dtype == self.lora_A.dtype == self.lora_B.dtype == torch.bfloat16):
            return _LoraLinearFn.apply(x, self.weight, self.lora_A, self.lora_B, self.scaling)
        return F.linear(x, self.weight) + self.scaling * F.linear(F.linear(self.lora_dropout(x), self.lora_A), self.lora_B)


class _LoraLinearFn(torch.autograd.Function):
    """y = x W^T + s (x A^T) B^T with the low-rank term added in the second GEMM's epilogue (addmm_, beta = 1: one rounding of
    the sum) instead of a separate elementwise add over [rows, out] -- at the 1B6 shape those adds were 10.7 % of the training
    step's kernel time (profiles/r03_dp_lora_kernel_shares.txt).  Backward likewise: gx = gy W, then += s (gy B) A in a GEMM
    epilogue; gA, gB from the rank-r intermediates; nothing of size [rows, out] is kept for it besides x (as F.linear keeps)."""

    @staticmethod
    def forward(ctx, x, weight, lora_A, lora_B, scaling):
        x2 = x.reshape(-1, x.shape[-1])
        xa = x2 @ lora_A.t()                                       # [rows, r]
        y = x2 @ weight.t()
        y.addmm_(xa, lora_B.t(), alpha=scaling)
        ctx.save_for_backward(x2, weight, lora_A, lora_B, xa)
        ctx.scaling, ctx.shape = scaling, x.shape
        return y.view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, gy):
        x2, weight, lora_A, lora_B, xa = ctx.saved_tensors
        s = ctx.scaling
        gy2 = gy.reshape(-1, gy.shape[-1])
        gyb = gy2 @ lora_B                                          # [rows, r]
        gx = gA = gB = None
        if ctx.needs_input_grad[0]:
            gx = gy2 @ weight
            gx.addmm_(gyb, lora_A, alpha=s)
            gx = gx.view(ctx.shape)
        if ctx.needs_input_grad[2]:
            gA = (gyb.t() @ x2) * s
        if ctx.needs_input_grad[3]:
            gB = (gy2.t() @ xa) * s
        return gx, None, gA, gB, None


def inject_lora(model: nn.Module, targets: Sequence[str] = ("ffn.key", "ffn.value", "ffn.receptance"), r: int = 8,
                alpha: float = 32.0, dropout: float = 0.0) -> List[str]:
    """Freeze `model`, replace every nn.Linear whose qualified name ends with one of `targets` by a LoraLinear
    (peft.inject_adapter_in_model with LoraConfig(target_modules=...), peft_train_bi_encoder.py:252-264).
    Returns the names of the replaced modules."""
    for p in model.parameters():
        p.requires_grad_(False)
    replaced = []
    for name, mod in list(model.named_modules()):
        for child_name, child in list(mod.named_children()):
            full = f"{name}.{child_name}" if name else child_name
            if isinstance(child, nn.Linear) and any(full.endswith(t) for t in targets):
                setattr(mod, child_name, LoraLinear.from_linear(child, r, alpha, dropout))
                replaced.append(full)
    return replaced


class Block(nn.Module):
    """Causal RWKV-6 block (src/model.py:904-933 without dropout / tiny-att): x + att(ln1 x), x + ffn(ln2 x)."""

    def __init__(self, n_embd, dim_att, dim_ffn, layer_id, wkv=None, wkv_varlen=None):
        super().__init__()
        self.layer_id = layer_id
        self.ln1 = nn.LayerNorm(n_embd)
        self.ln2 = nn.LayerNorm(n_embd)
        if layer_id == 0:
            self.ln0 = nn.LayerNorm(n_embd)
        self.att = callers.Tmix_x060(n_embd, dim_att, wkv=wkv, wkv_varlen=wkv_varlen)
        self.ffn = callers.CMix_x060(n_embd, dim_ffn)

    def forward(self, x, cu_seqlens=None, max_seqlen=None):
        """cu_seqlens (int32 [n_seq + 1] on the device of x) / max_seqlen: x is a packed batch [1,total_T,C] (callers.Tmix_x060.forward)."""
        if self.layer_id == 0:
            x = self.ln0(x)
        if cu_seqlens is not None:
            x = x + self.att(self.ln1(x), cu_seqlens=cu_seqlens, max_seqlen=max_seqlen)
            return x + self.ffn(self.ln2(x), cu_seqlens=cu_seqlens)
        x = x + self.att(self.ln1(x))
        return x + self.ffn(self.ln2(x))


def _backbone(model, idx, cu_seqlens, max_seqlen):
    """(ln_out(blocks(emb(idx))), the packed keywords) of a model with emb, blocks, ln_out and grad_cp; a packed batch is [1,total_T]."""
    x = model.emb(idx)
    packed = {} if cu_seqlens is None else {"cu_seqlens": cu_seqlens, "max_seqlen": max_seqlen}
    if packed:
        assert idx.size(0) == 1, "a packed batch is [1,total_T]"
    for block in model.blocks:
        if model.grad_cp and model.training and torch.is_grad_enabled():   # args.grad_cp, src/model_ext.py:1756-1758
            from torch.utils.checkpoint import checkpoint
            x = checkpoint(block, x, use_reentrant=False, **packed)
        else:
            x = block(x, **packed)
    return model.ln_out(x), packed


class SequenceEmbedder(nn.Module):
    """RwkvForSequenceEmbedding.forward (src/model_ext.py:1739-1769): emb -> blocks -> ln_out -> pooling at the
    first `emb_id` token -> optional tanh(dense(.))."""

    def __init__(self, vocab_size, n_embd, n_layer, dim_att=None, dim_ffn=None, emb_id=1, pad_id=0,
                 pooling_type="weightedmean", add_mlp=False, output_dim=0, grad_cp=False, wkv=None, wkv_varlen=None):
        super().__init__()
        self.emb_id, self.pad_id, self.pooling_type, self.grad_cp = emb_id, pad_id, pooling_type, grad_cp
        self.emb = nn.Embedding(vocab_size, n_embd)
        self.blocks = nn.ModuleList([Block(n_embd, dim_att or n_embd, dim_ffn or int(n_embd * 3.5) // 32 * 32, i, wkv=wkv,
                                           wkv_varlen=wkv_varlen) for i in range(n_layer)])
        self.ln_out = nn.LayerNorm(n_embd)
        self.dense = nn.Linear(n_embd, output_dim or n_embd) if add_mlp else None

    def forward(self, idx, cu_seqlens=None, max_seqlen=None, actual_len=None):
        """cu_seqlens (int32 [n_seq + 1] on the device of idx): idx is a packed batch [1,total_T] as pack_rows makes it -- the rows back to
        back, each cut behind its first emb_id token -- with max_seqlen the longest row and actual_len (int32 [n_seq]) the emb_id token's
        position in every row (None: the row's last token); one vector per sequence comes back, as from the padded rows.  Nothing of the
        packed route reads the device."""
        x, packed = _backbone(self, idx, cu_seqlens, max_seqlen)
        if packed:
            x = callers.pooling_packed(x, cu_seqlens, actual_len, self.pooling_type)
        else:
            actual_len = torch.eq(idx, self.emb_id).int().argmax(-1)
            x = callers.pooling(x, actual_len, self.pooling_type)
        if self.dense is not None:
            x = torch.tanh(self.dense(x.to(self.dense.weight.dtype)))   # pooling returns bf16 (src/model_ext.py:1721)
        return x


def training_loss(model: nn.Module, query, positive=None, negative=None):
    """RwkvForSequenceEmbedding.training_step with is_in_batch_negative (src/model_ext.py:1882-1911).  `query` may be a packed batch (a
    dict of batches(packed=True): the query, positive and negative rows of the step in one packed idx); positive and negative are then
    not used."""
    if isinstance(query, dict):
        p = query
        emb = model(p["idx"], cu_seqlens=p["cu_seqlens"], max_seqlen=p["max_seqlen"], actual_len=p["actual_len"]).float()
        bs = p["bs"]
        return callers.info_nce_loss(emb[:bs], emb[bs:2 * bs], emb[2 * bs:] if emb.size(0) > 2 * bs else None)
    parts = [query, positive] + ([negative] if negative is not None else [])
    emb = model(torch.cat(parts, dim=0)).float()
    bs = query.size(0)
    return callers.info_nce_loss(emb[:bs], emb[bs:2 * bs], emb[2 * bs:] if negative is not None else None)


class CausalLM(nn.Module):
    """The language model of src/model.py:1147-1154 (RWKV.forward without dropout / head_qk): emb -> blocks -> ln_out, and a bias-free
    head that forward does NOT apply: it returns the hidden state behind ln_out, and lm_training_loss hands it to callers.head_loss
    together with head.weight, so that the [rows, V] logits never exist (model.head(x) applies the head where somebody wants them)."""

    def __init__(self, vocab_size, n_embd, n_layer, dim_att=None, dim_ffn=None, grad_cp=False, wkv=None, wkv_varlen=None):
        super().__init__()
        self.grad_cp = grad_cp
        self.emb = nn.Embedding(vocab_size, n_embd)
        self.blocks = nn.ModuleList([Block(n_embd, dim_att or n_embd, dim_ffn or int(n_embd * 3.5) // 32 * 32, i, wkv=wkv,
                                           wkv_varlen=wkv_varlen) for i in range(n_layer)])
        self.ln_out = nn.LayerNorm(n_embd)
        self.head = nn.Linear(n_embd, vocab_size, bias=False)

    def forward(self, idx, cu_seqlens=None, max_seqlen=None):
        """cu_seqlens (int32 [n_seq + 1] on the device of idx) / max_seqlen: idx is a packed batch [1,total_T] as pack_lm_rows makes it."""
        return _backbone(self, idx, cu_seqlens, max_seqlen)[0]


def pack_lm_rows(idx, targets, lengths, total_multiple: int = 1, pad_id: int = 0):
    """The padded rows idx, targets [B, T] (host tensors) with lengths [B] as one packed batch: (idx [1, total_T], targets [1, total_T],
    cu_seqlens int32 [B + 1], max_seqlen int).  Row b keeps its first lengths[b] tokens.  total_multiple > 1 rounds total_T up with rows
    behind the last sequence that belong to none: pad_id tokens with target -100, which the packed operators never read and the loss
    ignores (lm_training_loss gives them no L2 term either)."""
    assert idx.dim() == 2 and idx.shape == targets.shape and total_multiple >= 1
    lens = torch.as_tensor(lengths, dtype=torch.long).clamp(0, idx.size(1))
    keep = torch.arange(idx.size(1)).unsqueeze(0) < lens.unsqueeze(1)
    cu = F.pad(lens.cumsum(0), (1, 0)).to(torch.int32)
    flat_idx, flat_tgt = idx[keep], targets[keep]
    total = max(-(-flat_idx.numel() // total_multiple) * total_multiple, 1)
    flat_idx = F.pad(flat_idx, (0, total - flat_idx.numel()), value=pad_id)
    flat_tgt = F.pad(flat_tgt, (0, total - flat_tgt.numel()), value=-100)
    return flat_idx.unsqueeze(0), flat_tgt.unsqueeze(0), cu, int(lens.max())


def lm_training_loss(model: nn.Module, idx, targets, mask=None, cu_seqlens=None, max_seqlen=None, chunk_rows: int = 4096,
                     l2wrap: float = 1e-4, kernels=None):
    """The reference's training_step loss (src/model.py:1244-1283) of a CausalLM through callers.head_loss.  idx, targets [B,T]: the L2
    term covers all B * T rows, pad rows included, as the reference's does.  With cu_seqlens (idx, targets [1,total_T] of pack_lm_rows) the
    L2 row count is cu_seqlens[-1], taken on the device, and rows outside every sequence get no L2 term: with target -100 they are then
    never read."""
    x = model(idx, cu_seqlens=cu_seqlens, max_seqlen=max_seqlen)
    if cu_seqlens is None:
        return callers.head_loss(x, model.head.weight, targets, mask, l2wrap, None, chunk_rows, kernels)
    pos = torch.arange(x.shape[-2], device=x.device)
    inside = (pos >= cu_seqlens[0]) & (pos < cu_seqlens[-1])
    return callers.head_loss(x, model.head.weight, targets, mask, l2wrap, cu_seqlens[-1], chunk_rows, kernels, l2_rows=inside)


def trainable_parameters(model: nn.Module) -> List[nn.Parameter]:
    return [p for p in model.parameters() if p.requires_grad]


def grad_allreduce_bytes(model: nn.Module) -> int:
    """Bytes one gradient all-reduce moves per rank and step (the message of SURVEY.md 8e)."""
    return sum(p.numel() * p.element_size() for p in trainable_parameters(model))


def wrap_ddp(model: nn.Module, device=None, bucket_cap_mb: int = 32):
    """DDP over the default process group (nccl = RCCL on ROCm, gloo in the CPU tests).  One ring all-reduce per
    bucket; the whole LoRA gradient set of the 1B6 model (13-28 MB) fits one 32 MB bucket, so the collective is
    per-link bound on xGMI only once per step and overlaps the tail of the backward."""
    from torch.nn.parallel import DistributedDataParallel as DDP
    ids = None if device is None or device.type == "cpu" else [device.index]
    return DDP(model, device_ids=ids, bucket_cap_mb=bucket_cap_mb, gradient_as_bucket_view=True,
               find_unused_parameters=False, broadcast_buffers=False)


# ---- synthetic data of the reference's shape: length-bucketed (query, positive, negative) triples --------------------
def synth_example(index: int, seq_len: int, vocab_size: int, emb_id: int = 1, pad_id: int = 0, min_len: int = 16):
    """Deterministic pseudo-random triple for dataset position `index`: tokens, then `emb_id`, then padding
    (the layout create_mask / pooling expect, src/model_ext.py:1763-1764)."""
    g = torch.Generator().manual_seed(1000003 * index + 17)
    out = []
    for _ in range(3):
        n = int(torch.randint(min_len, seq_len - 1, (1,), generator=g))
        row = torch.full((seq_len,), pad_id, dtype=torch.long)
        row[:n] = torch.randint(2, vocab_size, (n,), generator=g)
        row[n] = emb_id
        out.append(row)
    return out


def pack_rows(idx, emb_id: int = 1, total_multiple: int = 1, pad_id: int = 0):
    """The padded rows idx [B, T] (a host tensor, where the loader's batches live) as one packed batch: (idx [1, total_T], cu_seqlens int32
    [B + 1], max_seqlen int, actual_len int32 [B]).  Row b keeps its tokens 0 .. a_b inclusive, a_b = the position of its first emb_id
    (argmax semantics: a row without emb_id keeps one token, a_b = 0, and pools to what the dense path gives it); actual_len = a.
    total_multiple > 1 rounds total_T up to a multiple of it with pad_id rows behind the last sequence that belong to none
    (cu_seqlens[-1] < total_T): the packed operators never read such rows and write their outputs and gradients as +0
    (include/wkv6_amd.h, "rows outside every sequence"), and a run sees at most T B / total_multiple distinct GEMM shapes."""
    assert idx.dim() == 2 and total_multiple >= 1
    a = torch.eq(idx, emb_id).int().argmax(-1)
    keep = torch.arange(idx.size(1)).unsqueeze(0) <= a.unsqueeze(1)
    lens = a + 1
    cu = F.pad(lens.cumsum(0), (1, 0)).to(torch.int32)
    flat = idx[keep]
    total = -(-flat.numel() // total_multiple) * total_multiple
    flat = F.pad(flat, (0, total - flat.numel()), value=pad_id)
    return flat.unsqueeze(0), cu, int(lens.max()), a.to(torch.int32)


def batches(sampler: BucketBatchSampler, seq_len: int, vocab_size: int, packed: bool = False, total_multiple: int = 1) -> Iterable[dict]:
    """packed: one packed batch per step instead of three padded ones -- the query, then the positive, then the negative rows through
    pack_rows, with "bs" (rows per part) recorded; training_loss and train_steps take it as it is."""
    for idxs in sampler:
        rows = [synth_example(i, seq_len, vocab_size) for i in idxs]
        if packed:
            idx, cu, max_seqlen, actual_len = pack_rows(torch.stack([r[j] for j in range(3) for r in rows]), total_multiple=total_multiple)
            yield {"idx": idx, "cu_seqlens": cu, "max_seqlen": max_seqlen, "actual_len": actual_len, "bs": len(rows)}
            continue
        yield {"query": torch.stack([r[0] for r in rows]), "positive": torch.stack([r[1] for r in rows]),
               "negative": torch.stack([r[2] for r in rows])}


def to_device(batch: dict, device) -> dict:
    """The tensors of a batch of batches() on `device`; the ints of a packed batch (max_seqlen, bs) stay host ints."""
    return {k: v.to(device, non_blocking=True) if isinstance(v, torch.Tensor) else v for k, v in batch.items()}


def train_steps(model, opt, batch_iter, device, steps: int):
    """`steps` optimizer steps; returns the losses.  `model` is the DDP-wrapped SequenceEmbedder."""
    losses = []
    for _, batch in zip(range(steps), batch_iter):
        batch = to_device(batch, device)
        opt.zero_grad(set_to_none=True)
        loss = training_loss(model, batch) if "idx" in batch else training_loss(model, batch["query"], batch["positive"], batch.get("negative"))
        loss.backward()              # DDP all-reduces the LoRA gradients here
        opt.step()
        losses.append(loss.detach())
    return losses
