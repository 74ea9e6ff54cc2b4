"""Several LoRA adapters over one RWKV-6 base model, chosen per sequence of a packed batch.

What the reference runs (src/layers.py: LoraLinear.add_adapter / set_adapter(model, name); src/model_run.py: set_adapter, enable_lora
and the fused bi- / cross-encoder class): one base model under several adapters -- chat SFT, bi-encoder, cross-encoder -- with ONE active
adapter per call, switched by name before every pass ("not thread-safe since we need to switch the adapter name before encoding").  A
batch that mixes requests of three kinds is three passes there.

Here every sequence of a packed batch names its own adapter (or none) in a device tensor and the whole batch is one pass:
`MultiLoraLinear` holds a frozen base weight and POOLS of adapters, lora_A [n_adapters,R,in] and lora_B [n_adapters,out,R] (the layout of
the reference's lora_A / lora_B weights), `set_adapters(model, cu_seqlens, adapter)` is the reference's set_adapter with a tensor per
sequence in place of a name, and the low-rank term is the segmented matmul of csrc/wkv6_lora.hip (mix_op.lora_packed) behind the base
GEMM.  infctx.step_packed and the sub-layer functions reach the linears through the modules and need nothing else.

Out of scope: the reference's LoraEmbedding (an adapter on the embedding table), adapter training (train_dp.LoraLinear is the training
module; the eager path here has autograd, the HIP path is forward only), and torch_shim.
"""
from typing import Iterable, List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

# the reference's six targets (its chat / bi-encoder / cross-encoder adapters all name these)
DEFAULT_TARGETS = ("att.key", "att.value", "att.receptance", "ffn.key", "ffn.value", "ffn.receptance")


def row_adapters(cu_seqlens, adapter, total_T: int, n_adapters: int):
    """int64 [total_T]: the adapter that serves each packed row, -1 for none -- the rule of wkv6_lora_packed_bf16 (include/wkv6_amd.h): a
    row's sequence is the last s with cu_seqlens[s] <= row, the row is served when it lies inside that sequence's bounds clamped into
    [0,total_T] and adapter[s] lies in [0,n_adapters).  Nothing is read on the host."""
    n_seq = adapter.numel()
    cu = cu_seqlens.long()
    rows = torch.arange(total_T, device=cu.device)
    s = torch.searchsorted(cu[:n_seq].contiguous(), rows, right=True) - 1
    sc = s.clamp(min=0)
    ad = adapter.long()[sc]
    ok = (s >= 0) & (rows >= cu[sc].clamp(0, total_T)) & (rows < cu[sc + 1].clamp(0, total_T)) & (ad >= 0) & (ad < n_adapters)
    return torch.where(ok, ad, torch.full_like(ad, -1))


def lora_packed_eager(x, y, A_pool, B_pool, scale, adapter, cu_seqlens):
    """What mix_op.lora_packed computes, in eager PyTorch on any device and dtype, with autograd, out of place: x [total_T,K], y [total_T,N]
    -> the new y.  One masked pass per adapter, y = where(row_adapter == a, y + scale[a] * ((x @ A[a].T) @ B[a].T), y); nothing is read on
    the host.  xa = x @ A[a].T is rounded to the activation dtype (the reference under autocast, train_dp._LoraLinearFn); the rest of the
    term is formed in fp32 and the sum rounded once, as the kernels do."""
    which = row_adapters(cu_seqlens, adapter, x.shape[0], A_pool.shape[0]).unsqueeze(1)
    for a in range(A_pool.shape[0]):
        xa = F.linear(x, A_pool[a])
        term = F.linear(xa.float(), B_pool[a].float()) * scale[a]
        y = torch.where(which == a, (y.float() + term).to(y.dtype), y)
    return y


class MultiLoraLinear(nn.Module):
    """y = x W^T, then for every row of a sequence on adapter a:  y += scaling[a] * (x A[a]^T) B[a]^T  -- W frozen, no bias.

    `weight` [out,in]; the pools `lora_A` [n_adapters,R,in] and `lora_B` [n_adapters,out,R] start at zero (an empty adapter adds nothing);
    `scaling` is an fp32 buffer [n_adapters] = alpha / r of each adapter's own rank, and stays fp32 under .to(dtype).
    The batch is bound with set_adapters; unbound, the layer is the base linear.
    `kernels` (None: where they apply; False: never, the eager code, which also serves the CPU, fp16 / fp32 and autograd; True: they must,
    or forward raises) has the meaning of infctx's pool_kernels."""

    def __init__(self, in_features: int, out_features: int, n_adapters: int, r: int):
        super().__init__()
        assert n_adapters >= 1 and r >= 1
        self.in_features, self.out_features, self.n_adapters, self.r = in_features, out_features, n_adapters, r
        self.weight = nn.Parameter(torch.empty(out_features, in_features), requires_grad=False)
        self.lora_A = nn.Parameter(torch.zeros(n_adapters, r, in_features), requires_grad=False)
        self.lora_B = nn.Parameter(torch.zeros(n_adapters, out_features, r), requires_grad=False)
        self.register_buffer("scaling", torch.zeros(n_adapters, dtype=torch.float32))
        self.kernels = None
        self._cu = self._adapter = None
        nn.init.kaiming_uniform_(self.weight, a=5 ** 0.5)

    @classmethod
    def from_linear(cls, lin: nn.Linear, n_adapters: int, r: int) -> "MultiLoraLinear":
        assert lin.bias is None, "Biased MultiLoraLinear not supported"
        m = cls(lin.in_features, lin.out_features, n_adapters, r).to(lin.weight.device, lin.weight.dtype)
        with torch.no_grad():
            m.weight.copy_(lin.weight)
        return m

    def _apply(self, fn, *args, **kwargs):
        kept = self.scaling
        super()._apply(fn, *args, **kwargs)
        if self.scaling.dtype != torch.float32:          # .to(bf16) / .half(): alpha / r keeps its fp32 value, on the new device
            self.scaling = kept.to(self.scaling.device)
        return self

    def set_weights(self, index: int, lora_A, lora_B, alpha: float):
        """Adapter `index` = (lora_A [r,in], lora_B [out,r]) with scaling alpha / r; r <= R, a lower rank is zero-padded into the pool."""
        r = lora_A.shape[0]
        if not (0 <= index < self.n_adapters):
            raise IndexError(f"adapter index {index} outside the pool of {self.n_adapters}")
        if not (lora_A.dim() == 2 and lora_B.dim() == 2 and 1 <= r <= self.r and tuple(lora_A.shape) == (r, self.in_features)
                and tuple(lora_B.shape) == (self.out_features, r)):
            raise ValueError(f"adapter weights must be lora_A [r,{self.in_features}] and lora_B [{self.out_features},r] with r <= {self.r}, "
                             f"got {list(lora_A.shape)} and {list(lora_B.shape)}")
        with torch.no_grad():
            self.lora_A[index].zero_()
            self.lora_B[index].zero_()
            self.lora_A[index, :r].copy_(lora_A)
            self.lora_B[index, :, :r].copy_(lora_B)
            self.scaling[index] = float(alpha) / r

    def bind(self, cu_seqlens, adapter):
        """The batch the next forwards serve: cu_seqlens int [n_seq + 1] and adapter int [n_seq], kept by reference (refilling them in
        place re-routes a captured graph); None, None unbinds."""
        assert (cu_seqlens is None) == (adapter is None), "bind both cu_seqlens and adapter, or neither"
        if cu_seqlens is not None:
            assert cu_seqlens.dim() == 1 and adapter.dim() == 1 and cu_seqlens.numel() == adapter.numel() + 1, \
                "cu_seqlens is [n_seq + 1], adapter [n_seq]"
        self._cu, self._adapter = cu_seqlens, adapter

    def _use_kernels(self, x) -> bool:
        if self.kernels is False:
            return False
        from . import mix_op
        bf = torch.bfloat16
        ints_ok = all(t.dtype == torch.int32 and t.is_contiguous() and t.device == x.device for t in (self._cu, self._adapter))
        if self.kernels is None and not ints_ok:
            return False                                  # the eager code casts whatever it gets; under True mix_op refuses it
        why = None
        if not (x.is_cuda and x.dtype == self.weight.dtype == self.lora_A.dtype == self.lora_B.dtype == bf):
            why = "x, weight and the pools must be bf16 on the GPU"
        elif not (self.lora_A.is_contiguous() and self.lora_B.is_contiguous() and self.lora_A.device == self.lora_B.device == x.device):
            why = "the pools must be contiguous on the device of x"
        elif (self.r not in mix_op.LORA_RANKS or self.in_features % 64 or self.out_features % 64
              or not (64 <= self.in_features <= 16384 and 64 <= self.out_features <= 16384)):
            why = f"the pool rank must be one of {mix_op.LORA_RANKS} and in / out features multiples of 64 in [64, 16384]"
        elif x.numel() < self.in_features:
            why = "the batch has no row"
        elif torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            why = "a gradient is required (the kernels are forward only: call under torch.no_grad())"
        if why is not None and self.kernels:
            raise RuntimeError("kernels=True: " + why)
        return why is None

    def forward(self, x):
        y = F.linear(x, self.weight)
        if self._cu is None:
            return y
        rows = x.numel() // self.in_features
        if self._use_kernels(x):
            from . import mix_op
            x2 = x.reshape(rows, self.in_features)
            mix_op.lora_packed(x2 if x2.is_contiguous() else x2.contiguous(), y.view(rows, self.out_features), self.lora_A, self.lora_B,
                               self.scaling, self._adapter, self._cu)
            return y
        return lora_packed_eager(x.reshape(rows, self.in_features), y.reshape(rows, self.out_features), self.lora_A, self.lora_B,
                                 self.scaling, self._adapter, self._cu).view(y.shape)


def _modules(model) -> nn.Module:
    """`model` or, for a plain sequence of blocks (what infctx.step_packed takes), a ModuleList over them: names are then '0.att.key', ..."""
    return model if isinstance(model, nn.Module) else nn.ModuleList(list(model))


def inject_adapters(model, n_adapters: int, r: int = 8, targets: Sequence[str] = DEFAULT_TARGETS) -> List[str]:
    """Freeze `model` (a module or a sequence of blocks) and replace every nn.Linear whose qualified name ends with one of `targets` by a
    MultiLoraLinear with empty pools of n_adapters adapters of rank r (train_dp.inject_lora's pattern; the reference injects on load,
    src/layers.py: inject_lora_adapter_with_state_dict).  Returns the names of the replaced modules."""
    root = _modules(model)
    for p in root.parameters():
        p.requires_grad_(False)
    replaced = []
    for name, mod in list(root.named_modules()):
        for child_name, child in list(mod.named_children()):
            full = f"{name}.{child_name}" if name else child_name
            if isinstance(child, nn.Linear) and any(full.endswith(t) for t in targets):
                setattr(mod, child_name, MultiLoraLinear.from_linear(child, n_adapters, r))
                replaced.append(full)
    return replaced


def adapter_layers(model) -> Iterable:
    """(name, module) of every MultiLoraLinear of `model`."""
    return [(n, m) for n, m in _modules(model).named_modules() if isinstance(m, MultiLoraLinear)]


def set_adapters(model, cu_seqlens, adapter) -> None:
    """Bind the batch on every MultiLoraLinear of `model`: sequence s (rows cu_seqlens[s] .. cu_seqlens[s+1] of the packed batch) runs under
    adapter[s]; a value outside the pool, -1 by convention, means the base model only.  The reference's set_adapter(model, name) with a
    device tensor per sequence in place of a name.  Both tensors are bound by reference.  (None, None) unbinds: base linears."""
    for _, m in adapter_layers(model):
        m.bind(cu_seqlens, adapter)


def load_adapter(model, index: int, state_dict, alpha: float, peft_name: Optional[str] = None,
                 parent_model_name: Optional[str] = None) -> List[str]:
    """Fill adapter `index` of every MultiLoraLinear of `model` from `state_dict`, under the key names the reference's loader reads
    (src/layers.py: inject_lora_adapter_with_state_dict): '{key}.lora_A' / '{key}.lora_B' with peft_name None, otherwise
    '[{parent_model_name}.]{key}.lora_A.{peft_name}.weight' and the same for lora_B, {key} being the module's qualified name.  A layer
    without both keys keeps what it has.  Returns the names of the layers that were filled."""
    filled = []
    for key, m in adapter_layers(model):
        if peft_name is None:
            ka, kb = f"{key}.lora_A", f"{key}.lora_B"
        else:
            head = f"{parent_model_name}.{key}" if parent_model_name is not None else key
            ka, kb = f"{head}.lora_A.{peft_name}.weight", f"{head}.lora_B.{peft_name}.weight"
        if ka in state_dict and kb in state_dict:
            m.set_weights(index, state_dict[ka], state_dict[kb], alpha)
            filled.append(key)
    return filled
