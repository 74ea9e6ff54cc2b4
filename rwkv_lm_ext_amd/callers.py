"""Host-side callers of the WKV6 operator: what sits immediately on either side of the hot path in the reference.

Parameter names equal the reference's state_dict keys, so a reference checkpoint loads with ``load_state_dict``.

  reverse helpers      src/model_ext.py:398-419 (create_mask, reverse_x_idx, reverse_x)            SURVEY a12
  RWKV_Tmix_x052       src/model.py:292-374 (RWKV-5 time-mix: static lerps, static decay, WKV5 operator)
  Tmix_x060            src/model.py:376-477 == src/model_encoder_run.py:96-186 (time-mix)          SURVEY a13
  CMix_x060            src/model.py:616-644 == src/model_encoder_run.py:189-219 (channel-mix)      SURVEY a14
  Tmix_x060.forward_bi_c   composition C: (WKV(x) + unrev(WKV(rev x))) / 2, src/model_ext.py:421-437    SURVEY a15
  Tmix_x060.forward_bi_b   composition B: WKV(r,k,v,w,u) + unrev(WKV(r, rev k, rev v, w, u)), src/model_bi.py:325-350  SURVEY a16
  BiBlock / RwkvEncoder    src/model_encoder_run.py:222-348 (encoder with sentence embedding at the first emb_id)  SURVEY a15
  pooling / info_nce_loss  src/model_ext.py:1708-1738, 1882-1911                                       SURVEY a17
  pooling_packed           the same pooling on a packed batch (HIP kernels of mix_op.pool_packed, or an eager restatement)
  lm_loss / head_loss      src/model.py:937-974, 1244-1283 (F.cross_entropy + L2Wrap behind the LM head; HIP kernels of mix_op.ce_rows,
                           or an eager restatement); head_loss walks the head in row chunks and never holds [rows, V]

The WKV call itself is `wkv(B, T, C, H, r, k, v, w, u) -> y` (default: rwkv_lm_ext_amd.wkv.RUN_CUDA_RWKV6, the HIP
kernels; bf16 on the GPU); on a packed variable-length batch (forward(x, cu_seqlens=...)) it is the second hook
`wkv_varlen(total_T, C, H, r, k, v, w, u, cu_seqlens, max_seqlen) -> y`.  Everything else is plain PyTorch (the GEMMs ride rocBLAS), as in the reference.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F


# ---- a12: padding mask and in-row reversal ---------------------------------------------------------------------
def create_mask(x, emb_id=1, pad_id=0):
    """1 for ordinary tokens, 0 for pad and for the embedding marker (src/model_encoder_run.py:7-11)."""
    return ((x != pad_id) & (x != emb_id)).to(torch.int)


def reverse_x_idx(mask, max_len):
    """Per row: indices that reverse the first sum(mask) positions and keep the rest (src/model_ext.py:410-417).
    Vectorised (the reference loops over the batch in python)."""
    n = mask.sum(dim=1, keepdim=True).to(torch.long)                      # [B,1]
    pos = torch.arange(max_len, device=mask.device).unsqueeze(0)         # [1,T]
    return torch.where(pos < n, n - 1 - pos, pos)


def reverse_x(x, rev_idx):
    return torch.gather(x, 1, rev_idx.to(x.device).unsqueeze(-1).expand(-1, -1, x.size(-1)))


def packed_reverse_idx(cu_seqlens, rev_n, total_T):
    """reverse_x_idx on a packed batch: a [total_T] gather index that reverses the first rev_n[s] tokens of sequence s (rows
    cu_seqlens[s] .. cu_seqlens[s+1]-1; rev_n clamped to the sequence's length) and keeps every other row -- the rows of no sequence
    included -- in place.  Computed on the device of its arguments, no host read.  The index is its own inverse."""
    cu = cu_seqlens.long()
    n_seq = cu.numel() - 1
    pos = torch.arange(total_T, device=cu.device)
    seq = torch.searchsorted(cu[1:].contiguous(), pos, right=True).clamp(max=n_seq - 1)      # the last s with cu[s] <= row
    start = cu[seq]
    n = torch.minimum(rev_n.long().clamp_min(0)[seq], (cu[seq + 1] - start).clamp_min(0))
    t = pos - start
    return torch.where((t >= 0) & (t < n), start + n - 1 - t, pos)


def _default_wkv(B, T, C, H, r, k, v, w, u):
    from .wkv import RUN_CUDA_RWKV6
    bf = torch.bfloat16
    y = RUN_CUDA_RWKV6(B, T, C, H, *(t.to(bf).contiguous() for t in (r, k, v, w, u)))
    return y.to(r.dtype)


def _default_wkv_varlen(total_T, C, H, r, k, v, w, u, cu_seqlens, max_seqlen):
    from .wkv import RUN_CUDA_RWKV6_VARLEN
    bf = torch.bfloat16
    y = RUN_CUDA_RWKV6_VARLEN(total_T, C, H, *(t.to(bf).contiguous() for t in (r, k, v, w, u)), cu_seqlens, max_seqlen)
    return y.to(r.dtype)


def _packed_prev(x, cu_seqlens, shifted0=None):
    """x delayed by one token on a packed batch [1,total_T,C]: zero in front of every sequence's first token, or shifted0[s] ([n_seq,C],
    the token a serving loop carried over) in front of non-empty sequence s (eager path; the index arithmetic stays on the device of x)."""
    T = x.shape[1]
    opens = torch.zeros(T + 1, dtype=torch.bool, device=x.device)
    opens[cu_seqlens[:-1].long().clamp(0, T)] = True
    prev = F.pad(x, (0, 0, 1, -1)).masked_fill(opens[:T].view(1, T, 1), 0)
    if shifted0 is None:
        return prev
    cu = cu_seqlens.long().clamp(0, T)
    first = torch.where(cu[1:] > cu[:-1], cu[:-1], torch.full_like(cu[:-1], T))    # an empty sequence has no first token: row T is a dummy
    return F.pad(prev, (0, 0, 0, 1)).index_copy(1, first, shifted0.to(x.dtype).unsqueeze(0))[:, :T]


class Tmix_x060(nn.Module):
    """RWKV-6 time-mix around the WKV operator (src/model.py:376-477)."""

    def __init__(self, n_embd, dim_att, head_size=64, head_size_divisor=8, wkv=None, fused=None, wkv_varlen=None):
        """fused: None = the HIP elementwise kernels of mix_op whenever the input is a bf16 GPU tensor; True / False force.
        wkv_varlen: the operator call of forward(x, cu_seqlens=...) on a packed batch,
        `wkv_varlen(total_T, C, H, r, k, v, w, u, cu_seqlens, max_seqlen) -> y` with [1,total_T,C] tensors (default:
        wkv.RUN_CUDA_RWKV6_VARLEN)."""
        super().__init__()
        self.n_head = dim_att // head_size
        self.wkv = wkv or _default_wkv
        self.wkv_varlen = wkv_varlen or _default_wkv_varlen
        self.fused = fused
        # forward(): GroupNorm * gate inside the operator's forward kernel (wkv.WKV_6_GN) instead of a second kernel.  Off by
        # default: it saves the y round trip through HBM but the layer is not faster for it -- B x T = 48 x 512, C = 2048 on
        # MI355X: fwd+bwd 6.644 vs 6.626 ms, forward only 1.612 vs 1.593 ms (profiles/r03_tmix_layer_epilogue.txt): the 56 us
        # GroupNorm kernel runs at 5.4 TB/s, and the statistics exchange lengthens the forward's consumer waves by as much.
        self.fuse_epilogue = False
        # forward_bi_b / forward_bi_c with in-kernel reversal: both operator calls of the layer in one launch per pass
        # (wkv.WKV_6_PAIR) instead of two
        self.pair_launch = True
        # jit_func, inference only: the two low-rank pairs (ddlerp -> W1 -> tanh -> W2 -> ddlerp, and the decay) in two launches each
        # (mix_op.tmix_inputs, mix_op.decay_lowrank) instead of eleven.  Off by default: the contractions sum in the kernels' own order, so
        # the outputs differ from the torch matmuls' in their last bits (profiles/lowrank_parity.txt)
        self.fuse_lowrank = False
        self._lowrank_cache = None
        d_mix = 64 if n_embd == 4096 else 32                              # TIME_MIX_EXTRA_DIM
        d_decay = 128 if n_embd == 4096 else 64                           # TIME_DECAY_EXTRA_DIM
        z = lambda *s: nn.Parameter(torch.zeros(*s))
        for n in ("x", "w", "k", "v", "r", "g"):
            setattr(self, "time_maa_" + n, z(1, 1, n_embd))
        self.time_maa_w1 = z(n_embd, d_mix * 5)
        self.time_maa_w2 = z(5, d_mix, n_embd)
        self.time_decay = z(1, 1, dim_att)
        self.time_decay_w1 = z(n_embd, d_decay)
        self.time_decay_w2 = z(d_decay, dim_att)
        self.time_faaaa = z(self.n_head, head_size)
        self.receptance = nn.Linear(n_embd, dim_att, bias=False)
        self.key = nn.Linear(n_embd, dim_att, bias=False)
        self.value = nn.Linear(n_embd, dim_att, bias=False)
        self.output = nn.Linear(dim_att, n_embd, bias=False)
        self.gate = nn.Linear(n_embd, dim_att, bias=False)
        self.ln_x = nn.GroupNorm(self.n_head, dim_att, eps=1e-5 * head_size_divisor ** 2)

    def _maa5(self):
        """[5,C]: the static lerp weights of the decay, key, value, receptance and gate inputs, in the order the
        low-rank correction tensor is laid out (src/model.py:441-442: mw, mk, mv, mr, mg)."""
        return torch.cat([self.time_maa_w, self.time_maa_k, self.time_maa_v, self.time_maa_r, self.time_maa_g], 0).view(5, -1)

    def _use_fused(self, x):
        """The fused HIP kernels serve bf16 GPU activations with bf16 GPU parameters and rows of at most 4096 channels in
        multiples of 64 (csrc/wkv6_mix.hip: check_rows); anything else (fp32 parameters under autocast, a partly cast model,
        wider rows) takes the eager path unless `fused` forces a choice."""
        if self.fused is None:
            C = x.shape[-1]
            ok = lambda t: t.is_cuda and t.dtype == torch.bfloat16
            return (ok(x) and ok(self.time_maa_x) and ok(self.time_maa_w) and ok(self.ln_x.weight)
                    and C % 64 == 0 and C <= 4096)
        return self.fused

    _LOWRANK_PARAMS = ("time_maa_x", "time_maa_w", "time_maa_k", "time_maa_v", "time_maa_r", "time_maa_g", "time_maa_w1", "time_maa_w2",
                       "time_decay", "time_decay_w1", "time_decay_w2")

    def _lowrank_weights(self):
        """(maa_x [C], W1t [5 D, C], W2t [5, C, D], maa5 [5, C], D1t [Dd, C], D2t [N, Dd], time_decay [N]): the parameters of the two low-rank
        pairs as mix_op.tmix_inputs and mix_op.decay_lowrank take them, the matrices in nn.Linear layout [out, in].  The copies are kept on
        the module and rebuilt when a parameter's data_ptr() or _version changes (an optimizer step, load_state_dict, .to()).  A write
        through `p.data` (p.data.copy_(...), p.data.mul_(...)) changes neither, and the copies go stale without notice: call
        drop_lowrank_weights() behind such a write."""
        params = [getattr(self, n) for n in self._LOWRANK_PARAMS]
        key = tuple((p.data_ptr(), p._version, p.dtype, p.device) for p in params)
        if self._lowrank_cache is None or self._lowrank_cache[0] != key:
            with torch.no_grad():
                C = self.time_maa_x.shape[-1]
                held = (self.time_maa_x.detach().reshape(C).contiguous(), self.time_maa_w1.detach().t().contiguous(),
                        self.time_maa_w2.detach().transpose(1, 2).contiguous(), self._maa5().detach().contiguous(),
                        self.time_decay_w1.detach().t().contiguous(), self.time_decay_w2.detach().t().contiguous(),
                        self.time_decay.detach().reshape(-1).contiguous())
            self._lowrank_cache = (key, held)
        return self._lowrank_cache[1]

    def drop_lowrank_weights(self):
        """Forget the copies of _lowrank_weights: the next call makes them again (not inside a graph capture)."""
        self._lowrank_cache = None

    def _use_lowrank(self, x, rev_n):
        """fuse_lowrank applies: the fused path, nothing asks for a gradient, no reversal map, widths the kernels have."""
        if not (self.fuse_lowrank and rev_n is None and self._use_fused(x)):
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(getattr(self, n).requires_grad for n in self._LOWRANK_PARAMS)):
            return False
        from .mix_op import LOWRANK_D, LOWRANK_DD
        bf, N = torch.bfloat16, self.time_decay.shape[-1]
        return (x.dtype == bf and all(getattr(self, n).dtype == bf and getattr(self, n).device == x.device for n in self._LOWRANK_PARAMS)
                and self.time_maa_w2.shape[1] in LOWRANK_D and self.time_decay_w1.shape[1] in LOWRANK_DD
                and x.shape[-1] % 64 == 0 and x.shape[-1] <= 4096 and N % 64 == 0 and N <= 4096)

    def jit_func(self, x, shifted=None, rev_n=None, cu_seqlens=None, shifted0=None, shift_pool=None, slots=None):
        """Inputs of the WKV operator from the block input (src/model.py:435-459): every projection reads its own
        data-dependent blend of x_t and x_{t-1},  x + (x_{t-1} - x) * (maa_s + m_s),  where the five corrections m_s come
        from one shared low-rank pair (tanh(blend_x @ W1) -> per-stream W2).  Then r, k, v = Linear(blend), g = silu(Linear),
        w = time_decay + tanh(blend_w @ D1) @ D2.
        `shifted`: x delayed by one token; default zero-padded (nn.ZeroPad2d((0,0,1,-1))), the infctx path passes the
        previous chunk's last token in front (src/model.py:740-741).
        On bf16 GPU tensors the two blend stages are one HIP kernel each (mix_op.ddlerp).
        `rev_n` (fused path only, int32 [B]): the token shift runs over the stream whose first rev_n[b] tokens are reversed
        while every tensor stays in the original token order (row n2).
        `cu_seqlens` (int32 [n_seq + 1]): x is a packed variable-length batch [1,total_T,C]; the shift does not cross a sequence
        boundary (zero in front of every sequence); rev_n is then int32 [n_seq].
        `shifted0` (packed batches only, [n_seq,C]): the token in front of every sequence -- what a serving loop carried over from the
        sequence's previous call -- instead of zero.
        `shift_pool` (bf16 [n_slots,C]) with `slots` (int32 [n_seq], None: the sequence index), instead of shifted0, on the packed fused
        path without autograd: the token in front of sequence s is shift_pool[slots[s]] (zero for a slot outside the pool), fetched by the
        kernel itself (mix_op.ddlerp_slots).
        With `fuse_lowrank` set, on the fused path, where nothing requires a gradient and rev_n is None, the blends are one call of
        mix_op.tmix_inputs and the decay one of mix_op.decay_lowrank (four launches for eleven), in the dense form, packed with shifted0 and
        packed with shift_pool / slots alike; any other call keeps the code below.  The transposed weight copies are kept on the module
        (_lowrank_weights) and rebuilt when a parameter's data_ptr() or _version changes, so a step that is captured in a graph needs one
        warm-up call before the capture: the copies must exist, and must not be part of what the graph replays."""
        B, T, C = x.size()
        if cu_seqlens is not None:
            assert B == 1 and shifted is None, "a packed batch is [1,total_T,C]; the carried tokens go in as shifted0 [n_seq,C]"
        else:
            assert shifted0 is None, "shifted0 belongs to a packed batch (cu_seqlens); a dense batch passes `shifted`"
        lowrank = self._use_lowrank(x, rev_n)               # fuse_lowrank: both low-rank pairs in two launches each (fused path only)
        if shift_pool is not None:
            assert cu_seqlens is not None and shifted0 is None and rev_n is None, \
                "shift_pool / slots belong to a packed batch (cu_seqlens) and exclude shifted0 and rev_n"
            if not self._use_fused(x):
                raise RuntimeError("shift_pool / slots exist in the fused (HIP) path only; gather the rows and pass shifted0")
            from . import mix_op
            if lowrank:
                maa_x, W1t, W2t, maa5 = self._lowrank_weights()[:4]
                xw, xk, xv, xr, xg = mix_op.tmix_inputs(x.contiguous(), maa_x, W1t, W2t, maa5, cu_seqlens, None, shift_pool, slots).unbind(0)
            else:
                lead = mix_op.ddlerp_slots(x, self.time_maa_x.view(1, C), None, shift_pool, slots, cu_seqlens)[0]
                low = torch.tanh(lead @ self.time_maa_w1).view(B * T, 5, -1).transpose(0, 1)
                corr = torch.bmm(low, self.time_maa_w2).view(5, B, T, C)
                xw, xk, xv, xr, xg = mix_op.ddlerp_slots(x, self._maa5(), corr, shift_pool, slots, cu_seqlens).unbind(0)
        elif self._use_fused(x):
            assert slots is None, "slots name rows of shift_pool"
            from . import mix_op
            first = None if shifted is None else shifted[:, 0].contiguous()
            if shifted0 is not None:
                first = shifted0.contiguous()
            if lowrank:
                maa_x, W1t, W2t, maa5 = self._lowrank_weights()[:4]
                xw, xk, xv, xr, xg = mix_op.tmix_inputs(x.contiguous(), maa_x, W1t, W2t, maa5, cu_seqlens, first).unbind(0)
            else:
                lead = mix_op.ddlerp(x, self.time_maa_x.view(1, C), None, first, rev_n, cu_seqlens=cu_seqlens)[0]
                low = torch.tanh(lead @ self.time_maa_w1).view(B * T, 5, -1).transpose(0, 1)
                corr = torch.bmm(low, self.time_maa_w2).view(5, B, T, C)
                xw, xk, xv, xr, xg = mix_op.ddlerp(x, self._maa5(), corr, first, rev_n, cu_seqlens=cu_seqlens).unbind(0)
        else:
            assert rev_n is None, "the reversed-stream shift exists in the fused (HIP) path only"
            assert slots is None, "slots name rows of shift_pool"
            if cu_seqlens is not None:
                prev = _packed_prev(x, cu_seqlens, shifted0)
            else:
                prev = F.pad(x, (0, 0, 1, -1)) if shifted is None else shifted
            delta = prev - x
            lead = torch.addcmul(x, delta, self.time_maa_x)
            low = torch.tanh(lead @ self.time_maa_w1).view(B * T, 5, -1).transpose(0, 1)
            corr = torch.bmm(low, self.time_maa_w2).view(5, B, T, C)
            xw, xk, xv, xr, xg = (x + delta * (self._maa5().view(5, 1, 1, C) + corr)).unbind(0)
        if lowrank:
            D1t, D2t, time_decay = self._lowrank_weights()[4:]
            decay = mix_op.decay_lowrank(xw, D1t, D2t, time_decay)
        else:
            decay = self.time_decay + torch.tanh(xw @ self.time_decay_w1) @ self.time_decay_w2
        return self.receptance(xr), self.key(xk), self.value(xv), F.silu(self.gate(xg)), decay

    def jit_func_2(self, x, g):
        """per-head GroupNorm, gate, output projection (src/model.py:462-468); on bf16 GPU tensors the GroupNorm and the
        gate multiply are one HIP kernel (mix_op.group_norm_gate)."""
        B, T, C = x.size()
        if self._use_fused(x):
            from . import mix_op
            gated = mix_op.group_norm_gate(x.reshape(B * T, C), g.reshape(B * T, C), self.ln_x.weight, self.ln_x.bias,
                                           self.n_head, self.ln_x.eps).view(B, T, C)
            return self.output(gated)
        return self.output(self.ln_x(x.view(B * T, C)).view(B, T, C) * g)

    def _run(self, r, k, v, w):
        B, T, C = r.shape
        return self.wkv(B, T, C, self.n_head, r, k, v, w, self.time_faaaa)

    def forward(self, x, cu_seqlens=None, max_seqlen=None):
        """causal time-mix (src/model.py:470-477).  With the HIP operator on bf16 GPU tensors the operator, the per-head
        GroupNorm and the gate multiply are ONE kernel (wkv.WKV_6_GN): y never leaves the chip on its way to
        the normalisation.
        cu_seqlens (int32 [n_seq + 1] on the device of x): x is a packed variable-length batch [1,total_T,C] -- the sequences back
        to back, no padding; token shift and operator restart at every boundary.  max_seqlen: the longest sequence (default:
        total_T, which is always safe; the kernels need (max_seqlen + 64) * C < 2^31)."""
        if cu_seqlens is not None:
            r, k, v, g, w = self.jit_func(x, cu_seqlens=cu_seqlens)
            _, T, C = r.shape
            y = self.wkv_varlen(T, C, self.n_head, r, k, v, w, self.time_faaaa, cu_seqlens, T if max_seqlen is None else max_seqlen)
            return self.jit_func_2(y, g)
        r, k, v, g, w = self.jit_func(x)
        if self.wkv is _default_wkv and self._use_fused(x) and self.fuse_epilogue:
            from .wkv import RUN_CUDA_RWKV6_GN
            B, T, C = r.shape
            gated = RUN_CUDA_RWKV6_GN(B, T, C, self.n_head, *(t.contiguous() for t in (r, k, v, w)), self.time_faaaa, g,
                                      self.ln_x.weight, self.ln_x.bias, self.ln_x.eps)
            return self.output(gated)
        return self.jit_func_2(self._run(r, k, v, w), g)

    def _rev_wkv(self, r, k, v, w, rev_n, rev_mask):
        from .wkv import WKV_6_REV
        B, T, C = r.shape
        bf = torch.bfloat16
        return WKV_6_REV.apply(B, T, C, self.n_head, *(t.to(bf).contiguous() for t in (r, k, v, w, self.time_faaaa)),
                               rev_n, rev_mask).to(r.dtype)

    def _pair_wkv(self, fwd, rev, rev_n, rev_mask):
        """Both operator calls of a bidirectional composition in one launch per pass (wkv.WKV_6_PAIR, row n2)."""
        from .wkv import WKV_6_PAIR
        B, T, C = fwd[0].shape
        bf = torch.bfloat16
        y, ry = WKV_6_PAIR.apply(B, T, C, self.n_head, *(t.to(bf).contiguous() for t in (*fwd, *rev)),
                                 self.time_faaaa.to(bf).contiguous(), rev_n, rev_mask)
        return y.to(fwd[0].dtype), ry.to(fwd[0].dtype)

    def _in_kernel_reversal(self, x):
        """Rows n2: with the HIP operator on bf16 GPU tensors the reversed half of the bidirectional compositions is
        addressed inside the kernels (wkv6_*_rev_ex, ddlerp rev_n) instead of through torch.gather round trips."""
        return self.wkv is _default_wkv and self._use_fused(x)

    def _packed_in_kernel(self, x):
        return self._in_kernel_reversal(x) and self.wkv_varlen is _default_wkv_varlen

    def _packed_bi(self, fwd, rev, cu_seqlens, max_seqlen, rev_n, rev_mask):
        """Both operator calls of a composition on a packed batch, in-kernel: the pair launch (wkv.WKV_6_VARLEN_PAIR) or, with
        pair_launch = False, the plain packed call and the packed call under the map."""
        from .wkv import RUN_CUDA_RWKV6_VARLEN, WKV_6_VARLEN_PAIR, WKV_6_VARLEN_REV
        _, T, C = fwd[0].shape
        bf = torch.bfloat16
        u = self.time_faaaa.to(bf).contiguous()
        f, r = [t.to(bf).contiguous() for t in fwd], [t.to(bf).contiguous() for t in rev]
        if self.pair_launch:
            y, ry = WKV_6_VARLEN_PAIR.apply(T, C, self.n_head, *f, *r, u, cu_seqlens, max_seqlen, rev_n, rev_mask)
        else:
            y = RUN_CUDA_RWKV6_VARLEN(T, C, self.n_head, *f, u, cu_seqlens, max_seqlen)
            ry = WKV_6_VARLEN_REV.apply(T, C, self.n_head, *r, u, cu_seqlens, max_seqlen, rev_n, rev_mask)
        return y.to(fwd[0].dtype), ry.to(fwd[0].dtype)

    def _run_packed(self, r, k, v, w, cu_seqlens, max_seqlen):
        _, T, C = r.shape
        return self.wkv_varlen(T, C, self.n_head, r, k, v, w, self.time_faaaa, cu_seqlens, max_seqlen)

    @staticmethod
    def _packed_defaults(x, cu_seqlens, max_seqlen, rev_n):
        """max_seqlen: total_T is always safe; rev_n: every sequence's full length."""
        if rev_n is None:
            rev_n = (cu_seqlens[1:] - cu_seqlens[:-1]).to(torch.int32)
        return (x.shape[1] if max_seqlen is None else max_seqlen), rev_n.contiguous()

    def forward_bi_c(self, x, rev_idx, mask=None, cu_seqlens=None, max_seqlen=None, rev_n=None):
        """composition C (src/model_ext.py:421-437): reverse the hidden states, project twice, average.
        cu_seqlens (int32 [n_seq + 1]): x is a packed batch [1,total_T,C]; the first rev_n[s] tokens (int32 [n_seq], default: all) of
        every sequence are reversed, rev_idx and mask are not used.  bf16 GPU tensors with the default operator run the reversal
        inside the kernels; everything else gathers through packed_reverse_idx around the wkv_varlen hook."""
        if cu_seqlens is not None:
            max_seqlen, rev_n = self._packed_defaults(x, cu_seqlens, max_seqlen, rev_n)
            r, k, v, g, w = self.jit_func(x, cu_seqlens=cu_seqlens)
            if self._packed_in_kernel(x):
                from .wkv6_op import REV_ALL
                rr, rk, rv, _, rw = self.jit_func(x, rev_n=rev_n, cu_seqlens=cu_seqlens)
                y, ry = self._packed_bi((r, k, v, w), (rr, rk, rv, rw), cu_seqlens, max_seqlen, rev_n, REV_ALL)
            else:
                idx = packed_reverse_idx(cu_seqlens, rev_n, x.shape[1])
                y = self._run_packed(r, k, v, w, cu_seqlens, max_seqlen)
                rr, rk, rv, _, rw = self.jit_func(x[:, idx], cu_seqlens=cu_seqlens)
                ry = self._run_packed(rr, rk, rv, rw, cu_seqlens, max_seqlen)[:, idx]
            return self.jit_func_2((y + ry) / 2, g)
        r, k, v, g, w = self.jit_func(x)
        if mask is not None and self._in_kernel_reversal(x):
            from .wkv6_op import REV_ALL
            rev_n = mask.sum(dim=1).to(torch.int32)
            rr, rk, rv, _, rw = self.jit_func(x, rev_n=rev_n)      # the reversed stream's projections, in original order
            if self.pair_launch:
                y, ry = self._pair_wkv((r, k, v, w), (rr, rk, rv, rw), rev_n, REV_ALL)
            else:
                y, ry = self._run(r, k, v, w), self._rev_wkv(rr, rk, rv, rw, rev_n, REV_ALL)
        else:
            y = self._run(r, k, v, w)
            rr, rk, rv, _, rw = self.jit_func(reverse_x(x, rev_idx))
            ry = reverse_x(self._run(rr, rk, rv, rw), rev_idx)
        return self.jit_func_2((y + ry) / 2, g)

    def forward_bi_b(self, x, mask=None, cu_seqlens=None, max_seqlen=None, rev_n=None):
        """composition B (src/model_bi.py:325-350): only k and v are reversed, outputs are added.
        cu_seqlens (int32 [n_seq + 1]): x is a packed batch [1,total_T,C]; rev_n (int32 [n_seq]) defaults to every sequence's full
        length, mask is not used."""
        if cu_seqlens is not None:
            max_seqlen, rev_n = self._packed_defaults(x, cu_seqlens, max_seqlen, rev_n)
            r, k, v, g, w = self.jit_func(x, cu_seqlens=cu_seqlens)
            if self._packed_in_kernel(x):
                from .wkv6_op import REV_K, REV_V, REV_Y
                y, ry = self._packed_bi((r, k, v, w), (r, k, v, w), cu_seqlens, max_seqlen, rev_n, REV_K | REV_V | REV_Y)
            else:
                idx = packed_reverse_idx(cu_seqlens, rev_n, x.shape[1])
                y = self._run_packed(r, k, v, w, cu_seqlens, max_seqlen)
                ry = self._run_packed(r, k[:, idx], v[:, idx], w, cu_seqlens, max_seqlen)[:, idx]
            return self.jit_func_2(y + ry, g)
        B, T, C = x.size()
        if mask is None:
            mask = torch.ones(B, T, device=x.device)
        r, k, v, g, w = self.jit_func(x)
        if self._in_kernel_reversal(x):
            from .wkv6_op import REV_K, REV_V, REV_Y
            rev_n = mask.sum(dim=1).to(torch.int32)
            if self.pair_launch:
                y, ry = self._pair_wkv((r, k, v, w), (r, k, v, w), rev_n, REV_K | REV_V | REV_Y)
            else:
                y, ry = self._run(r, k, v, w), self._rev_wkv(r, k, v, w, rev_n, REV_K | REV_V | REV_Y)
            return self.jit_func_2(y + ry, g)
        y = self._run(r, k, v, w)
        rev_idx = reverse_x_idx(mask, T)
        ry = self._run(r, reverse_x(k, rev_idx), reverse_x(v, rev_idx), w)
        return self.jit_func_2(y + reverse_x(ry, rev_idx), g)


class CMix_x060(nn.Module):
    """RWKV-6 channel-mix FFN (src/model.py:616-644): squared-ReLU key, sigmoid receptance gate.  On bf16 GPU tensors the
    elementwise glue between the three GEMMs runs as HIP kernels (mix_op: token shift + both lerps in one pass, relu^2, and
    sigmoid * value in one pass each) instead of ten eager kernels; `fused` = None picks by tensor type, True / False force."""

    def __init__(self, n_embd, dim_ffn, fused=None):
        super().__init__()
        self.fused = fused
        self.time_maa_k = nn.Parameter(torch.zeros(1, 1, n_embd))
        self.time_maa_r = nn.Parameter(torch.zeros(1, 1, n_embd))
        self.key = nn.Linear(n_embd, dim_ffn, bias=False)
        self.receptance = nn.Linear(n_embd, n_embd, bias=False)
        self.value = nn.Linear(dim_ffn, n_embd, bias=False)

    def _use_fused(self, x):
        if self.fused is None:
            from . import mix_op
            C = x.shape[-1]
            return (mix_op.fusable(x, self.time_maa_k, self.time_maa_r) and x.dim() == 3 and C % 64 == 0 and C <= 4096
                    and self.key.weight.dtype == torch.bfloat16)
        return self.fused

    def forward(self, x, cu_seqlens=None, max_seqlen=None):
        """cu_seqlens (int32 [n_seq + 1]): x is a packed variable-length batch [1,total_T,C]; the token shift does not cross a
        sequence boundary.  (max_seqlen is accepted for symmetry with Tmix_x060.forward; the FFN has no use for it.)"""
        if self._use_fused(x):
            from . import mix_op
            xk, xr = mix_op.ddlerp(x, torch.cat([self.time_maa_k, self.time_maa_r], 0).view(2, -1), cu_seqlens=cu_seqlens)
            k = mix_op.sqrelu(self.key(xk))
            return mix_op.sigmoid_mul(self.receptance(xr), self.value(k))
        xx = (F.pad(x, (0, 0, 1, -1)) if cu_seqlens is None else _packed_prev(x, cu_seqlens)) - x
        k = torch.relu(self.key(x + xx * self.time_maa_k)) ** 2
        return torch.sigmoid(self.receptance(x + xx * self.time_maa_r)) * self.value(k)


class BiBlock(nn.Module):
    """src/model_encoder_run.py:222-259 (pre-LN residual block, ln0 on the first layer)."""

    def __init__(self, n_embd, dim_att, dim_ffn, layer_id, wkv=None, wkv_varlen=None):
        super().__init__()
        self.layer_id = layer_id
        self.ln1 = nn.LayerNorm(n_embd)
        self.ln2 = nn.LayerNorm(n_embd)
        if layer_id == 0:
            self.ln0 = nn.LayerNorm(n_embd)
        self.att = Tmix_x060(n_embd, dim_att, wkv=wkv, wkv_varlen=wkv_varlen)
        self.ffn = CMix_x060(n_embd, dim_ffn)

    def forward(self, x, rev_idx, mask, cu_seqlens=None, max_seqlen=None, rev_n=None):
        """cu_seqlens / max_seqlen / rev_n: x is a packed batch [1,total_T,C] (Tmix_x060.forward_bi_c); rev_idx and mask are not used."""
        if self.layer_id == 0:
            x = self.ln0(x)
        if cu_seqlens is not None:
            x = x + self.att.forward_bi_c(self.ln1(x), None, None, cu_seqlens=cu_seqlens, max_seqlen=max_seqlen, rev_n=rev_n)
            return x + self.ffn(self.ln2(x), cu_seqlens=cu_seqlens)
        x = x + self.att.forward_bi_c(self.ln1(x), rev_idx, mask)
        return x + self.ffn(self.ln2(x))


class RwkvEncoder(nn.Module):
    """Bidirectional RWKV-6 encoder (src/model_encoder_run.py:262-348, share_emb, no head_qk, no dropout)."""

    def __init__(self, vocab_size, n_embd, n_layer, dim_att=None, dim_ffn=None, emb_id=1, pad_id=0, wkv=None, wkv_varlen=None):
        super().__init__()
        self.emb_id, self.pad_id = emb_id, pad_id
        self.emb = nn.Embedding(vocab_size, n_embd)
        self.blocks = nn.ModuleList([BiBlock(n_embd, dim_att or n_embd, dim_ffn or 4 * n_embd, i, wkv=wkv, wkv_varlen=wkv_varlen)
                                     for i in range(n_layer)])
        self.ln_out = nn.LayerNorm(n_embd)

    def forward(self, idx, return_logits=False, cu_seqlens=None, max_seqlen=None):
        """cu_seqlens (int32 [n_seq + 1] on the device of idx): idx is a packed batch [1,total_T], the sequences back to back without
        pad tokens; rev_n[s] = the number of ordinary tokens of sequence s (a segment sum of create_mask, on the device)."""
        B, T = idx.size()
        mask = create_mask(idx, emb_id=self.emb_id, pad_id=self.pad_id)
        x = self.emb(idx)
        if cu_seqlens is not None:
            assert B == 1, "a packed batch is [1,total_T]"
            csum = F.pad(mask[0].cumsum(0), (1, 0))
            cu = cu_seqlens.long().clamp(0, T)
            rev_n = (csum[cu[1:]] - csum[cu[:-1]]).to(torch.int32)
            for block in self.blocks:
                x = block(x, None, None, cu_seqlens=cu_seqlens, max_seqlen=max_seqlen, rev_n=rev_n)
        else:
            rev_idx = reverse_x_idx(mask, T)
            for block in self.blocks:
                x = block(x, rev_idx, mask)
        hidden = self.ln_out(x)
        logits = torch.matmul(hidden, self.emb.weight.t())
        return (logits, hidden) if return_logits else logits

    def encode_sentence(self, idx, cu_seqlens=None, max_seqlen=None):
        """With cu_seqlens: one vector per sequence of the packed idx [1,total_T], taken at the sequence's first emb_id token (its first
        token when it has none, as argmax gives on a padded row)."""
        if cu_seqlens is not None:
            _, hidden = self.forward(idx, True, cu_seqlens=cu_seqlens, max_seqlen=max_seqlen)
            T = idx.size(1)
            count = torch.eq(idx[0], self.emb_id).long().cumsum(0)                   # emb_id tokens up to and including each row
            cu = cu_seqlens.long().clamp(0, T)
            before = F.pad(count, (1, 0))[cu[:-1]]
            position = torch.searchsorted(count, before + 1)                          # the first row whose count reaches before + 1
            position = torch.where(position < cu[1:], position, cu[:-1]).clamp(max=T - 1)
            return hidden[0, position]
        _, hidden = self.forward(idx, True)
        position = torch.eq(idx, self.emb_id).int().argmax(-1)
        return hidden[torch.arange(hidden.size(0)), position]


# ---- a17: embedding head ---------------------------------------------------------------------------------------
def pooling(x, actual_len, pooling_type="weightedmean"):
    """src/model_ext.py:1708-1738.  actual_len[b] = index of the first emb_id token of row b."""
    T = x.size(1)
    if pooling_type == "weightedmean":
        mask = torch.arange(T, device=x.device) <= actual_len.unsqueeze(1)
        weights = torch.arange(1, T + 1, device=x.device).unsqueeze(0).float() / actual_len.unsqueeze(1).float()
        weights = weights * mask.float()
        x = torch.sum(x * weights.unsqueeze(-1), dim=1) / actual_len.unsqueeze(1).float()
        return x.bfloat16()
    if pooling_type == "lasttoken":
        return x[torch.arange(x.size(0)), actual_len]
    if pooling_type == "avg":
        mask = (torch.arange(T, device=x.device).unsqueeze(0) < actual_len.unsqueeze(1)).to(x.dtype)
        return (torch.sum(x * mask.unsqueeze(-1), dim=1) / actual_len.unsqueeze(1).float()).bfloat16()
    raise ValueError(pooling_type)


def _pool_kernel(x, cu_seqlens, actual_len, kernels):
    """Whether mix_op.pool_packed serves this call (kernels as in infctx._sample_kernel: None where it applies, False never, True it
    must -- then mix_op says what is wrong)."""
    if kernels is False:
        return False
    if kernels:
        return True
    def ints(t):
        return isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_contiguous() and t.device == x.device
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and x.shape[-1] % 8 == 0 and x.data_ptr() % 16 == 0
            and ints(cu_seqlens) and (actual_len is None or ints(actual_len)))


def pooling_packed(x, cu_seqlens, actual_len=None, pooling_type="weightedmean", kernels=None):
    """`pooling` on a packed batch x [1,total_T,C] (or [total_T,C]) -> [n_seq,C]: sequence s holds rows cu_seqlens[s] .. cu_seqlens[s+1]-1
    and is pooled at a_s = clamp(actual_len[s], 0, len_s - 1) (actual_len None: its last token), its position of the first emb_id token.
    The operation is stated in include/wkv6_amd.h (wkv6_pool_packed_forward): fp32 sums rounded once -- to bf16 for the two means, as the
    dense function returns them; "lasttoken" is a copy in the type of x --, a NaN row where a_s == 0, a zero row for an empty sequence,
    and rows outside every sequence or past a_s are never read (the dense function multiplies them by zero: NaN * 0).
    kernels: None = the HIP kernels (mix_op.pool_packed) where they apply -- contiguous bf16 x on the GPU, contiguous int32 arrays on its
    device --, else the eager restatement below (CPU, fp32, fp16; differentiable by autograd; on the GPU its index_add sums in no fixed
    order); False = always eager; True = the kernels or their error.  Neither path reads the int arrays on the host."""
    if pooling_type not in ("weightedmean", "lasttoken", "avg"):
        raise ValueError(pooling_type)
    if _pool_kernel(x, cu_seqlens, actual_len, kernels):
        from . import mix_op
        return mix_op.pool_packed(x, cu_seqlens, actual_len, pooling_type)
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    T, n_seq = x2.shape[0], cu_seqlens.numel() - 1
    cu = cu_seqlens.long().clamp(0, T)
    start = cu[:-1]
    length = (cu[1:] - start).clamp_min(0)
    a = length - 1 if actual_len is None else torch.minimum(actual_len.long().clamp_min(0), length - 1)
    if pooling_type == "lasttoken":
        row = x2[(start + a).clamp(0, T - 1)]
        return torch.where((length > 0).unsqueeze(1), row, torch.zeros_like(row))
    pos = torch.arange(T, device=x.device)
    seq = torch.searchsorted(cu_seqlens.long()[:-1].contiguous(), pos, right=True) - 1        # the last s with cu_seqlens[s] <= row
    at = seq.clamp_min(0)
    t = pos - start[at]
    n = a + 1 if pooling_type == "weightedmean" else a                                        # tokens 0 .. n - 1 are summed
    summed = (seq >= 0) & (t >= 0) & (t < length[at]) & (t < n[at])
    weight = (t + 1).float() if pooling_type == "weightedmean" else torch.ones(T, device=x.device)
    terms = torch.where(summed.unsqueeze(1), x2.float() * weight.unsqueeze(1), torch.zeros((), device=x.device))
    total = torch.zeros(n_seq, C, device=x.device).index_add(0, at, terms)
    fa = a.clamp_min(1).float().unsqueeze(1)
    out = total / fa / fa if pooling_type == "weightedmean" else total / fa
    out = out * torch.where(a == 0, float("nan"), 1.0).to(out).unsqueeze(1)                  # 0 / 0; the gradient of such a row is NaN too
    return torch.where((length > 0).unsqueeze(1), out, torch.zeros((), device=x.device)).bfloat16()


def cos_sim(a, b):
    """sentence_transformers.util.cos_sim: all pairs, [len(a), len(b)]."""
    return F.normalize(a, p=2, dim=1) @ F.normalize(b, p=2, dim=1).t()


def pairwise_cos_sim(a, b):
    """sentence_transformers.util.pairwise_cos_sim: row i of a with row i of b."""
    return (F.normalize(a, p=2, dim=1) * F.normalize(b, p=2, dim=1)).sum(-1)


def info_nce_loss(query, positive, negative=None, scale=20.0):
    """In-batch-negative loss of RwkvForSequenceEmbedding.training_step (src/model_ext.py:1897-1911):
    CE([cos_sim(q, p) * 20 | pairwise_cos_sim(q, n) * 20], arange(bs)); negatives are per rank only."""
    scores = cos_sim(query, positive) * scale
    if negative is not None:
        scores = torch.cat([scores, pairwise_cos_sim(query, negative).unsqueeze(1) * scale], dim=1)
    labels = torch.arange(scores.shape[0], dtype=torch.long, device=scores.device)
    return F.cross_entropy(scores, labels)


# ---- the LM head's loss: F.cross_entropy + L2Wrap (src/model.py:937-974, 1244-1283) ------------------------------------------------
# What kernels=None means for lm_loss where the kernels apply (profiles/ce_rows_time.txt, measured at V = 65536 only): the two launches
# behind autograd beat torch's own cross-entropy + L2Wrap 3.3x at 4096 rows and 3.65x at 49152 rows, and lose 1.4x at 256 rows, where
# both are bound by the host's launches and this path makes more of them.  None takes the kernels from the smallest size at which they
# were measured faster, counted in logits.  Where the crossover lies between 256 and 4096 rows, and where it lies for another V -- the
# host's cost goes with the calls, not with the elements -- is not measured.  (head_loss runs the fused launch per chunk, which was
# faster than torch at every size measured: 4.0x at 256 rows.)
CE_KERNELS_FROM = 4096 * 65536


class _L2Wrap(torch.autograd.Function):
    """The reference's L2Wrap (src/model.py:937-974): the loss passes through; in the backward every row of the logits gets factor * max
    at its argmax, NOT multiplied by the incoming gradient.  factor: a float or a 0-d tensor; rows (a [rows] tensor or None) weights it."""

    @staticmethod
    def forward(ctx, loss, y, factor, rows):
        ctx.save_for_backward(y, rows)
        ctx.factor = factor
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        y, rows = ctx.saved_tensors
        maxx, ids = torch.max(y, -1, keepdim=True)
        gy = torch.zeros_like(y)
        term = maxx * ctx.factor
        if rows is not None:
            term = term * rows.to(term.dtype).view(term.shape)
        gy.scatter_(-1, ids, term.to(y.dtype))
        return grad_output, gy, None, None


def _l2_factor(l2wrap, rows, token_amount):
    """l2wrap / (B * T), or l2wrap / token_amount (the infctx form; a device tensor stays one); None: the term is off."""
    if not l2wrap or (not isinstance(token_amount, torch.Tensor) and token_amount == 0):
        return None
    return l2wrap / (rows if token_amount is None else token_amount)


_CE_TYPES = (torch.bfloat16, torch.float16, torch.float32)


def _ce_kernel(z, targets, kernels):
    """Whether mix_op.ce_rows serves logits rows z [rows, V] (kernels as in _pool_kernel): under None, where mix_op would accept them --
    its dtype, layout, alignment and device tests -- and the size is one at which the kernels were measured faster."""
    if kernels is False:
        return False
    if kernels:
        return True
    if not (z.is_cuda and z.dtype in _CE_TYPES and z.shape[0] * z.shape[1] >= CE_KERNELS_FROM and z.stride(1) == 1):
        return False
    from . import mix_op
    return (mix_op._ce_ld(z) is not None and z.data_ptr() % 16 == 0 and targets.dtype == torch.int64 and targets.device == z.device
            and targets.is_contiguous())


def _row_scales(targets, mask, factor, l2_rows):
    """(ce_scale, l2_scale) fp32 [rows] of the final loss, from device data alone: the weight of every row's loss in
    mean-over-non-ignored (or sum(loss * mask) / sum(mask)), and the L2 factor of every row."""
    if mask is None:
        valid = (targets != -100).float()
        ce = valid / valid.sum()
    else:
        m = mask.reshape(-1).float()
        ce = m / m.sum()
    if factor is None:
        l2 = torch.zeros_like(ce)
    else:
        l2 = torch.ones_like(ce) * factor
        if l2_rows is not None:
            l2 = l2 * l2_rows.reshape(-1).float()
    return ce.contiguous(), l2.contiguous()


def lm_loss(logits, targets, mask=None, l2wrap=1e-4, token_amount=None, kernels=None, l2_rows=None):
    """The loss of the reference's training_step on logits [B,T,V] (or packed [total_T,V]) and int64 targets of the leading shape
    (-100: the row is ignored): the mean of F.cross_entropy over the non-ignored rows, or with mask sum(loss * mask) / sum(mask) (my_qa_mask),
    then L2Wrap: in the backward every row of the logits -- ignored ones included, as in the reference -- gets l2wrap / (B * T) * max at
    its argmax, l2wrap / token_amount with token_amount (the infctx form; an int or a 0-d device tensor), not multiplied by the incoming
    gradient.  l2wrap = 0 turns it off; l2_rows ([rows] of 0 / 1, or None) names the rows that take it.  Every count stays on the device.
    kernels: None = the HIP kernels (mix_op.ce_rows: one pass for the statistics, one for the gradient, fp32 loss) where they apply and
    were measured faster -- GPU, rows a multiple of 8 elements apart, at least CE_KERNELS_FROM logits --, else the eager three lines below (CPU; double backward; the loss in the type of the
    logits); False = always eager; True = the kernels or their error."""
    V = logits.shape[-1]
    z, t = logits.reshape(-1, V), targets.reshape(-1)
    factor = _l2_factor(l2wrap, z.shape[0], token_amount)
    if _ce_kernel(z, t, kernels):
        from . import mix_op
        ce, l2 = _row_scales(t, mask, factor, l2_rows)
        return (mix_op.ce_rows(z, t, None if factor is None else l2) * ce).sum()
    if mask is None:
        loss = F.cross_entropy(z, t)
    else:
        m = mask.reshape(-1)
        loss = torch.sum(F.cross_entropy(z, t, reduction="none") * m) / torch.sum(m)
    return loss if factor is None else _L2Wrap.apply(loss, logits, factor, l2_rows)


def _ce_rows_grad_eager(z, t, ce, l2):
    """mix_op.ce_rows_grad_ restated: (loss_row fp32, the gradient in the type of z) of a chunk z [n,V]."""
    zf = z.float()
    lse = torch.logsumexp(zf, -1)
    valid = t != -100
    at = t.clamp_min(0).unsqueeze(1)
    loss = torch.where(valid, lse - zf.gather(1, at)[:, 0], torch.zeros_like(lse))
    g = torch.exp(zf - lse.unsqueeze(1))
    g.scatter_add_(1, at, -torch.ones_like(lse).unsqueeze(1))
    g = g * (ce * valid).unsqueeze(1)
    zmax, imax = zf.max(-1)
    g.scatter_add_(1, imax.unsqueeze(1), (l2 * zmax).unsqueeze(1))
    return loss, g.to(z.dtype)


def _gw_gemm(g, x, out):
    """out = g^T x [V,C]: the head's weight gradient of one chunk (a function of its own so that a test can count its calls)."""
    return torch.mm(g.t(), x, out=out)


class _HeadLoss(torch.autograd.Function):
    """sum_r ce_scale[r] * loss_row[r] of the logits x W^T, walked in chunks of chunk_rows rows of x through one reused logits buffer:
    GEMM, the fused cross-entropy kernel in place (the buffer then holds the chunk's logits gradient, final scales and all), gx = g W
    where x takes a gradient, and gW += g^T x where W does: each chunk's product is one GEMM in the type of x (for bf16: fp32 sums inside
    the GEMM, rounded to bf16 once, into one reused [V,C] buffer) and the chunks are added up in fp32.  The backward scales the stored
    gradients by the incoming one."""

    @staticmethod
    def forward(ctx, x, weight, targets, ce, l2, chunk_rows, use_kernels):
        rows, V = x.shape[0], weight.shape[0]
        ld = (V + 7) // 8 * 8
        buf = torch.empty((min(chunk_rows, rows), ld), device=x.device, dtype=x.dtype)
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gW = torch.zeros(weight.shape, device=x.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        gW_chunk = None if gW is None else torch.empty_like(weight)             # one chunk's product, in the type of the GEMM
        loss_rows = torch.empty(rows, device=x.device, dtype=torch.float32)
        if use_kernels:
            from . import mix_op
        for a in range(0, rows, chunk_rows):
            b = min(a + chunk_rows, rows)
            z = buf[:b - a, :V]
            torch.mm(x[a:b], weight.t(), out=z)
            if use_kernels:
                loss_rows[a:b] = mix_op.ce_rows_grad_(z, targets[a:b], ce[a:b], l2[a:b])
            else:
                loss_rows[a:b], g = _ce_rows_grad_eager(z, targets[a:b], ce[a:b], l2[a:b])
                z.copy_(g)
            if gx is not None:
                torch.mm(z, weight, out=gx[a:b])
            if gW is not None:
                gW += _gw_gemm(z, x[a:b], gW_chunk)
        ctx.save_for_backward(gx, gW)
        ctx.wdtype = weight.dtype
        return (loss_rows * ce).sum()

    @staticmethod
    def backward(ctx, gloss):
        gx, gW = ctx.saved_tensors
        return (None if gx is None else gx * gloss.to(gx.dtype), None if gW is None else (gW * gloss).to(ctx.wdtype), None, None, None,
                None, None)


def head_loss(x, weight, targets, mask=None, l2wrap=1e-4, token_amount=None, chunk_rows=4096, kernels=None, l2_rows=None):
    """lm_loss(x @ weight.T, targets, ...) without ever holding the [rows, V] logits: x [.., C] is the hidden state behind ln_out, weight
    [V, C] the bias-free head.  One autograd function walks x in chunks of chunk_rows rows; per chunk a logits GEMM into one reused buffer,
    the fused cross-entropy kernel in place with the FINAL scales (they come from targets and mask alone, on the device), gx = g W, and
    -- only if weight.requires_grad; a frozen head under LoRA skips that GEMM -- gW += g^T x, each chunk's product rounded to the type of
    x by its GEMM and the chunks summed in fp32.  Peak extra memory: chunk_rows * ld elements of logits (ld = V rounded up to 8) plus gx
    (plus, for a trainable head, an fp32 gW and one [V, C] chunk product).
    The backward multiplies the stored gx (and gW) by the incoming scalar gradient.  That also scales the L2 term, which L2Wrap -- and
    lm_loss -- leave unscaled: the two agree where the incoming gradient is 1, as at the loss.backward() of a training step, and differ
    under loss scaling or gradient accumulation by division.  No double backward.
    kernels: None = mix_op.ce_rows_grad_ on the GPU, an eager restatement of it per chunk elsewhere; False = always eager; True = the
    kernel or its error."""
    C = x.shape[-1]
    x2, t = x.reshape(-1, C), targets.reshape(-1)
    if weight.dim() != 2 or weight.shape[1] != C or weight.dtype != x.dtype:
        raise RuntimeError(f"head_loss: weight must be [V, C = {C}] in the type of x")
    if t.shape[0] != x2.shape[0] or chunk_rows < 1:
        raise RuntimeError("head_loss: targets must have one entry per row of x, chunk_rows must be >= 1")
    ce, l2 = _row_scales(t, mask, _l2_factor(l2wrap, x2.shape[0], token_amount), l2_rows)
    # None: the fused kernel where mix_op.ce_rows_grad_ accepts the chunk (the buffer's layout is this function's own)
    use = bool(kernels) if kernels is not None else (x.is_cuda and x.dtype in _CE_TYPES and t.dtype == torch.int64 and t.device == x.device)
    return _HeadLoss.apply(x2, weight, t, ce, l2, int(chunk_rows), use)


# ---- RWKV-5 time-mix (src/model.py:292-374) ------------------------------------------------------------------------
def _default_wkv5(B, T, C, H, r, k, v, w, u):
    from .wkv import RUN_CUDA_RWKV5
    bf = torch.bfloat16
    y = RUN_CUDA_RWKV5(B, T, C, H, *(t.to(bf).contiguous() for t in (r, k, v, w, u)))
    return y.to(r.dtype)


class RWKV_Tmix_x052(nn.Module):
    """RWKV-5 time-mix around the WKV5 operator (RWKV_TimeMix_RWKV5, src/model.py:292-374): token shift, four static lerps,
    r / k / v / gate projections, the operator with the [H,N] parameters time_decay (raw w) and time_faaaa (u),
    GroupNorm_H(y / head_size_divisor) * silu-gate, output projection.  Parameter names are the reference's state_dict keys;
    everything around the operator is plain PyTorch."""

    def __init__(self, n_embd, dim_att, head_size=64, head_size_divisor=8, wkv=None):
        super().__init__()
        assert dim_att % head_size == 0
        self.n_head = dim_att // head_size
        self.head_size_divisor = head_size_divisor
        self.wkv = wkv or _default_wkv5
        z = lambda *s: nn.Parameter(torch.zeros(*s))
        for n in ("k", "v", "r", "g"):
            setattr(self, "time_mix_" + n, z(1, 1, n_embd))
        self.time_decay = z(self.n_head, head_size)
        self.time_faaaa = z(self.n_head, head_size)
        self.receptance = nn.Linear(n_embd, dim_att, bias=False)
        self.key = nn.Linear(n_embd, dim_att, bias=False)
        self.value = nn.Linear(n_embd, dim_att, bias=False)
        self.output = nn.Linear(dim_att, n_embd, bias=False)
        self.gate = nn.Linear(n_embd, dim_att, bias=False)
        self.ln_x = nn.GroupNorm(self.n_head, dim_att)

    @torch.no_grad()
    def init_like_reference(self, layer_id, n_layer):
        """The reference's initial values of the mix weights, the decay ramp and the bonus (src/model.py:304-329)."""
        n_embd, dim_att = self.time_mix_k.shape[-1], self.time_decay.numel()
        r01 = layer_id / max(n_layer - 1, 1)
        r10 = 1.0 - layer_id / n_layer
        ddd = (torch.arange(n_embd, dtype=torch.float32) / n_embd).view(1, 1, n_embd)
        self.time_mix_k.copy_(ddd.pow(r10))
        self.time_mix_v.copy_(ddd.pow(r10) + 0.3 * r01)
        self.time_mix_r.copy_(ddd.pow(0.5 * r10))
        self.time_mix_g.copy_(ddd.pow(0.5 * r10))
        n = torch.arange(dim_att, dtype=torch.float32)
        self.time_decay.copy_((-6 + 5 * (n / (dim_att - 1)) ** (0.7 + 1.3 * r01)).view_as(self.time_decay))
        zigzag = ((n + 1) % 3 - 1) * 0.1
        self.time_faaaa.copy_((r01 * (1 - n / (dim_att - 1)) + zigzag).view_as(self.time_faaaa))
        return self

    def jit_func(self, x):
        xx = F.pad(x, (0, 0, 1, -1))                                    # nn.ZeroPad2d((0, 0, 1, -1))
        xk = x * self.time_mix_k + xx * (1 - self.time_mix_k)
        xv = x * self.time_mix_v + xx * (1 - self.time_mix_v)
        xr = x * self.time_mix_r + xx * (1 - self.time_mix_r)
        xg = x * self.time_mix_g + xx * (1 - self.time_mix_g)
        return self.receptance(xr), self.key(xk), self.value(xv), F.silu(self.gate(xg))

    def jit_func_2(self, x, g):
        B, T, C = x.size()
        # GroupNorm_H(y / divisor) written out on [B*T, H, N] in at least fp32 (y / 8 has a variance not far above eps), then back to
        # the module's dtype for the gate and the output projection
        H = self.n_head
        ct = torch.promote_types(x.dtype, torch.float32)
        xh = x.reshape(B * T, H, C // H).to(ct) / self.head_size_divisor
        xh = xh - xh.mean(-1, keepdim=True)
        xh = xh * torch.rsqrt(xh.square().mean(-1, keepdim=True) + self.ln_x.eps)
        x = (xh.reshape(B * T, C) * self.ln_x.weight.to(ct) + self.ln_x.bias.to(ct)).to(g.dtype).view(B, T, C)
        return self.output(x * g)

    def forward(self, x):
        r, k, v, g = self.jit_func(x)
        B, T, C = r.shape
        y = self.wkv(B, T, C, self.n_head, r, k, v, self.time_decay, self.time_faaaa)
        return self.jit_func_2(y, g)
