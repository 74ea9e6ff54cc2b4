"""Tmix_x060 / CMix_x060 on a packed variable-length batch (forward(x, cu_seqlens=...)), CPU tier: fp32, the token shift on the eager
path and the CPU oracle standing in for the operator through the modules' two hooks.  Expectation: the same module run on every sequence
alone ([1, len_s, C]) and the results concatenated; likewise the parameter gradients (summed over the sequences)."""
import numpy as np
import pytest
import torch

from conftest import max_norm_err
from oracle import caller_weights as cw
from oracle.contract import F32_TOL
from rwkv_lm_ext_amd import callers
from varlen_common import CALLER_LENS, cu_of


def make_oracle_fn(oracle):
    class OracleWkv(torch.autograd.Function):
        @staticmethod
        def forward(ctx, r, k, v, w, u):
            ctx.save_for_backward(r, k, v, w, u)
            f = lambda t: t.detach().float().numpy()
            return torch.from_numpy(oracle.forward(f(r), f(k), f(v), f(w), f(u)))

        @staticmethod
        def backward(ctx, gy):
            f = lambda t: t.detach().float().contiguous().numpy()
            g = oracle.backward(*(f(t) for t in ctx.saved_tensors), f(gy))
            return tuple(torch.from_numpy(g[n]) for n in ("gr", "gk", "gv", "gw", "gu"))
    return OracleWkv.apply


@pytest.fixture(scope="module")
def hooks(oracle):
    fn = make_oracle_fn(oracle)

    def wkv(B, T, C, H, r, k, v, w, u):
        return fn(r, k, v, w, u)

    def wkv_varlen(total_T, C, H, r, k, v, w, u, cu_seqlens, max_seqlen):
        """every sequence alone through the oracle (B = 1, T = len_s), concatenated; an empty sequence contributes nothing"""
        cu = cu_seqlens.tolist()
        assert cu[-1] == total_T and max_seqlen >= max(b - a for a, b in zip(cu, cu[1:]))
        parts = [fn(*(t[:, a:b] for t in (r, k, v, w)), u) for a, b in zip(cu, cu[1:]) if b > a]
        return torch.cat(parts, 1)
    return wkv, wkv_varlen


def packed_input(C, seed):
    lens = CALLER_LENS
    assert lens == [1, 2, 63, 64, 65, 130, 0, 7]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, sum(lens), C, generator=g)
    return lens, torch.from_numpy(cu_of(lens)), x


def per_sequence(module, x, lens):
    outs, t0 = [], 0
    for n in lens:
        if n:
            outs.append(module(x[:, t0:t0 + n]))
        t0 += n
    return torch.cat(outs, 1)


def grads_of(module, out, gy):
    module.zero_grad()
    out.backward(gy)
    return {n: p.grad.clone() for n, p in module.named_parameters()}


def first_tokens(lens):
    cu = cu_of(lens)
    return [int(cu[s]) for s in range(1, len(lens)) if lens[s] > 0]


def leak_at_every_later_first_token(dense, want, lens):
    """the dense module on the packed tensor (no cu_seqlens) lets the shift / the state run across the boundaries: it must differ from
    the expectation at the first token of every sequence after the first"""
    for t in first_tokens(lens):
        assert max_norm_err(dense[:, t], want[:, t]) > 100 * F32_TOL, t
    assert max_norm_err(dense[:, 0], want[:, 0]) <= F32_TOL                   # the first sequence's first token has nothing in front of it


def test_time_mix_packed_equals_per_sequence(hooks):
    wkv, wkv_varlen = hooks
    tm = callers.Tmix_x060(cw.N_EMBD, cw.DIM_ATT, wkv=wkv, wkv_varlen=wkv_varlen, fused=False)
    tm.load_state_dict(cw.tmix_weights(torch.Generator().manual_seed(11), layer_id=1), strict=True)
    lens, cu, x = packed_input(cw.N_EMBD, 5)
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(6))
    want = per_sequence(tm, x, lens)
    gwant = grads_of(tm, want, gy)
    got = tm(x, cu_seqlens=cu, max_seqlen=max(lens))
    ggot = grads_of(tm, got, gy)
    assert got.shape == x.shape
    assert max_norm_err(got.detach(), want.detach()) <= F32_TOL
    assert max_norm_err(tm(x, cu_seqlens=cu).detach(), want.detach()) <= F32_TOL          # max_seqlen defaults to total_T
    assert set(ggot) == set(gwant) and len(ggot) >= 17
    for n in gwant:
        assert max_norm_err(ggot[n], gwant[n]) <= F32_TOL, n
    with torch.no_grad():
        leak_at_every_later_first_token(tm(x), want, lens)


def test_channel_mix_packed_equals_per_sequence():
    cm = callers.CMix_x060(cw.N_EMBD, cw.DIM_FFN, fused=False)
    cm.load_state_dict(cw.cmix_weights(torch.Generator().manual_seed(12)), strict=True)
    lens, cu, x = packed_input(cw.N_EMBD, 7)
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(8))
    want = per_sequence(cm, x, lens)
    gwant = grads_of(cm, want, gy)
    got = cm(x, cu_seqlens=cu, max_seqlen=max(lens))
    ggot = grads_of(cm, got, gy)
    assert max_norm_err(got.detach(), want.detach()) <= F32_TOL
    for n in gwant:
        assert max_norm_err(ggot[n], gwant[n]) <= F32_TOL, n
    with torch.no_grad():
        leak_at_every_later_first_token(cm(x), want, lens)


def test_default_none_changes_nothing(hooks):
    wkv, wkv_varlen = hooks
    tm = callers.Tmix_x060(cw.N_EMBD, cw.DIM_ATT, wkv=wkv, wkv_varlen=wkv_varlen, fused=False)
    tm.load_state_dict(cw.tmix_weights(torch.Generator().manual_seed(11), layer_id=1), strict=True)
    cm = callers.CMix_x060(cw.N_EMBD, cw.DIM_FFN, fused=False)
    cm.load_state_dict(cw.cmix_weights(torch.Generator().manual_seed(12)), strict=True)
    x = torch.randn(2, 24, cw.N_EMBD, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        assert torch.equal(tm(x), tm(x, cu_seqlens=None, max_seqlen=None))
        assert torch.equal(cm(x), cm(x, None, None))
        # one sequence that is the whole tensor: the packed path is the dense one
        one = torch.tensor([0, 24], dtype=torch.int32)
        assert max_norm_err(tm(x[:1], cu_seqlens=one), tm(x[:1])) <= F32_TOL
        assert torch.equal(cm(x[:1], cu_seqlens=one), cm(x[:1]))
