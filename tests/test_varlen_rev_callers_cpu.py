"""The bidirectional compositions on a packed variable-length batch, CPU tier: fp32, eager token shift (fused=False), the CPU oracle
standing in for the operator through the hooks of tests/test_varlen_callers_cpu.py -- so the packed path here is the gather formulation
through callers.packed_reverse_idx.  Expectation: the same module run on every sequence alone and the results concatenated, outputs and
every parameter gradient, within F32_TOL."""
import pytest
import torch

from conftest import max_norm_err
from oracle import caller_weights as cw
from oracle.contract import F32_TOL
from rwkv_lm_ext_amd import callers
from test_varlen_callers_cpu import grads_of, hooks, packed_input  # noqa: F401  (hooks: the fixture)
from varlen_common import CALLER_LENS, cu_of

LENS = CALLER_LENS
REV = {"len": list(LENS), "len-1": [max(n - 1, 0) for n in LENS], "zero": [0] * len(LENS), "mixed": [1, 0, 17, 64, 33, 65, 0, 3]}


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32)


def test_packed_reverse_idx_known_answer():
    cu, rev = i32([0, 3, 3, 4, 9]), i32([3, 0, 0, 4])                          # lengths 3, 0, 1, 5
    idx = callers.packed_reverse_idx(cu, rev, 9)
    assert idx.tolist() == [2, 1, 0, 3, 7, 6, 5, 4, 8]
    assert idx[idx].tolist() == list(range(9))                                  # its own inverse
    # clamped to the sequence; rows of no sequence stay in place
    assert callers.packed_reverse_idx(i32([1, 3, 4]), i32([9, -2]), 6).tolist() == [0, 2, 1, 3, 4, 5]


def time_mix(hooks):
    wkv, wkv_varlen = hooks
    tm = callers.Tmix_x060(cw.N_EMBD, cw.DIM_ATT, wkv=wkv, wkv_varlen=wkv_varlen, fused=False)
    tm.load_state_dict(cw.tmix_weights(torch.Generator().manual_seed(11), layer_id=1), strict=True)
    return tm


def per_sequence_bi(tm, comp, x, lens, rev):
    outs, t0 = [], 0
    for n, nr in zip(lens, rev):
        if n:
            mask = (torch.arange(n) < nr).to(torch.int).view(1, n)
            xs = x[:, t0:t0 + n]
            outs.append(tm.forward_bi_b(xs, mask) if comp == "b" else tm.forward_bi_c(xs, callers.reverse_x_idx(mask, n)))
        t0 += n
    return torch.cat(outs, 1)


@pytest.mark.parametrize("vec", sorted(REV))
@pytest.mark.parametrize("comp", ["b", "c"])
def test_compositions_packed_equal_per_sequence(hooks, comp, vec):  # noqa: F811
    tm = time_mix(hooks)
    lens, cu, x = packed_input(cw.N_EMBD, 15)
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(16))
    rev = REV[vec]
    want = per_sequence_bi(tm, comp, x, lens, rev)
    gwant = grads_of(tm, want, gy)
    kw = dict(cu_seqlens=cu, max_seqlen=max(lens), rev_n=i32(rev))
    got = tm.forward_bi_b(x, **kw) if comp == "b" else tm.forward_bi_c(x, None, **kw)
    ggot = grads_of(tm, got, gy)
    assert got.shape == x.shape
    assert max_norm_err(got.detach(), want.detach()) <= F32_TOL
    assert set(ggot) == set(gwant) and len(ggot) >= 17
    for n in gwant:
        assert max_norm_err(ggot[n], gwant[n]) <= F32_TOL, n
    if vec == "len":                                                            # the defaults: every sequence's full length, max_seqlen = total_T
        with torch.no_grad():
            dflt = tm.forward_bi_b(x, cu_seqlens=cu) if comp == "b" else tm.forward_bi_c(x, None, cu_seqlens=cu)
        assert max_norm_err(dflt, want.detach()) <= F32_TOL


def encoder(hooks):
    wkv, wkv_varlen = hooks
    enc = callers.RwkvEncoder(cw.VOCAB, cw.N_EMBD, cw.N_LAYER, cw.DIM_ATT, cw.DIM_FFN, wkv=wkv, wkv_varlen=wkv_varlen)
    enc.load_state_dict(cw.encoder_weights(), strict=True)
    return enc


def test_encoder_packed_equals_padded(hooks):  # noqa: F811
    enc = encoder(hooks)
    g = torch.Generator().manual_seed(17)
    lens = [5, 1, 12, 2, 9]                                                     # ordinary tokens + the emb_id marker
    rows = [torch.cat([torch.randint(2, cw.VOCAB, (n - 1,), generator=g), torch.tensor([enc.emb_id])]) for n in lens]
    T = max(lens)
    padded = torch.stack([torch.cat([r, torch.full((T - len(r),), enc.pad_id)]) for r in rows])
    packed = torch.cat(rows).view(1, -1)
    cu = torch.from_numpy(cu_of(lens))
    with torch.no_grad():
        want_logits, want_hidden = enc(padded, True)
        got_logits, got_hidden = enc(packed, True, cu_seqlens=cu, max_seqlen=T)
        t0 = 0
        for b, n in enumerate(lens):
            assert max_norm_err(got_hidden[0, t0:t0 + n], want_hidden[b, :n]) <= F32_TOL, b
            assert max_norm_err(got_logits[0, t0:t0 + n], want_logits[b, :n]) <= F32_TOL, b
            t0 += n
        want = enc.encode_sentence(padded)
        got = enc.encode_sentence(packed, cu_seqlens=cu)
        assert got.shape == want.shape == (len(lens), cw.N_EMBD)
        assert max_norm_err(got, want) <= F32_TOL


def test_default_none_changes_nothing(hooks):  # noqa: F811
    tm, enc = time_mix(hooks), encoder(hooks)
    x = torch.randn(2, 24, cw.N_EMBD, generator=torch.Generator().manual_seed(9))
    mask = (torch.arange(24).view(1, 24) < torch.tensor([[24], [9]])).to(torch.int)
    rev_idx = callers.reverse_x_idx(mask, 24)
    idx = torch.randint(2, cw.VOCAB, (2, 10), generator=torch.Generator().manual_seed(10))
    idx[0, 7], idx[1, 4], idx[1, 5:] = enc.emb_id, enc.emb_id, enc.pad_id
    with torch.no_grad():
        assert torch.equal(tm.forward_bi_b(x, mask), tm.forward_bi_b(x, mask, cu_seqlens=None, max_seqlen=None, rev_n=None))
        assert torch.equal(tm.forward_bi_c(x, rev_idx), tm.forward_bi_c(x, rev_idx, None, cu_seqlens=None, max_seqlen=None, rev_n=None))
        blk = enc.blocks[0]
        h = enc.emb(idx)
        m = callers.create_mask(idx, enc.emb_id, enc.pad_id)
        assert torch.equal(blk(h, callers.reverse_x_idx(m, 10), m), blk(h, callers.reverse_x_idx(m, 10), m, None, None, None))
        assert torch.equal(enc(idx), enc(idx, False, cu_seqlens=None, max_seqlen=None))
        assert torch.equal(enc.encode_sentence(idx), enc.encode_sentence(idx, cu_seqlens=None))
