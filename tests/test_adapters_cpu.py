"""CPU tier of rwkv_lm_ext_amd.adapters: MultiLoraLinear's eager path against train_dp.LoraLinear and against a per-sequence loop, the rows
that stay with the base model, zero-padding of a lower rank, inject_adapters / load_adapter / set_adapters on a two-block model, and the
error bound of the GPU tests (tests/lora_common.py: restate) met by the eager bf16 path on the GPU tests' own inputs."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import lora_common as lc

i32 = lambda v: torch.tensor([int(t) for t in v], dtype=torch.int32)


def layer(K, N, n_adapters, R, ranks, seed, dtype=torch.float32):
    """A MultiLoraLinear with random base weight and adapter a of rank ranks[a] (alpha = 32), and the list of (A, B, alpha / r)."""
    from rwkv_lm_ext_amd import adapters
    g = torch.Generator().manual_seed(seed)
    lin = nn.Linear(K, N, bias=False)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(N, K, generator=g) / K ** 0.5)
    m = adapters.MultiLoraLinear.from_linear(lin.to(dtype), n_adapters, R)
    weights = []
    for a, r in enumerate(ranks):
        A, B = (torch.randn(r, K, generator=g) / K ** 0.5).to(dtype), (torch.randn(N, r, generator=g) / r ** 0.5).to(dtype)
        m.set_weights(a, A, B, 32.0)
        weights.append((A, B, 32.0 / r))
    return m, weights


def test_uniform_adapter_equals_the_training_module():
    """Every sequence on adapter a: the layer is a train_dp.LoraLinear holding a's weights, up to the fp32 reassociation of a rank-R sum."""
    from rwkv_lm_ext_amd import train_dp
    K, N, R, n = 96, 80, 8, 3
    m, weights = layer(K, N, n, R, [R] * n, seed=1)
    lens = [5, 1, 0, 11]
    cu, T = i32(lc.cu_of(lens, 0)), sum(lens)
    x = torch.randn(1, T, K, generator=torch.Generator().manual_seed(2))
    for a, (A, B, s) in enumerate(weights):
        ref = train_dp.LoraLinear(K, N, r=R, alpha=s * R)
        with torch.no_grad():
            ref.weight.copy_(m.weight)
            ref.lora_A.copy_(A)
            ref.lora_B.copy_(B)
        m.bind(cu, i32([a] * len(lens)))
        with torch.no_grad():
            got, want = m(x), ref(x)
            xa = F.linear(x, A)
            slack = 2 * R * 2.0 ** -23 * (F.linear(x, m.weight).abs() + s * F.linear(xa.abs(), B.abs()))
        assert got.shape == want.shape == (1, T, N)
        assert bool(((got - want).abs() <= slack).all()), a
    assert m.scaling.dtype == torch.float32 and torch.equal(m.scaling, torch.full((n,), 4.0))


def test_rows_of_no_adapter_and_an_unbound_layer_are_the_base_linear():
    K, N, R, n = 64, 48, 8, 3
    m, _ = layer(K, N, n, R, [R] * n, seed=3)
    lens = [4, 2, 7]
    cu, T = i32(lc.cu_of(lens, 0)), sum(lens)
    x = torch.randn(1, T, K, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        base = F.linear(x, m.weight)
        assert torch.equal(m(x), base)                                  # never bound
        for ad in ([-1, -1, -1], [n, n, n], [-1, n, lc.INT_MIN], [n + 7, -2, -1]):
            m.bind(cu, i32(ad))
            assert torch.equal(m(x), base), ad
        m.bind(cu, i32([1, -1, n]))                                     # sequence 0 alone is adapted
        y = m(x)
        assert torch.equal(y[0, 4:], base[0, 4:]) and not torch.equal(y[0, :4], base[0, :4])
        m.bind(cu + 2, i32([-1, 0, -1]))                                # rows in front of cu[0], and a last entry past total_T
        y = m(x)
        assert torch.equal(y[0, :6], base[0, :6]) and torch.equal(y[0, 8:], base[0, 8:]) and not torch.equal(y[0, 6:8], base[0, 6:8])
        m.bind(None, None)
        assert torch.equal(m(x), base)


def test_mixed_batch_equals_the_per_sequence_loop():
    K, N, R = 64, 128, 16
    m, weights = layer(K, N, lc.N_ADAPTERS, R, [16, 8, 16, 4, 16], seed=5)
    for T in lc.TOTALS:
        cu = lc.cu_of()
        x = torch.randn(T, K, generator=torch.Generator().manual_seed(6))
        m.bind(i32(cu), i32(lc.ADAPTERS))
        with torch.no_grad():
            got = m(x)
            want = F.linear(x, m.weight)
            for s, a in enumerate(lc.ADAPTERS):
                lo, hi = min(cu[s], T), min(cu[s + 1], T)
                if 0 <= a < lc.N_ADAPTERS and hi > lo:
                    A, B, sc = weights[a]
                    want[lo:hi] += sc * F.linear(F.linear(x[lo:hi], A), B)
        which = torch.from_numpy(lc.rows_of(cu, lc.ADAPTERS, T))
        assert torch.equal(got[which < 0], F.linear(x, m.weight)[which < 0])
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
        assert not torch.allclose(got[which >= 0], F.linear(x, m.weight)[which >= 0], atol=1e-2)


def test_zero_padding_a_lower_rank_changes_nothing():
    from rwkv_lm_ext_amd import adapters
    K, N, n = 64, 64, 2
    small, weights = layer(K, N, n, 8, [8, 8], seed=7)
    wide = adapters.MultiLoraLinear.from_linear(nn.Linear(K, N, bias=False), n, 16)
    with torch.no_grad():
        wide.weight.copy_(small.weight)
    for a, (A, B, s) in enumerate(weights):
        wide.set_weights(a, A, B, s * 8)
        assert torch.equal(wide.lora_A[a, :8], A) and not wide.lora_A[a, 8:].any()
        assert torch.equal(wide.lora_B[a, :, :8], B) and not wide.lora_B[a, :, 8:].any()
    assert torch.equal(wide.scaling, small.scaling)                       # alpha / r of the adapter's own rank, not of the pool's
    lens = [3, 9, 1]
    cu, ad = i32(lc.cu_of(lens, 0)), i32([1, 0, 1])
    x = torch.randn(1, sum(lens), K, generator=torch.Generator().manual_seed(8))
    small.bind(cu, ad)
    wide.bind(cu, ad)
    with torch.no_grad():
        assert torch.equal(small(x), wide(x))
    with pytest.raises(ValueError):
        small.set_weights(0, torch.zeros(16, K), torch.zeros(N, 16), 32.0)     # a higher rank does not fit
    with pytest.raises(IndexError):
        small.set_weights(n, torch.zeros(8, K), torch.zeros(N, 8), 32.0)


def test_inject_load_and_bind_on_a_two_block_model():
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import adapters, train_dp
    g = torch.Generator().manual_seed(9)
    model = nn.Module()
    model.blocks = nn.ModuleList([train_dp.Block(cw.N_EMBD, cw.DIM_ATT, cw.DIM_FFN, i) for i in range(2)])
    names = adapters.inject_adapters(model, n_adapters=3, r=8)
    want = [f"blocks.{i}.{t}" for i in range(2) for t in adapters.DEFAULT_TARGETS]
    assert sorted(names) == sorted(want)
    layers = dict(adapters.adapter_layers(model))
    assert sorted(layers) == sorted(want)
    assert isinstance(model.blocks[0].att.output, nn.Linear) and isinstance(model.blocks[1].att.gate, nn.Linear)     # not targets
    assert not any(p.requires_grad for p in model.parameters())
    assert all(not m.lora_A.any() and not m.lora_B.any() and not m.scaling.any() for m in layers.values())
    # a plain list of blocks (what step_packed takes) and a narrower target list
    blocks = [train_dp.Block(cw.N_EMBD, cw.DIM_ATT, cw.DIM_FFN, i) for i in range(2)]
    assert sorted(adapters.inject_adapters(blocks, 2, 16, targets=("ffn.key",))) == ["0.ffn.key", "1.ffn.key"]
    assert isinstance(blocks[1].ffn.key, adapters.MultiLoraLinear) and blocks[1].ffn.key.r == 16

    def weights(r):
        return {k: (torch.randn(r, m.in_features, generator=g), torch.randn(m.out_features, r, generator=g)) for k, m in layers.items()}

    # the reference's two key styles: '{key}.lora_A', and '[{parent}.]{key}.lora_A.{peft_name}.weight'
    w0, w1, w2 = weights(8), weights(4), weights(8)
    sd0 = {f"{k}.lora_{n}": t for k, (a, b) in w0.items() for n, t in (("A", a), ("B", b))}
    sd1 = {f"{k}.lora_{n}.sft.weight": t for k, (a, b) in w1.items() for n, t in (("A", a), ("B", b))}
    sd2 = {f"rwkvModel.{k}.lora_{n}.bi.weight": t for k, (a, b) in w2.items() for n, t in (("A", a), ("B", b))}
    del sd2["rwkvModel.blocks.1.ffn.value.lora_B.bi.weight"]                      # a layer without both keys keeps what it has
    assert sorted(adapters.load_adapter(model, 0, sd0, alpha=32.0)) == sorted(want)
    assert sorted(adapters.load_adapter(model, 1, sd1, alpha=16.0, peft_name="sft")) == sorted(want)
    assert adapters.load_adapter(model, 2, sd1, alpha=16.0, peft_name="bi") == []
    assert adapters.load_adapter(model, 2, sd2, alpha=32.0, peft_name="bi") == []   # the parent's name is part of the key
    got = adapters.load_adapter(model, 2, sd2, alpha=32.0, peft_name="bi", parent_model_name="rwkvModel")
    assert sorted(got) == sorted(set(want) - {"blocks.1.ffn.value"})
    for k, m in layers.items():
        assert torch.equal(m.lora_A[0], w0[k][0]) and torch.equal(m.lora_B[0], w0[k][1])
        assert torch.equal(m.lora_A[1, :4], w1[k][0]) and not m.lora_A[1, 4:].any() and torch.equal(m.lora_B[1, :, :4], w1[k][1])
        if k == "blocks.1.ffn.value":
            assert not m.lora_A[2].any() and torch.equal(m.scaling, torch.tensor([4.0, 4.0, 0.0]))
        else:
            assert torch.equal(m.lora_A[2], w2[k][0]) and torch.equal(m.scaling, torch.tensor([4.0, 4.0, 4.0]))
    # binding is by reference, on every layer; unbinding makes the blocks the base model again
    cu, ad = i32([0, 3, 8]), i32([1, -1])
    adapters.set_adapters(model, cu, ad)
    assert all(m._cu is cu and m._adapter is ad for m in layers.values())
    x = torch.randn(1, 8, cw.N_EMBD, generator=g)
    key = model.blocks[0].ffn.key
    with torch.no_grad():
        base = F.linear(x, key.weight)
        y = key(x)
        assert torch.equal(y[0, 3:], base[0, 3:]) and not torch.equal(y[0, :3], base[0, :3])
        ad.fill_(-1)                                                              # refilled in place: re-routed without a new binding
        assert torch.equal(key(x), base)
    adapters.set_adapters(model, None, None)
    assert all(m._cu is None and m._adapter is None for m in layers.values())
    # .to(bf16) keeps alpha / r in fp32
    model.to(torch.bfloat16)
    assert key.weight.dtype == key.lora_A.dtype == torch.bfloat16 and key.scaling.dtype == torch.float32
    # kernels=True where the kernels do not apply
    key.kernels = True
    key.bind(cu, ad)
    with torch.no_grad(), pytest.raises(RuntimeError, match="kernels=True: x, weight and the pools must be bf16 on the GPU"):
        key(x.to(torch.bfloat16))
    key.kernels = False
    with torch.no_grad():
        assert key(x.to(torch.bfloat16)).dtype == torch.bfloat16


def test_the_eager_path_has_autograd():
    m, _ = layer(64, 64, 2, 8, [8, 8], seed=11)
    m.lora_A.requires_grad_(True)
    m.lora_B.requires_grad_(True)
    m.bind(i32([0, 2, 5]), i32([1, 0]))
    x = torch.randn(5, 64, generator=torch.Generator().manual_seed(12), requires_grad=True)
    m(x).square().sum().backward()
    assert x.grad is not None and m.lora_A.grad.abs().sum() > 0 and m.lora_B.grad.abs().sum() > 0 and m.weight.grad is None


@pytest.mark.parametrize("total_T", lc.TOTALS)
@pytest.mark.parametrize("K,N,R", lc.SHAPES + lc.MIXED_SHAPES)
def test_eager_bf16_meets_the_error_bound_of_the_gpu_tests(K, N, R, total_T):
    """lora_packed_eager in bf16 on the CPU, on the inputs of tests/test_lora_packed_gpu.py, against the fp64 restatement:
    |out - E| <= 2^-8 |E| + 2 |scale| sum_j |B_nj| (2^-9 |e_j| + K 2^-23 S_j) for every element, rows of no adapter exact."""
    from rwkv_lm_ext_amd import adapters
    x, y0, A, B, scale = lc.case(K, N, R, total_T)
    E, bound = lc.reference(K, N, R, total_T)
    with torch.no_grad():
        out = adapters.lora_packed_eager(x, y0, A, B, scale, i32(lc.ADAPTERS), i32(lc.cu_of()))
    assert out.dtype == lc.bf and out.shape == y0.shape
    ratio = lc.worst_ratio(out, E, bound)
    print(f"K={K} N={N} R={R} total_T={total_T}: max |out - E| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    which = torch.from_numpy(lc.rows_of(lc.cu_of(), lc.ADAPTERS, total_T))
    assert torch.equal(out[which < 0].view(torch.int16), y0[which < 0].view(torch.int16))
    assert (which >= 0).sum() > 100 and float((out.float() - y0.float()).abs()[which >= 0].mean()) > 0.3      # the term is as large as y0
