"""Per-sequence LoRA adapters on the GPU: wkv6_lora_packed_bf16 (include/wkv6_amd.h) through mix_op.lora_packed, adapters.MultiLoraLinear
and infctx.step_packed under adapters.inject_adapters / set_adapters.

(a) a mixed batch equals one call per sequence, bit for bit; (b) rows of no adapter and of no sequence keep their bits, whatever they
are; (c) every element lies within the bound of tests/lora_common.py (restate) of the fp64 restatement; (d) a NaN adapter reaches exactly
the rows that name it; (e) 300 sequences against the eager path; (f) step_packed on a mixed batch equals step_packed on every sequence
alone, and all sequences on -1 equal the blocks before injection; (g) a captured step replays after everything was refilled in place.

The batch of (a)-(d): lengths LENS behind LEAD rows of no sequence, adapters ADAPTERS (-1, n_adapters and INT_MIN among them, sequence 3
empty), total_T in TOTALS.  (d) says that nobody names adapter 1 and that adapter 3 has rows, which ADAPTERS does not give (sequence 6
names 1, and only the empty sequence names 3): it runs ADAPTERS with sequences 1 and 6 moved to adapter 3.

(a)-(d) run lora_common.SHAPES and MIXED_SHAPES.  (K, N, R), MIXED_SHAPES -- the shrink walks K / 32 steps in 4 interleaved chunks, 4 steps
a pass (main loop), then singly (remainder), and no shape of SHAPES runs both loops in one call: (768, 2688, 8): main once, two remainder
steps a chunk, three quarters of the contraction padded, 42 column blocks over the expand's 16 workgroups (3, 3, .., 2, 2); (2688, 768,
16): main five times, one remainder step a chunk, half padded; (576, 1088, 64): main once, a remainder step for chunks 0 and 1 only, two
expand steps, 17 blocks (workgroup 0 walks one more than the rest); (1088, 64, 32): main twice, a remainder step for two chunks.
(h) sixteen groups in a tile: GROUPS_LENS / GROUPS_ADAPTERS over 20 adapters at (192, 192, 16) and (768, 64, 8) -- rows 16..31 are sixteen
one-token sequences on sixteen adapters (16..19 among them), rows 32..47 nine groups with a two-row sequence and a row on no adapter
between them -- (a) and (c).  (i) many tiles: 4100 rows of (64, 64, 8) under many_batch(), 60 sequences over the 20 adapters with -1,
20 and INT_MIN among them: (a), (c) and (b)."""
import pytest
import torch

import lora_common as lc
from lora_common import bf
from test_rwkv6_varlen_gpu import bits, same

pytestmark = pytest.mark.gpu


def i32(x):
    return torch.tensor([int(v) for v in x], dtype=torch.int32, device="cuda")


def on_gpu(K, N, R, total_T, n_adapters=lc.N_ADAPTERS):
    return tuple(t.cuda() for t in lc.case(K, N, R, total_T, n_adapters=n_adapters))


def run(x, y0, A, B, scale, adapters, cu):
    from rwkv_lm_ext_amd import mix_op
    y = y0.clone()
    with torch.no_grad():
        out = mix_op.lora_packed(x, y, A, B, scale, i32(adapters), i32(cu))
    torch.cuda.synchronize()
    assert out is y
    return y


@pytest.mark.parametrize("total_T", lc.TOTALS)
@pytest.mark.parametrize("K,N,R", lc.SHAPES + lc.MIXED_SHAPES)
def test_mixed_batch_equals_one_call_per_sequence_bitwise(K, N, R, total_T):
    x, y0, A, B, scale = on_gpu(K, N, R, total_T)
    cu = lc.cu_of()
    mixed = run(x, y0, A, B, scale, lc.ADAPTERS, cu)
    which = torch.from_numpy(lc.rows_of(cu, lc.ADAPTERS, total_T)).cuda()
    assert same(mixed[which < 0], y0[which < 0]) and not bool((bits(mixed[which >= 0]) == bits(y0[which >= 0])).all(1).any())
    joined = y0.clone()
    for s, a in enumerate(lc.ADAPTERS):
        alone = run(x, y0, A, B, scale, [a], cu[s:s + 2])
        lo, hi = min(cu[s], total_T), min(cu[s + 1], total_T)
        assert same(alone[:lo], y0[:lo]) and same(alone[hi:], y0[hi:]), s         # a call touches its own rows only
        joined[lo:hi] = alone[lo:hi]
    assert same(mixed, joined)


@pytest.mark.parametrize("total_T", lc.TOTALS)
@pytest.mark.parametrize("K,N,R", lc.SHAPES + lc.MIXED_SHAPES)
def test_rows_of_no_adapter_and_of_no_sequence_keep_their_bits(K, N, R, total_T):
    x, _, A, B, scale = on_gpu(K, N, R, total_T)
    g = torch.Generator().manual_seed(5)
    y0 = torch.randint(-32768, 32768, (total_T, N), generator=g, dtype=torch.int32).to(torch.int16).cuda().view(bf)      # NaN payloads included
    assert bool(y0.isnan().any())
    cu = lc.cu_of()
    out = run(x, y0, A, B, scale, lc.ADAPTERS, cu)
    which = torch.from_numpy(lc.rows_of(cu, lc.ADAPTERS, total_T)).cuda()
    assert int((which < 0).sum()) >= lc.LEAD + 18 and same(out[which < 0], y0[which < 0])
    assert not same(out[which >= 0], y0[which >= 0])
    # garbage in both int arrays: memory-safe, and with no valid adapter nothing changes
    wild = [1 << 30, -5, lc.INT_MIN, (1 << 31) - 1, 7, 0, -1, 99, 3, 2, 1]
    assert same(run(x, y0, A, B, scale, [lc.N_ADAPTERS, -1, lc.INT_MIN, (1 << 31) - 1, 1 << 20, -7, 5, 6, 7, 8], wild), y0)
    run(x, y0, A, B, scale, lc.ADAPTERS, wild)


@pytest.mark.parametrize("total_T", lc.TOTALS)
@pytest.mark.parametrize("K,N,R", lc.SHAPES + lc.MIXED_SHAPES)
def test_error_against_the_fp64_restatement(K, N, R, total_T):
    """|out - E| <= 2^-8 |E| + 2 |scale| sum_j |B_nj| (2^-9 |e_j| + K 2^-23 S_j) for every element."""
    out = run(*on_gpu(K, N, R, total_T), lc.ADAPTERS, lc.cu_of())
    E, bound = lc.reference(K, N, R, total_T)
    ratio = lc.worst_ratio(out.cpu(), E, bound)
    print(f"K={K} N={N} R={R} total_T={total_T}: max |out - E| / bound = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("K,N,R", lc.SHAPES + lc.MIXED_SHAPES)
def test_a_nan_adapter_reaches_exactly_the_rows_that_name_it(K, N, R):
    total_T = lc.TOTALS[0]
    x, y0, A, B, scale = on_gpu(K, N, R, total_T)
    adapters = list(lc.ADAPTERS)
    adapters[1] = adapters[6] = 3             # rows 40 and 59: single tokens inside tiles that hold adapters 2, 4 and rows of none
    assert 1 not in adapters
    cu = lc.cu_of()
    clean = run(x, y0, A, B, scale, adapters, cu)
    An, Bn = A.clone(), B.clone()
    for a in (1, 3):
        An[a] = float("nan")
        Bn[a] = float("nan")
    out = run(x, y0, An, Bn, scale, adapters, cu)
    which = torch.from_numpy(lc.rows_of(cu, adapters, total_T)).cuda()
    assert int((which == 3).sum()) == 2 and not bool(clean.isnan().any())
    assert bool(out[which == 3].isnan().all())
    assert same(out[which != 3], clean[which != 3])
    # NaN in one matrix only
    for An_, Bn_ in ((An, B), (A, Bn)):
        out = run(x, y0, An_, Bn_, scale, adapters, cu)
        assert bool(out[which == 3].isnan().all()) and same(out[which != 3], clean[which != 3])


def equals_one_call_per_sequence_and_meets_the_bound(K, N, R, total_T, cu, adapters, what):
    """(a) and (c) on a batch of its own over lc.MANY_ADAPTERS adapters; returns (which, the inputs on the GPU)."""
    n = lc.MANY_ADAPTERS
    x, y0, A, B, scale = on_gpu(K, N, R, total_T, n)
    mixed = run(x, y0, A, B, scale, adapters, cu)
    joined = y0.clone()
    for s, a in enumerate(adapters):
        lo, hi = min(cu[s], total_T), min(cu[s + 1], total_T)
        if hi > lo:
            joined[lo:hi] = run(x, y0, A, B, scale, [a], cu[s:s + 2])[lo:hi]
    assert same(mixed, joined)
    which = lc.rows_of(cu, adapters, total_T, n)
    E, bound = lc.restate(*lc.case(K, N, R, total_T, n_adapters=n), which)
    ratio = lc.worst_ratio(mixed.cpu(), E, bound)
    print(f"{what} K={K} N={N} R={R} total_T={total_T}: max |out - E| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    w = torch.from_numpy(which).cuda()
    assert same(mixed[w < 0], y0[w < 0]) and not bool((bits(mixed[w >= 0]) == bits(y0[w >= 0])).all(1).any())
    return which, (x, y0, A, B, scale)


@pytest.mark.parametrize("K,N,R", lc.GROUPS_SHAPES)
def test_sixteen_groups_in_a_tile(K, N, R):
    """A tile of sixteen one-token sequences on sixteen adapters of a pool of 20 (for_each_group's longest walk: the shrink deals 16 x 4
    items round its 8 waves, an expand wave serves groups w, w + 4, w + 8, w + 12) beside a tile of nine groups: (a) and (c)."""
    cu, total_T = lc.cu_of(lc.GROUPS_LENS, 0), lc.GROUPS_TOTAL
    which = lc.rows_of(cu, lc.GROUPS_ADAPTERS, total_T, lc.MANY_ADAPTERS)
    assert len(set(which[16:32].tolist())) == 16 and which[16:32].min() >= 0 and which[16:32].max() > 15      # sixteen groups, adapters above 15
    third = which[32:48].tolist()
    assert len(set(third) - {-1}) == 9 and third[4] == -1 and third[2] == third[3] and third[10:] == [third[10]] * 6
    assert which[15] != which[16] and (which[42:72] == which[42]).all() and (which[72:] == -1).all() and len(which) == total_T
    got, _ = equals_one_call_per_sequence_and_meets_the_bound(K, N, R, total_T, cu, lc.GROUPS_ADAPTERS, "sixteen groups")
    assert (got == which).all()


def test_many_tiles():
    """4100 rows, 257 tiles: row * K, row * N and row * R from rows in the thousands, about 60 sequences over 20 adapters with boundaries
    inside tiles all the way: (a), (c), and (b) with random bit patterns in y."""
    (K, N, R), total_T = lc.MANY_SHAPE, lc.MANY_TOTAL
    cu, adapters = (list(v) for v in lc.many_batch())
    assert total_T >= 4096 and len(adapters) >= 55 and -1 in adapters and lc.MANY_ADAPTERS in adapters and lc.INT_MIN in adapters
    assert len({a for a in adapters if 0 <= a < lc.MANY_ADAPTERS}) >= 18 and any(b == a for a, b in zip(cu, cu[1:]))
    assert sum(1 for v in cu if v % 16) >= 50 and min(cu) == lc.LEAD and cu[1] < 512 and total_T - 512 < max(cu) < total_T
    which, (x, _, A, B, scale) = equals_one_call_per_sequence_and_meets_the_bound(K, N, R, total_T, cu, adapters, "many tiles")
    assert int((which < 0).sum()) >= 100 and int((which >= 0).sum()) >= 3000
    g = torch.Generator().manual_seed(6)
    y0 = torch.randint(-32768, 32768, (total_T, N), generator=g, dtype=torch.int32).to(torch.int16).cuda().view(bf)      # NaN payloads included
    out = run(x, y0, A, B, scale, adapters, cu)
    w = torch.from_numpy(which).cuda()
    assert bool(y0.isnan().any()) and same(out[w < 0], y0[w < 0]) and not same(out[w >= 0], y0[w >= 0])


def test_three_hundred_sequences_against_the_eager_path():
    """300 sequences, 297 of one token, over 5 adapters (and a few on none): MultiLoraLinear with the kernels against its eager path over
    the same base GEMM, |kernels - eager| within the bound of (c) around the fp64 restatement of that y0."""
    from rwkv_lm_ext_amd import adapters
    K, N, R, n = 192, 192, 16, 5
    g = torch.Generator().manual_seed(17)
    lens = [1] * 300
    lens[7], lens[150], lens[299] = 33, 18, 5
    ad = torch.randint(-1, n, (300,), generator=g).tolist()
    cu, T = lc.cu_of(lens, 0), sum(lens)
    m = adapters.MultiLoraLinear(K, N, n, R)
    A, B = torch.randn(n, R, K, generator=g) / K ** 0.5, torch.randn(n, N, R, generator=g) / R ** 0.5
    with torch.no_grad():
        m.weight.copy_(torch.randn(N, K, generator=g) / K ** 0.5)
        for a in range(n):
            m.set_weights(a, A[a], B[a], R * (0.5 + 3.5 * float(torch.rand(1, generator=g))))
    m = m.cuda().to(bf)
    assert m.scaling.dtype == torch.float32
    x = torch.randn(1, T, K, generator=g).to(bf).cuda()
    m.bind(i32(cu), i32(ad))
    with torch.no_grad():
        m.kernels = True
        got = m(x)
        m.kernels = False
        want = m(x)
        m.bind(None, None)
        y0 = m(x)
    torch.cuda.synchronize()
    which = lc.rows_of(cu, ad, T, n)
    E, bound = lc.restate(x[0].cpu(), y0[0].cpu(), m.lora_A.cpu(), m.lora_B.cpu(), m.scaling.cpu(), which)
    err = (got[0].cpu().double() - want[0].cpu().double()).abs()
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
    print(f"300 sequences: max |kernels - eager| / bound = {ratio:.3f}; kernels against E: {lc.worst_ratio(got[0].cpu(), E, bound):.3f}, "
          f"eager against E: {lc.worst_ratio(want[0].cpu(), E, bound):.3f}")
    assert ratio <= 1.0
    w = torch.from_numpy(which).cuda()
    assert same(got[0][w < 0], y0[0][w < 0]) and int((w >= 0).sum()) > 250 and not same(got[0][w >= 0], y0[0][w >= 0])


# ---- the serving step
def adapted_blocks(n_adapters=3, r=8, seed=23):
    """two_blocks() of test_packed_shift_gpu.py (C = 128, dim_ffn = 256) before and after inject_adapters, every adapter with B != 0."""
    from rwkv_lm_ext_amd import adapters
    from test_packed_shift_gpu import two_blocks
    plain, blocks = two_blocks(), two_blocks()
    names = adapters.inject_adapters(blocks, n_adapters, r)
    assert len(names) == 12
    g = torch.Generator().manual_seed(seed)
    for _, m in adapters.adapter_layers(blocks):
        assert m.weight.dtype == bf and m.weight.is_cuda and m.scaling.dtype == torch.float32
        m.kernels = True
        for a in range(n_adapters):
            m.set_weights(a, torch.randn(r, m.in_features, generator=g) / m.in_features ** 0.5, torch.randn(m.out_features, r, generator=g) / r ** 0.5,
                          alpha=8.0 * (a + 1))
    return plain, blocks


def test_step_packed_mixed_batch_against_one_sequence_at_a_time():
    """step_packed under bound adapters with out_slots and snap, kernels on, against step_packed on every sequence alone over the same x
    (n_seq = 1, so that the GEMMs see the same shapes): outputs and all three pools, bit for bit; all sequences on -1 against the blocks
    before injection."""
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import adapters, infctx
    from test_packed_shift_gpu import cum
    plain, blocks = adapted_blocks()
    E, heads, n_slots = cw.N_EMBD, cw.DIM_ATT // 64, 16
    lens, src, out, ad = [130, 64, 0, 70, 5, 1], [4, 1, 6, 0, -1, 5], [8, 9, 10, 11, 12, 5], [1, 0, 2, -1, 2, 1]
    snap_slots, cu_snap = [13, 14, 15, 2, 3], [0, 2, 3, 3, 5, 5, 5]
    g = torch.Generator().manual_seed(71)
    x = torch.randn(1, sum(lens), E, generator=g).cuda().to(bf)
    pools = infctx.PackedPools.create(2, n_slots, E, heads, "cuda", bf)
    pools.shift_att.copy_(torch.randn(2, n_slots, E, generator=g))
    pools.shift_ffn.copy_(torch.randn(2, n_slots, E, generator=g))
    pools.wkv.copy_(torch.randn(2, n_slots, heads, 64, 64, generator=g) * 0.3)
    fields = ("shift_att", "shift_ffn", "wkv")
    clone = lambda p: infctx.PackedPools(*(getattr(p, f).clone() for f in fields))
    before = clone(pools)
    c = cum(lens)
    snap = (64, i32(cu_snap), i32(snap_slots))
    with torch.no_grad():
        adapters.set_adapters(blocks, i32(c), i32(ad))
        y = infctx.step_packed(blocks, x, i32(c), max(lens), pools, i32(src), out_slots=i32(out), snap=snap, pool_kernels=True)
        # all on -1 (and unbound): the blocks before injection
        for binding in ((i32(c), i32([-1] * len(lens))), (None, None)):
            adapters.set_adapters(blocks, *binding)
            base, want = clone(before), clone(before)
            yb = infctx.step_packed(blocks, x, i32(c), max(lens), base, i32(src), out_slots=i32(out), snap=snap, pool_kernels=True)
            yp = infctx.step_packed(plain, x, i32(c), max(lens), want, i32(src), out_slots=i32(out), snap=snap, pool_kernels=True)
            torch.cuda.synchronize()
            assert same(yb, yp) and all(same(getattr(base, f), getattr(want, f)) for f in fields)
        assert not same(y[0, :130], yp[0, :130]) and same(y[0, c[3]:c[4]], yp[0, c[3]:c[4]])       # adapters matter; sequence 3 is on none
        for s, n in enumerate(lens):
            if n == 0:
                continue
            for j in list(range(min(n // 64, cu_snap[s + 1] - cu_snap[s]))) + [None]:
                upto, where = (n, out[s]) if j is None else (64 * (j + 1), snap_slots[cu_snap[s] + j])
                alone = clone(before)
                home = src[s] if src[s] >= 0 else 7                      # "no state": a zeroed slot of the copies
                if src[s] < 0:
                    for f in fields:
                        getattr(alone, f)[:, home] = 0
                adapters.set_adapters(blocks, i32([c[s], c[s] + upto]), i32([ad[s]]))
                ya = infctx.step_packed(blocks, x, i32([c[s], c[s] + upto]), upto, alone, i32([home]), pool_kernels=True)
                torch.cuda.synchronize()
                for f in fields:
                    assert same(getattr(pools, f)[:, where], getattr(alone, f)[:, home]), (s, j, f)
                if j is None:
                    assert same(y[0, c[s]:c[s + 1]], ya[0, c[s]:c[s + 1]]), s


def test_step_packed_with_adapters_replays_from_a_graph():
    """step_packed with bound adapters captured once on one stream, replayed after x, cu_seqlens, slots, adapter and the pools were refilled
    in place: the replay equals an eager run on the same data."""
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import adapters, infctx
    from test_packed_shift_gpu import cum
    _, blocks = adapted_blocks(seed=29)
    E, heads, n_slots, total, n_seq, bound = cw.N_EMBD, cw.DIM_ATT // 64, 8, 40, 5, 40
    g = torch.Generator().manual_seed(81)
    fields = ("shift_att", "shift_ffn", "wkv")

    def data(lens, slots, ad):
        assert sum(lens) == total and len(lens) == n_seq and max(lens) <= bound
        return (torch.randn(1, total, E, generator=g).to(bf).cuda(), i32(cum(lens)), i32(slots), i32(ad),
                [torch.randn(2, n_slots, E, generator=g).to(bf).cuda(), torch.randn(2, n_slots, E, generator=g).to(bf).cuda(),
                 (torch.randn(2, n_slots, heads, 64, 64, generator=g) * 0.3).cuda()])

    first, second = data([10, 1, 0, 24, 5], [4, 1, 6, 0, -1], [0, 1, 2, -1, 2]), data([1, 20, 9, 0, 10], [7, 2, n_slots, 3, 5], [2, 2, 0, 1, 3])
    x, cu, slots, ad = (t.clone() for t in first[:4])
    pools = infctx.PackedPools(*(t.clone() for t in first[4]))
    adapters.set_adapters(blocks, cu, ad)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        infctx.step_packed(blocks, x, cu, bound, pools, slots, pool_kernels=True)       # warm-up: library, self-test, rocBLAS
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            y = infctx.step_packed(blocks, x, cu, bound, pools, slots, pool_kernels=True)
    torch.cuda.current_stream().wait_stream(side)
    results = []
    for name, d in (("the captured partition", first), ("another partition", second)):
        adapters.set_adapters(blocks, cu, ad)
        for held, new in zip([x, cu, slots, ad] + [getattr(pools, f) for f in fields], list(d[:4]) + d[4]):
            held.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eager = infctx.PackedPools(*(t.clone() for t in d[4]))
        adapters.set_adapters(blocks, d[1], d[3])
        with torch.no_grad():
            want = infctx.step_packed(blocks, d[0], d[1], bound, eager, d[2], pool_kernels=True)
        torch.cuda.synchronize()
        assert same(y, want), name
        assert all(same(getattr(pools, f), getattr(eager, f)) for f in fields), name
        results.append(y.clone())
    assert not same(first[3], second[3]) and not same(results[0], results[1])
