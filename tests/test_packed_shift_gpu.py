"""The token-shift slot pool on the GPU: wkv6_ddlerp_slots_forward / wkv6_shift_keep (include/wkv6_amd.h) through mix_op.ddlerp_slots /
mix_op.shift_keep, infctx.tmix_forward_packed / cmix_forward_packed(pool_kernels=), and the block-level step on top
(infctx.block_forward_packed, step_packed, last_token_rows, PackedPools).

Every comparison is bitwise: the kernels copy rows and repeat the lerp arithmetic of wkv6_ddlerp_varlen_forward, so there is no tolerance to
choose.  References are calls that existed before these kernels did (mix_op.ddlerp on gathered rows, the eager _keep_* functions,
pool_kernels=False, the same layers on one sequence at a time) and, for shift_keep, a numpy restatement of the header's rules."""
import numpy as np
import pytest
import torch

from test_rwkv6_varlen_gpu import bf, bits, same

pytestmark = pytest.mark.gpu
NAN = float("nan")


def i32(x):
    return torch.tensor([int(v) for v in x], dtype=torch.int32, device="cuda")


def cum(lens):
    return np.concatenate([[0], np.cumsum(lens)]).tolist()


def random_bits(shape, g):
    """bf16 of uniformly random bit patterns: NaNs of every payload, infinities and denormals included."""
    return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16).cuda().view(bf)


# ---- 1. the lerp that reads the pool
LENS1 = [0, 1, 1, 5, 0, 33, 2]
N_SLOTS1 = 9
# sequence 0 (empty) is the only one to name slot 5; 1 and 2 share slot 2 (fan-out); -1 and n_slots lie outside the pool
SLOTS1 = [5, 2, 2, -1, 5, N_SLOTS1, 0]


@pytest.mark.parametrize("C", [64, 256, 4096])
@pytest.mark.parametrize("NS,has_m", [(1, False), (5, True), (2, False)])
def test_ddlerp_slots_equals_the_varlen_lerp_on_gathered_rows(C, NS, has_m):
    from rwkv_lm_ext_amd import mix_op
    g = torch.Generator().manual_seed(100 + C + NS)
    total, n_seq = sum(LENS1), len(LENS1)
    x = torch.randn(1, total, C, generator=g).to(bf).cuda()
    maa = torch.rand(NS, C, generator=g).to(bf).cuda()
    m = (0.1 * torch.randn(NS, 1, total, C, generator=g)).to(bf).cuda() if has_m else None
    cu = i32(cum(LENS1))
    for slots in (SLOTS1, None):
        named = [s if slots is None else slots[s] for s in range(n_seq)]
        live = {p for s, p in enumerate(named) if LENS1[s] > 0 and 0 <= p < N_SLOTS1}
        pool = torch.randn(N_SLOTS1, C, generator=g).to(bf).cuda()
        for p in range(N_SLOTS1):                       # rows nobody reads -- unreferenced ones and those only an empty sequence names
            if p not in live:
                pool[p] = NAN
        gathered = torch.zeros(n_seq, C, dtype=bf, device="cuda")
        for s, p in enumerate(named):
            if p in live:
                gathered[s] = pool[p]
        before = pool.clone()
        with torch.no_grad():
            want = mix_op.ddlerp(x, maa, m, shifted0=gathered, cu_seqlens=cu)
            got = mix_op.ddlerp_slots(x, maa, m, pool, None if slots is None else i32(slots), cu)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(got).all()), slots
        assert same(got, want), slots
        assert same(pool, before), slots
    assert live == {1, 2, 3, 5, 6}                      # slot = sequence index: the rows of the two empty sequences (0, 4) were NaN


# ---- 2. the launch that writes the pool
# (start, end) of the sequences in cu_seqlens terms: empty; 70; 6 (a multiple of 3); 200, which max_seqlen cuts to 130; 64; 1; and one whose
# end lies past total_T (clamped: 40 tokens)
CU2 = [0, 0, 70, 76, 276, 340, 341, 400]
TOTAL2, MAX2, N_SLOTS2 = 381, 130, 400
LEN2 = [0, 70, 6, 130, 64, 1, 40]
DST2 = [3, 7, -1, 11, N_SLOTS2, 5, 9]                   # the empty sequence names slot 3; -1 and n_slots lie outside the pool


def keep_restated(x, pool, cu, total, max_seqlen, slot_out, snap_every, cu_snap, snap_slot):
    """include/wkv6_amd.h, wkv6_shift_keep, on numpy arrays of bits.  Returns the new pool and the set of rows written."""
    out, n_slots, n_seq, written = pool.copy(), pool.shape[0], len(cu) - 1, set()
    n_snap = 0 if snap_slot is None else len(snap_slot)
    clamp = lambda v, lo, hi: min(max(int(v), lo), hi)
    for s in range(n_seq):
        a, b = clamp(cu[s], 0, total), clamp(cu[s + 1], 0, total)
        n = min(max(b - a, 0), max_seqlen)
        dst = s if slot_out is None else int(slot_out[s])
        if n > 0 and 0 <= dst < n_slots:
            out[dst] = x[a + n - 1]
            written.add(dst)
        if snap_every > 0 and n_snap > 0:
            c0, c1 = clamp(cu_snap[s], 0, n_snap), clamp(cu_snap[s + 1], 0, n_snap)
            for j in range(min(n // snap_every, max(c1 - c0, 0))):
                dst = int(snap_slot[c0 + j])
                if 0 <= dst < n_slots:
                    out[dst] = x[a + (j + 1) * snap_every - 1]
                    written.add(dst)
    return out, written


def snapshot_plan(snap_every):
    """Grants per sequence: the empty one is granted 2 (it earns none), sequence 1 one fewer than it earns, sequence 3 two more, the others
    what they earn.  Snapshot slots are distinct, apart from the ones outside the pool sprinkled in."""
    earned = [n // snap_every for n in LEN2]
    grant = list(earned)
    grant[0], grant[1], grant[3] = 2, max(earned[1] - 1, 0), earned[3] + 2
    cu_snap = cum(grant)
    free = [p for p in range(N_SLOTS2) if p not in DST2]
    perm = torch.randperm(len(free), generator=torch.Generator().manual_seed(snap_every)).tolist()
    assert cu_snap[-1] <= len(free)
    snap_slot = [free[perm[e]] for e in range(cu_snap[-1])]
    for e in range(cu_snap[-1]):
        if e % 11 == 3:
            snap_slot[e] = -7
        elif e % 13 == 5:
            snap_slot[e] = N_SLOTS2 + 2
    return earned, grant, cu_snap, snap_slot


@pytest.mark.parametrize("C", [64, 256, 4096])
@pytest.mark.parametrize("snap_every", [1, 3, 64])
def test_shift_keep_against_the_rules_and_the_eager_functions(C, snap_every):
    from rwkv_lm_ext_amd import infctx, mix_op
    g = torch.Generator().manual_seed(7 * C + snap_every)
    x = random_bits((TOTAL2, C), g)
    pool0 = random_bits((N_SLOTS2, C), g)
    earned, grant, cu_snap, snap_slot = snapshot_plan(snap_every)
    assert any(n > 0 and n % snap_every == 0 for n in LEN2)              # a snapshot at position len_s
    assert grant[1] < earned[1]
    assert grant[3] > earned[3] and any(not 0 <= p < N_SLOTS2 for p in snap_slot)
    cu, dst = i32(CU2), i32(DST2)
    xb, pb = bits(x).cpu().numpy(), bits(pool0).cpu().numpy()
    cases = {"snapshots": (dst, (snap_every, i32(cu_snap), i32(snap_slot))),
             "n_snap = 0": (dst, (snap_every, i32([0] * len(CU2)), i32([]))),
             "snap_every = 0, no arrays": (dst, (0, None, None)),
             "no snap": (dst, None)}
    for name, (slot_out, snap) in cases.items():
        pool = pool0.clone()
        mix_op.shift_keep(x, cu, MAX2, pool, slot_out, snap)
        live_snap = snap is not None and snap[0] > 0 and snap[2].numel() > 0
        want, written = keep_restated(xb, pb, CU2, TOTAL2, MAX2, DST2, snap[0] if live_snap else 0, cu_snap if live_snap else None,
                                      snap_slot if live_snap else None)
        eager = pool0.clone()
        infctx._keep_last_tokens(eager, slot_out, x, cu, MAX2)
        if live_snap:
            infctx._keep_snap_tokens(eager, snap, x, cu, MAX2)
        torch.cuda.synchronize()
        got = bits(pool).cpu().numpy()
        assert np.array_equal(got, want), name
        assert same(pool, eager), name
        untouched = [p for p in range(N_SLOTS2) if p not in written]
        assert 3 in untouched and np.array_equal(got[untouched], pb[untouched]), name
        if name == "snapshots":
            assert {7, 11, 5, 9} < written                                # ... and snapshot rows beside the four final tokens
        else:
            assert written == {7, 11, 5, 9}, name
    # slot_out = NULL is the sequence index (row 0, the empty sequence's, keeps its bits)
    pool = pool0.clone()
    mix_op.shift_keep(x, cu, MAX2, pool, None)
    want, written = keep_restated(xb, pb, CU2, TOTAL2, MAX2, None, 0, None, None)
    torch.cuda.synchronize()
    assert written == {1, 2, 3, 4, 5, 6} and np.array_equal(bits(pool).cpu().numpy(), want)


# ---- the layers
def sublayers():
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import callers
    tm = callers.Tmix_x060(cw.N_EMBD, cw.DIM_ATT)
    tm.load_state_dict(cw.tmix_weights(torch.Generator().manual_seed(11), layer_id=1), strict=True)
    cm = callers.CMix_x060(cw.N_EMBD, cw.DIM_FFN)
    cm.load_state_dict(cw.cmix_weights(torch.Generator().manual_seed(12)), strict=True)
    return tm.cuda().to(bf), cm.cuda().to(bf)


def two_blocks():
    """Two train_dp.Block layers (the first with ln0) with the weights of oracle/caller_weights.py."""
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import train_dp
    g = torch.Generator().manual_seed(31)
    blocks = []
    for i in range(2):
        b = train_dp.Block(cw.N_EMBD, cw.DIM_ATT, cw.DIM_FFN, i)
        w = dict(cw.tmix_weights(g, "att.", layer_id=i), **cw.cmix_weights(g, "ffn."))
        for ln in ("ln1", "ln2") + (("ln0",) if i == 0 else ()):
            w[ln + ".weight"] = 1 + 0.1 * torch.randn(cw.N_EMBD, generator=g)
            w[ln + ".bias"] = 0.1 * torch.randn(cw.N_EMBD, generator=g)
        b.load_state_dict(w, strict=True)
        blocks.append(b.cuda().to(bf))
    return blocks


def random_pools(n_slots, E, heads, g):
    shift_t, shift_c = (torch.randn(n_slots, E, generator=g).to(bf).cuda() for _ in range(2))
    return shift_t, shift_c, (torch.randn(n_slots, heads, 64, 64, generator=g) * 0.3).cuda()


def run_sublayers(tm, cm, x, cu, max_seqlen, pools, slots, kernels, **kw):
    from rwkv_lm_ext_amd import infctx
    shift_t, shift_c, wkv = (t.clone() for t in pools)
    with torch.no_grad():
        att = infctx.tmix_forward_packed(tm, x, cu, max_seqlen, shift_t, wkv, slots, pool_kernels=kernels, **kw)
        ffn = infctx.cmix_forward_packed(cm, x, cu, shift_c, slots, pool_kernels=kernels, **kw)
    torch.cuda.synchronize()
    return att, ffn, shift_t, shift_c, wkv


def test_two_decode_steps_in_place_equal_one_call_on_two_tokens():
    """slot_out == slot: the lerp's first-token workgroup reads the row that the keep launch writes behind it.  Every call runs on the
    same x [1,2n,C] (so that the GEMMs see one shape): the two-token call takes sequence s = rows 2s, 2s + 1; step 1 serves row 2s as a
    sequence of its own with slot p_s and row 2s + 1 as a sequence without state, step 2 the other way round."""
    tm, cm = sublayers()
    n, n_slots, E = 5, 8, tm.time_maa_x.shape[-1]
    home = [6, 0, 3, 7, 2]
    g = torch.Generator().manual_seed(41)
    x = torch.randn(1, 2 * n, E, generator=g).cuda().to(bf)
    pools = random_pools(n_slots, E, tm.n_head, g)
    both = run_sublayers(tm, cm, x, i32(range(0, 2 * n + 1, 2)), 2, pools, i32(home), True)
    cu1 = i32(range(2 * n + 1))
    first, second = i32(sum(([p, -1] for p in home), [])), i32(sum(([-1, p] for p in home), []))
    for kernels in (True, False):
        s1 = run_sublayers(tm, cm, x, cu1, 1, pools, first, kernels)
        s2 = run_sublayers(tm, cm, x, cu1, 1, s1[2:], second, kernels)
        for t in range(2):                                                # att, ffn
            assert same(s1[t][0, 0::2], both[t][0, 0::2]) and same(s2[t][0, 1::2], both[t][0, 1::2]), (kernels, t)
        for t in range(2, 5):                                             # the three pools
            assert same(s2[t], both[t]), (kernels, t)
    for s, p in enumerate(home):
        assert same(both[2][p], x[0, 2 * s + 1]) and same(both[3][p], x[0, 2 * s + 1])
    for p in (1, 4, 5):
        assert all(same(both[t][p], pools[t - 2][p]) for t in range(2, 5))


def test_layer_level_kernels_against_the_eager_pools():
    """A mixed batch -- prompts, decode tokens, an empty sequence, a sequence without state -- with out_slots and snap, then a decode-only
    batch with max_seqlen = 1: pool_kernels=True and False leave the same bits in the outputs, both shift pools and the WKV pool."""
    tm, cm = sublayers()
    E, n_slots = tm.time_maa_x.shape[-1], 16
    g = torch.Generator().manual_seed(51)
    lens, src, out = [130, 1, 0, 70, 1, 5], [4, 1, 6, 0, -1, 2], [8, 9, 10, 11, 12, n_slots]
    snap = (64, i32([0, 2, 2, 3, 5, 5, 5]), i32([13, 14, 15, 3, -1]))       # 130: both; the empty one: one it cannot earn; 70: 1 of 2 granted
    x = torch.randn(1, sum(lens), E, generator=g).cuda().to(bf)
    pools = random_pools(n_slots, E, tm.n_head, g)
    for kw in (dict(out_slots=i32(out), snap=snap), dict(snap=snap), dict(out_slots=i32(out)), {}):
        a = run_sublayers(tm, cm, x, i32(cum(lens)), max(lens), pools, i32(src), True, **kw)
        b = run_sublayers(tm, cm, x, i32(cum(lens)), max(lens), pools, i32(src), False, **kw)
        assert all(same(p, q) for p, q in zip(a, b)), sorted(kw)
        assert not same(a[2], pools[0]) and not same(a[3], pools[1])
    n = 12
    x = torch.randn(1, n, E, generator=g).cuda().to(bf)
    slots = [3, 15, -1, 0, 7, 8, n_slots, 1, 2, 9, 4, 11]
    a = run_sublayers(tm, cm, x, i32(range(n + 1)), 1, pools, i32(slots), True)
    b = run_sublayers(tm, cm, x, i32(range(n + 1)), 1, pools, i32(slots), False)
    assert all(same(p, q) for p, q in zip(a, b))
    for s, p in enumerate(slots):
        if 0 <= p < n_slots:
            assert same(a[2][p], x[0, s]) and same(a[3][p], x[0, s])
    # slots the kernels cannot take (int64: the eager channel-mix code has always cast them) stay with the eager code by default
    from rwkv_lm_ext_amd import infctx
    shift_c = pools[1].clone()
    with torch.no_grad():
        ffn = infctx.cmix_forward_packed(cm, x, i32(range(n + 1)), shift_c, i32(slots).long())
        with pytest.raises(RuntimeError, match="slots must be"):
            infctx.cmix_forward_packed(cm, x, i32(range(n + 1)), shift_c.clone(), i32(slots).long(), pool_kernels=True)
    torch.cuda.synchronize()
    assert same(ffn, a[1]) and same(shift_c, a[3])


def test_three_hundred_sequences():
    """Past 256 sequences: 297 decode tokens and three prompts (33, 70 and 40 tokens) among them, in place, against pool_kernels=False."""
    tm, cm = sublayers()
    E, n_slots = tm.time_maa_x.shape[-1], 320
    lens = [1] * 300
    lens[7], lens[150], lens[299] = 33, 70, 40
    g = torch.Generator().manual_seed(61)
    x = torch.randn(1, sum(lens), E, generator=g).cuda().to(bf)
    pools = random_pools(n_slots, E, tm.n_head, g)
    slots = torch.randperm(n_slots, generator=g)[:300].tolist()
    a = run_sublayers(tm, cm, x, i32(cum(lens)), max(lens), pools, i32(slots), True)
    b = run_sublayers(tm, cm, x, i32(cum(lens)), max(lens), pools, i32(slots), False)
    assert all(same(p, q) for p, q in zip(a, b))
    c = cum(lens)
    for s in (0, 7, 150, 255, 256, 257, 299):
        assert same(a[2][slots[s]], x[0, c[s + 1] - 1]) and same(a[3][slots[s]], x[0, c[s + 1] - 1]), s


def test_block_and_step_against_one_sequence_at_a_time():
    """step_packed on two blocks (ln0 in the first) with out_slots and snap against step_packed on every sequence alone -- n_seq = 1 over
    the same x, so that the GEMMs see the same shapes -- cut at each snapshot position and uncut; block_forward_packed is one layer of
    it; last_token_rows against host indexing."""
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import infctx
    blocks = two_blocks()
    E, heads, n_slots = cw.N_EMBD, cw.DIM_ATT // 64, 16
    lens, src, out = [130, 64, 0, 70, 5, 1], [4, 1, 6, 0, -1, 5], [8, 9, 10, 11, 12, 5]
    snap_slots, cu_snap = [13, 14, 15, 2, 3], [0, 2, 3, 3, 5, 5, 5]      # 130: both; 64: its one; 70: one of the two granted (slot 3 stays)
    g = torch.Generator().manual_seed(71)
    x = torch.randn(1, sum(lens), E, generator=g).cuda().to(bf)
    pools = infctx.PackedPools.create(2, n_slots, E, heads, "cuda", bf)
    assert (pools.shift_att.dtype, pools.shift_ffn.dtype, pools.wkv.dtype) == (bf, bf, torch.float32)
    pools.shift_att.copy_(torch.randn(2, n_slots, E, generator=g))
    pools.shift_ffn.copy_(torch.randn(2, n_slots, E, generator=g))
    pools.wkv.copy_(torch.randn(2, n_slots, heads, 64, 64, generator=g) * 0.3)
    fields = ("shift_att", "shift_ffn", "wkv")
    clone = lambda p: infctx.PackedPools(*(getattr(p, f).clone() for f in fields))
    before = clone(pools)
    c = cum(lens)
    snap = (64, i32(cu_snap), i32(snap_slots))
    with torch.no_grad():
        y = infctx.step_packed(blocks, x, i32(c), max(lens), pools, i32(src), out_slots=i32(out), snap=snap, pool_kernels=True)
        # one layer of it
        one_layer = clone(before)
        y0 = infctx.block_forward_packed(blocks[0], x, i32(c), max(lens), one_layer, 0, i32(src), out_slots=i32(out), snap=snap)
        y1 = infctx.block_forward_packed(blocks[1], y0, i32(c), max(lens), one_layer, 1, i32(src), out_slots=i32(out), snap=snap)
        torch.cuda.synchronize()
        assert same(y1, y) and all(same(getattr(one_layer, f), getattr(pools, f)) for f in fields)
        written = set()
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
                ya = infctx.step_packed(blocks, x, i32([c[s], c[s] + upto]), upto, alone, i32([home]), pool_kernels=True)
                torch.cuda.synchronize()
                for f in fields:
                    assert same(getattr(pools, f)[:, where], getattr(alone, f)[:, home]), (s, j, f)
                written.add(where)
                if j is None:
                    assert same(y[0, c[s]:c[s + 1]], ya[0, c[s]:c[s + 1]]), s
        assert written == {8, 9, 11, 12, 5, 13, 14, 15, 2}
        for p in set(range(n_slots)) - written:
            assert all(same(getattr(pools, f)[:, p], getattr(before, f)[:, p]) for f in fields), p
        # the rows the head needs: the last served token of every sequence, zeros for the empty one
        for cut in (max(lens), 64, 1):
            rows = infctx.last_token_rows(y, i32(c), cut)
            torch.cuda.synchronize()
            assert tuple(rows.shape) == (len(lens), E)
            for s, n in enumerate(lens):
                want = y[0, c[s] + min(n, cut) - 1] if n else torch.zeros(E, dtype=bf, device="cuda")
                assert same(rows[s], want), (cut, s)


def test_step_packed_replays_from_a_graph():
    """step_packed (two blocks, kernels on) captured once on one stream, replayed after x, cu_seqlens, slots and the pools were refilled in
    place with another partition of the rows: the replay equals an eager run on the same data, so no host read of a device array decides
    anything."""
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import infctx
    blocks = two_blocks()
    E, heads, n_slots, total, n_seq, bound = cw.N_EMBD, cw.DIM_ATT // 64, 8, 40, 5, 40
    g = torch.Generator().manual_seed(81)
    fields = ("shift_att", "shift_ffn", "wkv")

    def data(lens, slots):
        assert sum(lens) == total and len(lens) == n_seq and max(lens) <= bound
        return (torch.randn(1, total, E, generator=g).to(bf).cuda(), i32(cum(lens)), i32(slots),
                [torch.randn(2, n_slots, E, generator=g).to(bf).cuda(), torch.randn(2, n_slots, E, generator=g).to(bf).cuda(),
                 (torch.randn(2, n_slots, heads, 64, 64, generator=g) * 0.3).cuda()])

    first, second = data([10, 1, 0, 24, 5], [4, 1, 6, 0, -1]), data([1, 20, 9, 0, 10], [7, 7 - 5, n_slots, 3, 5])
    x, cu, slots = (t.clone() for t in first[:3])
    pools = infctx.PackedPools(*(t.clone() for t in first[3]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        infctx.step_packed(blocks, x, cu, bound, pools, slots, pool_kernels=True)       # warm-up: library, self-test, rocBLAS
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            y = infctx.step_packed(blocks, x, cu, bound, pools, slots, pool_kernels=True)
    torch.cuda.current_stream().wait_stream(side)
    for name, d in (("the captured partition", first), ("another partition", second)):
        for held, new in zip([x, cu, slots] + [getattr(pools, f) for f in fields], list(d[:3]) + d[3]):
            held.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eager = infctx.PackedPools(*(t.clone() for t in d[3]))
        with torch.no_grad():
            want = infctx.step_packed(blocks, d[0], d[1], bound, eager, d[2], pool_kernels=True)
        torch.cuda.synchronize()
        assert same(y, want), name
        assert all(same(getattr(pools, f), getattr(eager, f)) for f in fields), name
    assert not same(first[1], second[1])
