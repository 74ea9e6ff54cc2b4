"""Tmix_x060.fuse_lowrank under the serving step (infctx.step_packed): two small blocks, C = 128, H = 2, the weights of
oracle/caller_weights.py.

(a) A mixed batch of prompts of 1..40 tokens and decode tokens, an empty sequence and a sequence without state among them, equals the
    same step one sequence at a time bit for bit -- n_seq = 1 over the same x, so that the GEMMs see the same shapes --, outputs and pools.
(b) Captured in a graph after one warm-up call, the replay equals the eager call bit for bit, also after everything was refilled in place.
(c) The attribute decides the library calls: off, the time-mix sub-layer makes exactly today's (two wkv6_ddlerp_slots_forward); on, one
    wkv6_tmix_lerp_lowrank_bf16 and one wkv6_decay_lowrank_bf16 behind their workspace queries, and no ddlerp."""
import pytest
import torch

from test_packed_shift_gpu import cum, i32, same, two_blocks

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
FIELDS = ("shift_att", "shift_ffn", "wkv")


def fused_blocks():
    blocks = two_blocks()
    for b in blocks:
        b.requires_grad_(False)
        b.att.fuse_lowrank = True
    return blocks


def filled_pools(n_slots, E, heads, g):
    from rwkv_lm_ext_amd import infctx
    return infctx.PackedPools(torch.randn(2, n_slots, E, generator=g).to(bf).cuda(), torch.randn(2, n_slots, E, generator=g).to(bf).cuda(),
                              (torch.randn(2, n_slots, heads, 64, 64, generator=g) * 0.3).cuda())


def clone(p):
    from rwkv_lm_ext_amd import infctx
    return infctx.PackedPools(*(getattr(p, f).clone() for f in FIELDS))


def test_step_with_fuse_lowrank_equals_one_sequence_at_a_time():
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import infctx
    blocks = fused_blocks()
    E, heads, n_slots = cw.N_EMBD, cw.DIM_ATT // 64, 16
    lens, src, out = [40, 1, 17, 0, 1, 16, 1, 5, 1, 33], [4, 1, 6, 0, -1, 2, 9, 3, 10, 7], [8, 1, 6, 0, 12, 2, 9, 3, 10, 11]
    g = torch.Generator().manual_seed(91)
    x = torch.randn(1, sum(lens), E, generator=g).cuda().to(bf)
    before = filled_pools(n_slots, E, heads, g)
    pools, c = clone(before), cum(lens)
    with torch.no_grad():
        y = infctx.step_packed(blocks, x, i32(c), max(lens), pools, i32(src), out_slots=i32(out), pool_kernels=True)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(y).any())
        written = set()
        for s, n in enumerate(lens):
            if n == 0:
                continue
            alone = clone(before)
            home = src[s] if src[s] >= 0 else 15                             # "no state": a zeroed slot of the copies
            if src[s] < 0:
                for f in FIELDS:
                    getattr(alone, f)[:, home] = 0
            ya = infctx.step_packed(blocks, x, i32([c[s], c[s + 1]]), n, alone, i32([home]), pool_kernels=True)
            torch.cuda.synchronize()
            assert same(y[0, c[s]:c[s + 1]], ya[0, c[s]:c[s + 1]]), s
            for f in FIELDS:
                assert same(getattr(pools, f)[:, out[s]], getattr(alone, f)[:, home]), (s, f)
            written.add(out[s])
        for p in set(range(n_slots)) - written:
            assert all(same(getattr(pools, f)[:, p], getattr(before, f)[:, p]) for f in FIELDS), p


def test_step_with_fuse_lowrank_replays_from_a_graph():
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import infctx
    blocks = fused_blocks()
    E, heads, n_slots, total, n_seq, bound = cw.N_EMBD, cw.DIM_ATT // 64, 8, 40, 5, 40
    g = torch.Generator().manual_seed(92)

    def data(lens, slots):
        assert sum(lens) == total and len(lens) == n_seq and max(lens) <= bound
        return torch.randn(1, total, E, generator=g).to(bf).cuda(), i32(cum(lens)), i32(slots), filled_pools(n_slots, E, heads, g)

    first, second = data([10, 1, 0, 24, 5], [4, 1, 6, 0, -1]), data([1, 20, 9, 0, 10], [7, 2, n_slots, 3, 5])
    x, cu, slots = (t.clone() for t in first[:3])
    pools = clone(first[3])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        infctx.step_packed(blocks, x, cu, bound, pools, slots, pool_kernels=True)       # the warm-up call: the weight copies exist from here on
        torch.cuda.synchronize()
        held = [b.att._lowrank_weights() for b in blocks]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            y = infctx.step_packed(blocks, x, cu, bound, pools, slots, pool_kernels=True)
    torch.cuda.current_stream().wait_stream(side)
    assert all(a is b for h, blk in zip(held, blocks) for a, b in zip(h, blk.att._lowrank_weights()))      # the capture made no new copies
    for name, d in (("the captured partition", first), ("another partition", second)):
        for dst, new in zip([x, cu, slots] + [getattr(pools, f) for f in FIELDS], list(d[:3]) + [getattr(d[3], f) for f in FIELDS]):
            dst.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eager = clone(d[3])
        with torch.no_grad():
            want = infctx.step_packed(blocks, d[0], d[1], bound, eager, d[2], pool_kernels=True)
        torch.cuda.synchronize()
        assert same(y, want), name
        assert all(same(getattr(pools, f), getattr(eager, f)) for f in FIELDS), name


def test_the_attribute_decides_the_library_calls(monkeypatch):
    """Recorded without running a kernel, as tests/test_op_calls_gpu.py does."""
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import _lib, infctx
    from test_op_calls_gpu import Recorder
    blocks = fused_blocks()
    tm = blocks[1].att
    E, heads, n_slots = cw.N_EMBD, cw.DIM_ATT // 64, 4
    x = torch.zeros(1, 8, E, dtype=bf, device="cuda")
    cu, slots = i32([0, 3, 8]), i32([1, 0])
    shift, wkv = torch.zeros(n_slots, E, dtype=bf, device="cuda"), torch.zeros(n_slots, heads, 64, 64, device="cuda")
    tm._lowrank_weights()
    rec = Recorder(torch)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(_lib, "_selftested", set(range(torch.cuda.device_count())))

    def symbols(on):
        tm.fuse_lowrank = on
        del rec.records[:]
        with torch.no_grad():
            infctx.tmix_forward_packed(tm, x, cu, 8, shift, wkv, slots, pool_kernels=True)
        torch.cuda.synchronize()
        return [r[1] for r in rec.records]

    off, on = symbols(False), symbols(True)
    assert off[:2] == ["wkv6_ddlerp_slots_forward"] * 2 and not any("lowrank" in s for s in off)
    assert on[:4] == ["wkv6_lowrank_workspace_bytes", "wkv6_tmix_lerp_lowrank_bf16", "wkv6_lowrank_workspace_bytes", "wkv6_decay_lowrank_bf16"]
    assert not any("ddlerp" in s for s in on) and on[4:] == off[2:]           # the operator, GroupNorm * gate and shift_keep as before
    tmix = rec.records[1][2]
    assert tmix[:4] == [8, 2, E, 32] and tmix[7] == n_slots and tmix[15] == 4096 and len(tmix) == 17
    dec = rec.records[3][2]
    assert dec[:4] == [8, E, 64, cw.DIM_ATT] and dec[10] == 4096 and len(dec) == 12
