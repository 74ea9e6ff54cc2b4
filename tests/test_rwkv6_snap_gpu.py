"""State snapshots and a separate output slot of the packed stateful inference on the GPU: rwkv6_forward_varlen_snap_* (include/wkv6_amd.h)
through wkv6_op.rwkv6.forward_varlen_*(state_slot_out=, snap_every=, cu_snap=, snap_slot=), torch.ops.rwkv6.forward_varlen_snap_* and
infctx.tmix_forward_packed / cmix_forward_packed(out_slots=, snap=).

Contract: for every sequence, y and the destination slot equal BIT FOR BIT what the plain forward_varlen_<io> call leaves from the same
source state, and snapshot j equals the final state that call leaves when the sequence is cut to (j + 1) * snap_every tokens.  Every test
but the oracle one compares bits, against calls that existed before the snapshots did.  The plain calls of the main batch are made once
per (I/O type, route) and shared (`reference`); nobody writes to what it returns."""
import numpy as np
import pytest
import torch

from conftest import max_norm_err
from test_rwkv6_varlen_gpu import IOS, bf, bits, host, make, oracle_one, ops, packed, rows_of, same, state_tol  # noqa: F401 (ops: fixture)

pytestmark = pytest.mark.gpu
# both sides of the routing threshold (32) and of a 64-token group, exactly one and two groups, an empty sequence
LENS = [0, 1, 31, 63, 64, 65, 128, 130, 200]
H, N_SLOTS = 2, 32
SRC = [3, 17, 8, 29, 0, 12, 25, 6, 21]              # source slot of the nine sequences, permuted
DST = [10, 1, 30, 14, 23, 5, 19, 27, 9]             # destination slots, distinct from each other and from every source
SNAPS = [13, 2, 28, 7, 20, 31, 11, 24, 16]          # snapshot slots; nobody names 4, 15, 18, 22, 26
assert len(set(SRC + DST + SNAPS)) == 27 and max(SRC + DST + SNAPS) < N_SLOTS
LEVELS = (64, 128, 192)                             # every snapshot position of LENS at snap_every = 64 or 128


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device="cuda")


def snap_call(ops, d, pool, src, dst, snap_every=0, cu_snap=None, snap_slot=None, algo=None, max_seqlen=None, ws=None, y=None):
    fn = getattr(ops.rwkv6, {torch.bfloat16: "forward_varlen_bf16", torch.float16: "forward_varlen_fp16",
                             torch.float32: "forward_varlen_fp32"}[d["io"]])
    y = torch.full_like(d["r"], float("nan")) if y is None else y
    fn(d["total"], 64 * d["H"], d["H"], pool, src, d["r"], d["k"], d["v"], d["eew"], d["u"], y, d["cu"],
       d["max_seqlen"] if max_seqlen is None else max_seqlen, algo=algo, ws=ws, state_slot_out=dst, snap_every=snap_every,
       cu_snap=cu_snap, snap_slot=snap_slot)
    return y


def cut(d, keep):
    """The batch whose cu_seqlens cuts sequence s to its first keep[s] tokens (the rows gathered, nothing else changed)."""
    c = d["cu"].tolist()
    idx = torch.cat([torch.arange(c[s], c[s] + n) for s, n in enumerate(keep)]).cuda()
    out = dict(d, lens=list(keep), total=int(idx.numel()), max_seqlen=max(keep), cu=i32(np.concatenate([[0], np.cumsum(keep)])))
    for x in ("r", "k", "v", "eew"):
        out[x] = d[x][idx].contiguous()
    return out


def plain_prefix_states(ops, d, lens, src, algo, levels):
    """{L: the pool the plain call leaves, from d["pool"], when every sequence of L tokens and more is cut to L and the others to 0}."""
    finals = {}
    for L in levels:
        p = d["pool"].clone()
        packed(ops, cut(d, [L if n >= L else 0 for n in lens]), p, src, algo=algo)
        finals[L] = p
    return finals


_REF = {}


def reference(ops, io, algo):
    """The plain calls on the main batch: (batch, y, pool, {L: pool of the batch cut to L tokens}), all in place on the SOURCE slots."""
    if (io, algo) not in _REF:
        d = make(LENS, IOS[io], seed=21, heads=H, n_slots=N_SLOTS)
        pool = d["pool"].clone()
        y = packed(ops, d, pool, i32(SRC), algo=algo)
        finals = plain_prefix_states(ops, d, LENS, i32(SRC), algo, LEVELS)
        torch.cuda.synchronize()
        _REF[(io, algo)] = (d, y, pool, finals)
    return _REF[(io, algo)]


def plan(lens, snap_every):
    counts = [n // snap_every for n in lens]
    return counts, [0] + list(np.cumsum(counts))


@pytest.mark.parametrize("variant", ["routed", "algo_scan"])
@pytest.mark.parametrize("snap_every", [64, 128])
@pytest.mark.parametrize("io", sorted(IOS))
def test_snapshots_equal_todays_prefix_calls(ops, io, snap_every, variant):
    algo = "scan" if variant == "algo_scan" else None
    d, y_ref, pool_ref, finals = reference(ops, io, algo)
    counts, cs = plan(LENS, snap_every)
    snap_slot = SNAPS[:cs[-1]]
    pool = d["pool"].clone()
    y = snap_call(ops, d, pool, i32(SRC), i32(DST), snap_every, i32(cs), i32(snap_slot), algo=algo)
    torch.cuda.synchronize()
    assert same(y, y_ref), (io, snap_every, variant, "y")
    written = set()
    for s, n in enumerate(LENS):
        if n == 0:
            continue                                                     # (its destination is checked with the untouched slots)
        assert same(pool[DST[s]], pool_ref[SRC[s]]), (io, snap_every, variant, s, n, "final state")
        written.add(DST[s])
        for j in range(counts[s]):
            p = snap_slot[cs[s] + j]
            assert same(pool[p], finals[(j + 1) * snap_every][SRC[s]]), (io, snap_every, variant, s, n, j, "snapshot")
            written.add(p)
    for p in range(N_SLOTS):                                             # the sources among them
        if p not in written:
            assert same(pool[p], d["pool"][p]), (io, snap_every, variant, p, "untouched")
    if snap_every == 64:                                                 # a snapshot at the sequence's end is stored as well as the final state
        s = LENS.index(128)
        assert counts[s] == 2 and same(pool[snap_slot[cs[s] + 1]], pool[DST[s]])


@pytest.mark.parametrize("variant", ["routed", "algo_scan"])
@pytest.mark.parametrize("io", sorted(IOS))
def test_continuing_from_a_snapshot(ops, io, variant):
    """One plain call runs, for every snapshot (s, j), the rest of sequence s from the snapshot's slot: its y rows and its final state are
    those of the uncut sequence.  bf16 on the routed call leaves out the rests below 32 tokens (1, 2 and 8 tokens here): the plain call
    hands those to the exact scan while the uncut sequence ran them on the chunked kernel, and the two kernels round differently."""
    algo = "scan" if variant == "algo_scan" else None
    d, y_ref, pool_ref, _ = reference(ops, io, algo)
    counts, cs = plan(LENS, 64)
    snap_slot = SNAPS[:cs[-1]]
    pool = d["pool"].clone()
    snap_call(ops, d, pool, i32(SRC), i32(DST), 64, i32(cs), i32(snap_slot), algo=algo)
    c = d["cu"].tolist()
    pieces = [(s, j, LENS[s] - 64 * (j + 1)) for s in range(len(LENS)) for j in range(counts[s])]
    pieces = [(s, j, rest) for s, j, rest in pieces if rest > 0 and (rest >= 32 or not (io == "bf16" and algo is None))]
    assert len(pieces) == (4 if io == "bf16" and algo is None else 7)
    idx = torch.cat([torch.arange(c[s] + 64 * (j + 1), c[s + 1]) for s, j, _ in pieces]).cuda()
    rests = [rest for _, _, rest in pieces]
    d2 = dict(d, lens=rests, total=int(idx.numel()), max_seqlen=max(rests), cu=i32(np.concatenate([[0], np.cumsum(rests)])))
    for x in ("r", "k", "v", "eew"):
        d2[x] = d[x][idx].contiguous()
    y2 = packed(ops, d2, pool, i32(snap_slot[cs[s] + j] for s, j, _ in pieces), algo=algo)
    torch.cuda.synchronize()
    t0 = 0
    for s, j, rest in pieces:
        assert same(y2[t0:t0 + rest], y_ref[c[s + 1] - rest:c[s + 1]]), (io, variant, s, j, rest, "y")
        assert same(pool[snap_slot[cs[s] + j]], pool_ref[SRC[s]]), (io, variant, s, j, rest, "final state")
        t0 += rest


@pytest.mark.parametrize("io", sorted(IOS))
def test_fan_out_from_one_source_slot(ops, io):
    lens, src, dst = [40, 70, 5], [7, 7, 7], [1, 20, 12]
    d = make(lens, IOS[io], seed=22, heads=H, n_slots=N_SLOTS)
    pool = d["pool"].clone()
    y = snap_call(ops, d, pool, i32(src), i32(dst), 64, i32([0, 0, 1, 1]), i32([25]))
    private = d["pool"].clone()                                          # the plain call, in place, from a private copy of slot 7 each
    for p in dst:
        private[p] = d["pool"][7]
    y_ref = packed(ops, d, private, i32(dst))
    at64 = d["pool"].clone()
    packed(ops, cut(d, [0, 64, 0]), at64, i32(src))
    torch.cuda.synchronize()
    assert same(y, y_ref)
    for p in dst:
        assert same(pool[p], private[p]), p
    assert same(pool[25], at64[7])
    for p in range(N_SLOTS):
        if p not in dst + [25]:
            assert same(pool[p], d["pool"][p]), p                        # slot 7 among them


@pytest.mark.parametrize("io", sorted(IOS))
def test_defaults_through_the_new_symbol_are_todays_call(ops, io):
    d, y_ref, pool_ref, _ = reference(ops, io, None)
    pool, y = d["pool"].clone(), torch.full_like(d["r"], float("nan"))
    getattr(torch.ops.rwkv6, f"forward_varlen_snap_{io}")(d["total"], 64 * H, H, pool, i32(SRC), None, d["r"], d["k"], d["v"], d["eew"],
                                                          d["u"], y, d["cu"], d["max_seqlen"], 0, None, None)
    torch.cuda.synchronize()
    assert same(y, y_ref) and same(pool, pool_ref)


@pytest.mark.parametrize("io", sorted(IOS))
def test_nothing_else_is_touched(ops, io):
    """NaN-filled guard slots on both sides of the pool; source, destination and snapshot slots of -1 and n_slots + 5; a cu_snap that grants
    fewer snapshots than a sequence could take, more than it could take, and entries beyond n_snap; a max_seqlen that cuts a sequence
    below a boundary.  Only the seven named slots change; gap rows of y are +0."""
    lens, max_len, out = [70, 130, 0, 200, 64], 150, N_SLOTS + 5
    src, dst = [2, -1, 9, out, 4], [11, 13, 20, 15, out]
    #            seq 0: 1 of 3 granted | seq 1: 1 granted of 2 | empty | seq 3, cut to 150: 2 of 3, the first skipped | seq 4: [9, 1000) -> [9, 10)
    snap_slot, cu_snap = [21, 22, 23, 24, 25, 26, -1, 27, 28, 29], [0, 3, 4, 6, 9, 1000]
    d = make(lens, IOS[io], seed=23, heads=H, lead=3, tail=5, n_slots=N_SLOTS)
    c = d["cu"].tolist()
    gaps = [slice(0, c[0]), slice(c[3] + max_len, c[4]), slice(c[5], d["total"])]
    assert [g.stop - g.start for g in gaps] == [3, 50, 5]
    for x in ("r", "k", "v", "eew"):
        for g in gaps:
            d[x][g] = float("nan")
    guard = 8
    buf = torch.full((guard + N_SLOTS + guard, H, 64, 64), float("nan"), device="cuda")
    pool = buf[guard:guard + N_SLOTS]
    for p in (2, 4):
        pool[p] = d["pool"][p]
    before = buf.clone()
    y = snap_call(ops, d, pool, i32(src), i32(dst), 64, i32(cu_snap), i32(snap_slot), max_seqlen=max_len)
    # the plain call, in place: every sequence from a private copy of its source (a zeroed slot for "no state")
    want = {}
    for limit in (max_len, 64, 128):
        p = torch.zeros_like(d["pool"])
        p[11], p[30] = d["pool"][2], d["pool"][4]
        want[limit] = (packed(ops, d, p, i32([11, 13, -1, 15, 30]), max_seqlen=limit), p)
    torch.cuda.synchronize()
    for g in gaps:
        assert not bool(bits(y[g]).any()), g                              # +0 bitwise
    live = torch.ones(d["total"], dtype=torch.bool, device="cuda")
    for g in gaps:
        live[g] = False
    assert bool(torch.isfinite(y[live]).all()) and same(y[live], want[max_len][0][live])
    expect = {11: want[max_len][1][11], 13: want[max_len][1][13], 15: want[max_len][1][15],
              21: want[64][1][11], 24: want[64][1][13], 27: want[128][1][15], 29: want[64][1][30]}
    touched = torch.zeros(buf.shape[0], dtype=torch.bool, device="cuda")
    for p, state in expect.items():
        assert same(pool[p], state), (io, p)
        touched[guard + p] = True
    assert same(buf[~touched], before[~touched])


@pytest.mark.parametrize("io", ["bf16", "fp32"])
def test_oracle_parity_of_the_snapshots(ops, oracle, io):
    d, _, _, _ = reference(ops, io, None)
    counts, cs = plan(LENS, 64)
    snap_slot = SNAPS[:cs[-1]]
    pool = d["pool"].clone()
    snap_call(ops, d, pool, i32(SRC), i32(DST), 64, i32(cs), i32(snap_slot))
    torch.cuda.synchronize()
    c = d["cu"].tolist()
    for s, n in enumerate(LENS):
        for j in range(counts[s]):
            _, so = oracle_one(oracle, d, slice(c[s], c[s] + 64 * (j + 1)), d["pool"][SRC[s]])
            e = max_norm_err(host(pool[snap_slot[cs[s] + j]]), so)
            print(f"snapshot {io} seq {s} (len {n}) after {64 * (j + 1)} tokens: {e:.2e}")
            assert e <= state_tol(d["io"], True), (s, j, e)               # (sequences of 64 tokens and more: bf16 ran the chunked kernel)


def test_a_prefill_with_snapshots_replays_from_a_graph(ops):
    """One captured prefill step (preparation, chunked launch, scan launch for the window below 32), replayed with other snapshot slots
    written into the captured snap_slot tensor."""
    lens, src, dst = [128, 64, 200, 20], [3, 9, 0, 5], [10, 11, 12, 13]
    d = make(lens, bf, seed=24, heads=H, n_slots=N_SLOTS)
    counts, cs = plan(lens, 64)
    choices = ([20, 21, 22, 23, 24, 25], [31, 30, 29, 28, 27, 26], [25, 20, 24, 21, 23, 22])
    ws = ops.new_rwkv6_varlen_workspace(len(lens), "cuda")
    eager = []
    for ch in choices:
        p = d["pool"].clone()
        eager.append((snap_call(ops, d, p, i32(src), i32(dst), 64, i32(cs), i32(ch), ws=ws), p))
    torch.cuda.synchronize()
    assert not same(eager[0][1], eager[1][1])
    pool, y, snap_slot = d["pool"].clone(), torch.empty_like(d["r"]), i32(choices[0])
    src_t, dst_t, cs_t = i32(src), i32(dst), i32(cs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        snap_call(ops, d, pool, src_t, dst_t, 64, cs_t, snap_slot, ws=ws, y=y)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            snap_call(ops, d, pool, src_t, dst_t, 64, cs_t, snap_slot, ws=ws, y=y)
    torch.cuda.current_stream().wait_stream(side)
    for i in (1, 2):
        pool.copy_(d["pool"])
        snap_slot.copy_(i32(choices[i]))
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same(y, eager[i][0]) and same(pool, eager[i][1]), i


def test_many_workgroups(ops):
    """H = 32, C = 2048, 40 sequences of 64 to 192 tokens: 1280 workgroups; final states in place (no state_slot_out)."""
    lens = [64, 128, 192] + [64 + (37 * i) % 129 for i in range(3, 40)]
    assert len(lens) == 40 and min(lens) == 64 and max(lens) == 192
    counts, cs = plan(lens, 64)
    n_slots = 40 + cs[-1]
    d = make(lens, bf, seed=25, heads=32, n_slots=n_slots)
    perm = torch.randperm(n_slots, generator=torch.Generator().manual_seed(26)).tolist()
    src, snap_slot = perm[:40], perm[40:]
    pool = d["pool"].clone()
    y = snap_call(ops, d, pool, i32(src), None, 64, i32(cs), i32(snap_slot))
    ref = d["pool"].clone()
    y_ref = packed(ops, d, ref, i32(src))
    finals = plain_prefix_states(ops, d, lens, i32(src), None, LEVELS)
    torch.cuda.synchronize()
    assert same(y, y_ref)
    for s in range(40):
        assert same(pool[src[s]], ref[src[s]]), (s, lens[s])
        for j in range(counts[s]):
            assert same(pool[snap_slot[cs[s] + j]], finals[64 * (j + 1)][src[s]]), (s, lens[s], j)


def test_layer_level_out_slots_and_snapshots():
    """infctx.tmix_forward_packed / cmix_forward_packed with out_slots and snap against the same functions without them, run on every
    sequence alone (n_seq = 1 over the same x, so that the GEMMs see the same shapes) cut at each snapshot position and uncut: outputs,
    WKV pool and both shift pools compare bitwise, a snapshot's shift token and WKV state lie in the same slot number."""
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import callers, infctx
    tm = callers.Tmix_x060(cw.N_EMBD, cw.DIM_ATT)
    tm.load_state_dict(cw.tmix_weights(torch.Generator().manual_seed(11), layer_id=1), strict=True)
    tm = tm.cuda().to(bf)
    cm = callers.CMix_x060(cw.N_EMBD, cw.DIM_FFN)
    cm.load_state_dict(cw.cmix_weights(torch.Generator().manual_seed(12)), strict=True)
    cm = cm.cuda().to(bf)
    E, heads, n_slots = cw.N_EMBD, tm.n_head, 16
    lens, src, out = [130, 64, 0, 70, 5], [4, 1, 6, 0, -1], [8, 9, 10, 11, 12]
    snap_slots, cu_snap = [13, 14, 15, 2, 3], [0, 2, 3, 3, 5, 5]          # 130: both; 64: its one; 70: one of the two granted (slot 3 stays)
    g = torch.Generator().manual_seed(14)
    x = torch.randn(1, sum(lens), E, generator=g).cuda().to(bf)
    assert tm._use_fused(x) and cm._use_fused(x)
    shift_t, shift_c = (torch.randn(n_slots, E, generator=g).to(bf).cuda() for _ in range(2))
    wkv_pool = (torch.randn(n_slots, heads, 64, 64, generator=g) * 0.3).cuda()
    before = (shift_t.clone(), shift_c.clone(), wkv_pool.clone())
    c = np.concatenate([[0], np.cumsum(lens)]).tolist()
    snap = (64, i32(cu_snap), i32(snap_slots))
    with torch.no_grad():
        att = infctx.tmix_forward_packed(tm, x, i32(c), max(lens), shift_t, wkv_pool, i32(src), out_slots=i32(out), snap=snap)
        ffn = infctx.cmix_forward_packed(cm, x, i32(c), shift_c, i32(src), out_slots=i32(out), snap=snap)
        written = set()
        for s, n in enumerate(lens):
            if n == 0:
                continue
            for j in list(range(min(n // 64, cu_snap[s + 1] - cu_snap[s]))) + [None]:
                upto, where = (n, out[s]) if j is None else (64 * (j + 1), snap_slots[cu_snap[s] + j])
                st, sc, wp = (t.clone() for t in before)
                home = src[s] if src[s] >= 0 else 7                      # "no state": a zeroed slot of the copies
                if src[s] < 0:
                    st[home], sc[home], wp[home] = 0, 0, 0
                one, cu1 = i32([home]), i32([c[s], c[s] + upto])
                att1 = infctx.tmix_forward_packed(tm, x, cu1, upto, st, wp, one)
                ffn1 = infctx.cmix_forward_packed(cm, x, cu1, sc, one)
                torch.cuda.synchronize()
                assert same(wkv_pool[where], wp[home]), (s, j, "wkv state")
                assert same(shift_t[where], st[home]) and same(shift_c[where], sc[home]), (s, j, "shift tokens")
                assert same(shift_t[where], x[0, c[s] + upto - 1]), (s, j)
                written.add(where)
                if j is None:
                    rows = slice(c[s], c[s + 1])
                    assert same(att[0, rows], att1[0, rows]) and same(ffn[0, rows], ffn1[0, rows]), (s, "outputs")
    assert written == {8, 9, 11, 12, 13, 14, 15, 2}
    for p in range(n_slots):
        if p not in written:
            assert same(shift_t[p], before[0][p]) and same(shift_c[p], before[1][p]) and same(wkv_pool[p], before[2][p]), p
