"""Long sequences of the packed stateful inference cut over T on the GPU: rwkv6_forward_varlen_split_bf16 (include/wkv6_amd.h) through
wkv6_op.rwkv6.forward_varlen_bf16(seg_len=), torch.ops.rwkv6.forward_varlen_split_bf16 and infctx.tmix_forward_packed(seg_len=).

Contract: a sequence that is not cut equals the snap call BIT FOR BIT, and so do a cut sequence's first seg_len rows of y and its snapshots
up to position seg_len; y of a cut sequence equals the dense two-level path (rwkv6.forward_bf16 under dispatch(tsplit=)) bit for bit; behind
the first segment the results hold the bounds of test_wkv6_gpu.py::test_two_level_scan_forward_for_few_long_sequences, in that test's input
regime (rand_inputs(..., "init")): y the bf16 contract of oracle/contract.py, states max_norm_err <= 1e-3 against the oracle's, y within
2^-8 max|y| of the uncut call.  The uncut snap calls and the oracle's results on the main batch are made once and shared (`reference`);
nobody writes to what it returns."""
import numpy as np
import pytest
import torch

from conftest import max_norm_err
from test_rwkv6_snap_gpu import cut, i32, plan, snap_call
from test_rwkv6_varlen_gpu import bf, bits, host, oracle_one, ops, same  # noqa: F401 (ops: fixture)
from test_wkv6_gpu import check, rand_inputs

pytestmark = pytest.mark.gpu
H, C, N_SLOTS = 2, 128, 48
# an empty sequence, a decode token, both sides of one, two, three and four 64-token groups
L = [0, 1, 63, 64, 65, 127, 128, 129, 192, 200, 257]
SRC = [3, 17, 8, 29, 0, 12, 25, 6, 21, 40, 33]      # source slot of the eleven sequences, permuted
DST = [10, 1, 30, 14, 23, 5, 19, 27, 9, 44, 36]     # destination slots, distinct from each other and from every source
SNAPS = [13, 2, 28, 7, 20, 31, 11, 24, 16, 4, 15, 18, 22, 26, 32, 34, 35]   # snapshot slots (17 at snap_every = 64)
assert len(set(SRC + DST + SNAPS)) == 39 and max(SRC + DST + SNAPS) < N_SLOTS
SEGS = (64, 128)
STATE_TOL = 1e-3                                    # the two-level test's bound on the prefill's final state


def make_init(lens, seed, heads=H, lead=0, tail=0, n_slots=N_SLOTS):
    """test_rwkv6_varlen_gpu.make in the regime of the two-level test: rand_inputs(seed, 1, total, heads, "init"), a random bf16-representable
    state in every slot."""
    total = lead + sum(lens) + tail
    r, k, v, w, u, _ = rand_inputs(seed, 1, total, heads, "init")
    dv = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dt).contiguous()
    w_ = dv(w[0], torch.float32)
    g = torch.Generator().manual_seed(seed + 1000)
    pool = (torch.randn(n_slots, heads, 64, 64, generator=g) * 0.5).to(bf).float().cuda()
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]) + lead, dtype=torch.int32, device="cuda")
    return dict(r=dv(r[0], bf), k=dv(k[0], bf), v=dv(v[0], bf), w=w_, eew=torch.exp(-torch.exp(w_)).contiguous(), u=dv(u, bf), pool=pool,
                cu=cu, lens=list(lens), H=heads, total=total, io=bf, max_seqlen=max(max(lens), 1))


def split_call(ops, d, pool, src, dst, seg_len, snap_every=0, cu_snap=None, snap_slot=None, max_seqlen=None, ws=None, y=None):
    y = torch.full_like(d["r"], float("nan")) if y is None else y
    ops.rwkv6.forward_varlen_bf16(d["total"], 64 * d["H"], d["H"], pool, src, d["r"], d["k"], d["v"], d["eew"], d["u"], y, d["cu"],
                                  d["max_seqlen"] if max_seqlen is None else max_seqlen, ws=ws, state_slot_out=dst, snap_every=snap_every,
                                  cu_snap=cu_snap, snap_slot=snap_slot, seg_len=seg_len)
    return y


_REF = {}


def reference(ops):
    """The main batch, and the uncut snap call on it with every snapshot of snap_every = 64: (batch, y, pool, counts, cu_snap)."""
    if "snap" not in _REF:
        d = make_init(L, seed=31)
        counts, cs = plan(L, 64)
        assert cs[-1] == len(SNAPS)
        pool = d["pool"].clone()
        y = snap_call(ops, d, pool, i32(SRC), i32(DST), 64, i32(cs), i32(SNAPS))
        torch.cuda.synchronize()
        _REF["snap"] = (d, y, pool, counts, cs)
    return _REF["snap"]


def oracle_states(oracle, d, src):
    """{(s, n): (y, state) of the oracle on the first n tokens of sequence s from its source slot}, for n = every multiple of 64 and the end."""
    if "oracle" not in _REF:
        c, out = d["cu"].tolist(), {}
        for s, n in enumerate(d["lens"]):
            for upto in sorted(set(list(range(64, n + 1, 64)) + ([n] if n else []))):
                out[(s, upto)] = oracle_one(oracle, d, slice(c[s], c[s] + upto), d["pool"][src[s]])
        _REF["oracle"] = out
    return _REF["oracle"]


def within_one_pass_bound(y, y_ref, what):
    a, b = host(y_ref), host(y)
    e, m = float(np.abs(a - b).max()), float(np.abs(a).max())
    print(f"{what}: max |y - y_uncut| {e:.3e}, bound 2^-8 max|y| = {2.0 ** -8 * m:.3e}")
    assert e <= 2.0 ** -8 * m, what


def test_nothing_changes_when_nothing_is_cut(ops):
    d, y_ref, pool_ref, _, cs = reference(ops)
    for seg_len in (0, 320):
        pool, y = d["pool"].clone(), torch.full_like(d["r"], float("nan"))
        torch.ops.rwkv6.forward_varlen_split_bf16(d["total"], C, H, pool, i32(SRC), i32(DST), d["r"], d["k"], d["v"], d["eew"], d["u"], y,
                                                  d["cu"], d["max_seqlen"], 64, i32(cs), i32(SNAPS), seg_len)
        torch.cuda.synchronize()
        assert same(y, y_ref), seg_len
        assert same(pool, pool_ref), seg_len


@pytest.mark.parametrize("seg_len", SEGS)
def test_first_segment_exact_and_uncut_sequences_unchanged(ops, seg_len):
    d, y_ref, pool_ref, counts, cs = reference(ops)
    pool = d["pool"].clone()
    y = split_call(ops, d, pool, i32(SRC), i32(DST), seg_len, 64, i32(cs), i32(SNAPS))
    torch.cuda.synchronize()
    c = d["cu"].tolist()
    n_cut = 0
    for s, n in enumerate(L):
        head = slice(c[s], c[s] + min(n, seg_len))
        assert same(y[head], y_ref[head]), (seg_len, s, n, "first segment of y")
        for j in range(counts[s]):
            if 64 * (j + 1) <= seg_len:
                p = SNAPS[cs[s] + j]
                assert same(pool[p], pool_ref[p]), (seg_len, s, n, j, "snapshot inside the first segment")
        if n <= seg_len:
            assert same(pool[DST[s]], pool_ref[DST[s]]), (seg_len, s, n, "destination of an uncut sequence")
        else:
            n_cut += 1
            assert bool(torch.isfinite(y[c[s]:c[s + 1]].float()).all()) and bool(torch.isfinite(pool[DST[s]]).all())
    assert n_cut == {64: 7, 128: 4}[seg_len]
    for p in range(N_SLOTS):                                             # the sources and the empty sequence's destination among them
        if p not in DST[1:] + SNAPS:
            assert same(pool[p], d["pool"][p]), (seg_len, p, "untouched")


@pytest.mark.parametrize("T,seg_len", [(512, 128), (256, 64)])
def test_same_arithmetic_as_the_dense_two_level_path(ops, T, seg_len):
    d = make_init([T], seed=32, n_slots=4)
    pool = d["pool"].clone()
    y = split_call(ops, d, pool, i32([2]), None, seg_len)
    state = d["pool"][2:3].clone()
    want = torch.empty(1, T, C, device="cuda", dtype=bf)
    with ops.dispatch(split=0, tsplit=4):
        ops.rwkv6.forward_bf16(1, T, C, H, state, *(d[x].unsqueeze(0) for x in ("r", "k", "v", "eew")), d["u"], want)
    one = torch.empty(1, T, C, device="cuda", dtype=bf)
    with ops.dispatch(split=0, tsplit=0):
        ops.rwkv6.forward_bf16(1, T, C, H, d["pool"][2:3].clone(), *(d[x].unsqueeze(0) for x in ("r", "k", "v", "eew")), d["u"], one)
    torch.cuda.synchronize()
    assert same(y, want[0]), (T, seg_len)
    assert not same(y, one[0]), "the dense call was not cut: the comparison shows nothing"
    # (the final state is a running state of the forward here and the chaining kernel's there: not bit-identical, held by test_oracle_parity)
    print(f"T {T} seg_len {seg_len}: final state against the dense two-level call {max_norm_err(host(pool[2]), host(state[0])):.2e}")


@pytest.mark.parametrize("seg_len", SEGS)
def test_oracle_parity(ops, oracle, seg_len):
    d, y_ref, _, counts, cs = reference(ops)
    want = oracle_states(oracle, d, SRC)
    pool = d["pool"].clone()
    y = split_call(ops, d, pool, i32(SRC), i32(DST), seg_len, 64, i32(cs), i32(SNAPS))
    torch.cuda.synchronize()
    c = d["cu"].tolist()
    for s, n in enumerate(L):
        if n == 0:
            continue
        rows = slice(c[s], c[s + 1])
        check(y[rows], want[(s, n)][0], bf, f"split {seg_len} seq {s} (len {n}) y")
        e = max_norm_err(host(pool[DST[s]]), want[(s, n)][1])
        print(f"split {seg_len} seq {s} (len {n}) final state: {e:.2e}")
        assert e <= STATE_TOL, (s, n, e)
        for j in range(counts[s]):
            e = max_norm_err(host(pool[SNAPS[cs[s] + j]]), want[(s, 64 * (j + 1))][1])
            print(f"split {seg_len} seq {s} (len {n}) snapshot at {64 * (j + 1)}: {e:.2e}")
            assert e <= STATE_TOL, (s, n, j, e)
        within_one_pass_bound(y[rows], y_ref[rows], f"split {seg_len} seq {s} (len {n})")


_FINALS = {}


def split_prefix_states(ops, d, seg_len):
    """{P: the pool the split call leaves, in place on SRC, when every sequence of P tokens and more is cut to P and the others to 0}."""
    if seg_len not in _FINALS:
        out = {}
        for P in (64, 128, 192, 256):
            p = d["pool"].clone()
            split_call(ops, cut(d, [P if n >= P else 0 for n in L]), p, i32(SRC), None, seg_len)
            out[P] = p
        torch.cuda.synchronize()
        _FINALS[seg_len] = out
    return _FINALS[seg_len]


@pytest.mark.parametrize("snap_every", [64, 128])
@pytest.mark.parametrize("seg_len", SEGS)
def test_snap_contract_under_splitting(ops, seg_len, snap_every):
    """Snapshot j is the final state of the same split call on the sequence cut to (j + 1) * snap_every tokens; one at the sequence's end
    equals the final state; snapshot and destination slots outside the pool store nothing (and stop nothing else)."""
    d = reference(ops)[0]
    finals = split_prefix_states(ops, d, seg_len)
    counts, cs = plan(L, snap_every)
    snap_slot = list(SNAPS[:cs[-1]])
    s257, s129 = L.index(257), L.index(129)
    skipped = [cs[s257] + 1, cs[s129]]                                    # a snapshot of a cut sequence each: no slot
    for i, bad in zip(skipped, (-1, N_SLOTS + 5)):
        snap_slot[i] = bad
    dst = list(DST)
    dst[L.index(200)], dst[L.index(65)] = N_SLOTS, -3                     # their final states go nowhere
    pool = d["pool"].clone()
    split_call(ops, d, pool, i32(SRC), i32(dst), seg_len, snap_every, i32(cs), i32(snap_slot))
    torch.cuda.synchronize()
    written = set()
    for s, n in enumerate(L):
        for j in range(counts[s]):
            p = snap_slot[cs[s] + j]
            if 0 <= p < N_SLOTS:
                assert same(pool[p], finals[(j + 1) * snap_every][SRC[s]]), (seg_len, snap_every, s, n, j, "snapshot")
                written.add(p)
                if (j + 1) * snap_every == n and 0 <= dst[s] < N_SLOTS:
                    assert same(pool[p], pool[dst[s]]), (seg_len, snap_every, s, n, "a snapshot at the end is the final state")
        if n > 0 and 0 <= dst[s] < N_SLOTS:
            written.add(dst[s])
    assert sum(1 for s, n in enumerate(L) if n and n % snap_every == 0 and 0 <= dst[s] < N_SLOTS) >= 1     # (128 at either snap_every)
    for p in range(N_SLOTS):
        if p not in written:
            assert same(pool[p], d["pool"][p]), (seg_len, snap_every, p, "untouched")


@pytest.mark.parametrize("seg_len", SEGS)
def test_fan_out_and_in_place(ops, seg_len):
    """Three cut sequences read slot 7 and write three destinations, a fourth is cut and in place on slot 9: the same sequences one per call."""
    lens, src, dst = [130, 200, 257, 150], [7, 7, 7, 9], [1, 20, 12, 9]
    d = make_init(lens, seed=33)
    pool = d["pool"].clone()
    y = split_call(ops, d, pool, i32(src), i32(dst), seg_len, 64, i32([0, 2, 2, 3, 3]), i32([25, 26, 27]))
    alone = d["pool"].clone()
    c = d["cu"].tolist()
    ys = []
    for s, n in enumerate(lens):
        one = cut(d, [n if t == s else 0 for t in range(len(lens))])
        granted = {0: [25, 26], 2: [27]}.get(s, [])
        cs1 = [0] * (s + 1) + [len(granted)] * (len(lens) - s)
        ys.append(split_call(ops, one, alone, i32(src), i32(dst), seg_len, 64, i32(cs1), i32(granted + [0])))
    torch.cuda.synchronize()
    for s in range(len(lens)):
        assert same(y[c[s]:c[s + 1]], ys[s]), (seg_len, s, "y")
    assert same(pool, alone), seg_len
    for p in range(N_SLOTS):
        if p not in dst + [25, 26, 27]:
            assert same(pool[p], d["pool"][p]), p                        # slot 7 among them


@pytest.mark.parametrize("seg_len", SEGS)
def test_nothing_else_is_touched(ops, seg_len):
    """A NaN-filled pool with guard slots on both sides and NaN-filled gap rows of the inputs: rows in front of cu[0], behind cu[n_seq], and
    what max_seqlen = 150 cuts off the 200-token sequence (mid-segment at either seg_len).  The same call on clean copies names what must
    come out; slots nobody names keep their bits; gap rows of y are +0; the uncut sequences equal the snap call."""
    lens, max_len, out = [70, 130, 0, 200, 64], 150, N_SLOTS + 5
    src, dst = [2, -1, 9, out, 4], [11, 13, 20, 15, out]
    snap_slot, cu_snap = [21, 22, 23, 24, 25, 26, -1, 27, 28, 29], [0, 3, 4, 6, 9, 1000]
    d = make_init(lens, seed=34, lead=3, tail=5)
    c = d["cu"].tolist()
    gaps = [slice(0, c[0]), slice(c[3] + max_len, c[4]), slice(c[5], d["total"])]
    assert [g.stop - g.start for g in gaps] == [3, 50, 5]
    clean_pool = d["pool"].clone()
    y_clean = split_call(ops, d, clean_pool, i32(src), i32(dst), seg_len, 64, i32(cu_snap), i32(snap_slot), max_seqlen=max_len)
    snap_pool = d["pool"].clone()
    y_snap = snap_call(ops, d, snap_pool, i32(src), i32(dst), 64, i32(cu_snap), i32(snap_slot), max_seqlen=max_len)
    for x in ("r", "k", "v", "eew"):
        for g in gaps:
            d[x][g] = float("nan")
    guard = 8
    buf = torch.full((guard + N_SLOTS + guard, H, 64, 64), float("nan"), device="cuda")
    pool = buf[guard:guard + N_SLOTS]
    for p in (2, 4):
        pool[p] = d["pool"][p]
    before = buf.clone()
    y = split_call(ops, d, pool, i32(src), i32(dst), seg_len, 64, i32(cu_snap), i32(snap_slot), max_seqlen=max_len)
    torch.cuda.synchronize()
    for g in gaps:
        assert not bool(bits(y[g]).any()), g                              # +0 bitwise
    live = torch.ones(d["total"], dtype=torch.bool, device="cuda")
    for g in gaps:
        live[g] = False
    assert bool(torch.isfinite(y[live].float()).all()) and same(y[live], y_clean[live])
    named = [11, 13, 15, 21, 24, 27, 29]                                  # (test_rwkv6_snap_gpu.py has the derivation)
    touched = torch.zeros(buf.shape[0], dtype=torch.bool, device="cuda")
    for p in named:
        assert bool(torch.isfinite(pool[p]).all()) and same(pool[p], clean_pool[p]), (seg_len, p)
        touched[guard + p] = True
    assert same(buf[~touched], before[~touched])
    uncut = [s for s, n in enumerate(lens) if 0 < min(n, max_len) <= seg_len]
    assert uncut == {64: [4], 128: [0, 4]}[seg_len]
    for s in uncut:
        assert same(y[c[s]:c[s + 1]], y_snap[c[s]:c[s + 1]]), (seg_len, s)
    if seg_len == 128:
        assert same(pool[11], snap_pool[11]) and same(pool[21], snap_pool[21])
    assert same(pool[29], snap_pool[29])


def test_many_items(ops, oracle):
    """300 sequences, 296 of 1 .. 40 tokens and 4 of 257 .. 640, seg_len = 64: the prefix sums of the item table pass the 256 preparation
    threads (two sequences per thread), and most of the grid's workgroups find no item."""
    long_at = {7: 257, 150: 640, 255: 300, 299: 448}
    lens = [long_at.get(i, 1 + (7 * i) % 40) for i in range(300)]
    assert sorted(set(lens) - set(long_at.values())) == list(range(1, 41))
    d = make_init(lens, seed=35, n_slots=300)
    pool = d["pool"].clone()
    y = split_call(ops, d, pool, None, None, 64)
    ref = d["pool"].clone()
    y_ref = snap_call(ops, d, ref, None, None)
    torch.cuda.synchronize()
    c = d["cu"].tolist()
    for s, n in enumerate(lens):
        rows = slice(c[s], c[s + 1])
        if s not in long_at:
            assert same(y[rows], y_ref[rows]) and same(pool[s], ref[s]), (s, n)
            continue
        yo, so = oracle_one(oracle, d, rows, d["pool"][s])
        check(y[rows], yo, bf, f"many items seq {s} (len {n}) y")
        e = max_norm_err(host(pool[s]), so)
        print(f"many items seq {s} (len {n}) final state: {e:.2e}")
        assert e <= STATE_TOL, (s, n, e)
        within_one_pass_bound(y[rows], y_ref[rows], f"many items seq {s} (len {n})")
        assert same(y[c[s]:c[s] + 64], y_ref[c[s]:c[s] + 64]), (s, n)


def test_a_split_prefill_replays_from_a_graph(ops):
    """One capture of the split call with a caller workspace (preparation, state pass, chaining, forward per item, scan launch for the window
    below 32: five launches on one stream, no parallel branch), replayed twice on fresh inputs."""
    lens, src, dst = [257, 64, 200, 20], [3, 9, 0, 5], [10, 11, 12, 13]
    counts, cs = plan(lens, 64)
    batches = [make_init(lens, seed=36 + i) for i in range(3)]
    ws = ops.new_rwkv6_varlen_split_workspace(sum(lens), len(lens), 64, C, H, "cuda")
    eager = []
    for d in batches:
        p = d["pool"].clone()
        eager.append((split_call(ops, d, p, i32(src), i32(dst), 64, 64, i32(cs), i32(range(20, 20 + cs[-1])), ws=ws), p))
    torch.cuda.synchronize()
    assert not same(eager[1][0], eager[2][0])
    d = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batches[0].items()}
    pool, y = d["pool"].clone(), torch.empty_like(d["r"])
    src_t, dst_t, cs_t, snap_t = i32(src), i32(dst), i32(cs), i32(range(20, 20 + cs[-1]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        split_call(ops, d, pool, src_t, dst_t, 64, 64, cs_t, snap_t, ws=ws, y=y)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            split_call(ops, d, pool, src_t, dst_t, 64, 64, cs_t, snap_t, ws=ws, y=y)
    torch.cuda.current_stream().wait_stream(side)
    for i in (1, 2):
        for x in ("r", "k", "v", "eew", "u"):
            d[x].copy_(batches[i][x])
        pool.copy_(batches[i]["pool"])
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same(y, eager[i][0]) and same(pool, eager[i][1]), i


def test_layer_level_seg_len():
    """infctx.tmix_forward_packed(seg_len=128) against seg_len=0 on a small Tmix_x060: outputs and WKV states within OP_TOL of
    tests/test_callers_gpu.py (the bound of test_layer_level_packed_serving_step), bitwise where nothing is cut; the shift tokens are copies."""
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import callers, infctx
    from test_callers_gpu import OP_TOL
    tm = callers.Tmix_x060(cw.N_EMBD, cw.DIM_ATT)
    tm.load_state_dict(cw.tmix_weights(torch.Generator().manual_seed(11), layer_id=1), strict=True)
    tm = tm.cuda().to(bf)
    E, heads, n_slots = cw.N_EMBD, tm.n_head, 16
    lens, src, out = [300, 64, 0, 129, 5], [4, 1, 6, 0, -1], [8, 9, 10, 11, 12]
    snap_slots, cu_snap = [13, 14, 15, 2, 3], [0, 2, 3, 3, 5, 5]
    g = torch.Generator().manual_seed(15)
    x = torch.randn(1, sum(lens), E, generator=g).cuda().to(bf)
    shift0 = torch.randn(n_slots, E, generator=g).to(bf).cuda()
    wkv0 = (torch.randn(n_slots, heads, 64, 64, generator=g) * 0.3).cuda()
    c = np.concatenate([[0], np.cumsum(lens)]).tolist()
    snap = (128, i32(cu_snap), i32(snap_slots))
    res = {}
    with torch.no_grad():
        for seg_len in (0, 128):
            shift_t, wkv_pool = shift0.clone(), wkv0.clone()
            att = infctx.tmix_forward_packed(tm, x, i32(c), max(lens), shift_t, wkv_pool, i32(src), out_slots=i32(out), snap=snap, seg_len=seg_len)
            res[seg_len] = (att, shift_t, wkv_pool)
    torch.cuda.synchronize()
    (a0, st0, wp0), (a1, st1, wp1) = res[0], res[128]
    assert same(st0, st1)
    assert not same(wp0, wp1) and not same(a0, a1), "nothing was cut: the comparison shows nothing"
    for s, n in enumerate(lens):
        if n == 0:
            continue
        rows = slice(c[s], c[s + 1])
        if n <= 128:
            assert same(a0[0, rows], a1[0, rows]) and same(wp0[out[s]], wp1[out[s]]), (s, n)
        e, es = max_norm_err(host(a1[0, rows]), host(a0[0, rows])), max_norm_err(host(wp1[out[s]]), host(wp0[out[s]]))
        print(f"time-mix seg_len 128 against 0, seq {s} (len {n}): out {e:.2e}, state {es:.2e}")
        assert e <= OP_TOL and es <= OP_TOL, (s, n, e, es)
    for p in (13, 14, 2):                                                 # 300: positions 128, 256; 129: position 128 (slot 3 stays)
        es = max_norm_err(host(wp1[p]), host(wp0[p]))
        assert es <= OP_TOL, (p, es)
    assert same(wp1[13], wp0[13]) and same(wp1[2], wp0[2])                # snapshots at position 128 = seg_len: inside the first segment
    for p in range(n_slots):
        if p not in (8, 9, 11, 12, 13, 14, 2):
            assert same(wp1[p], wkv0[p]) and same(st1[p], st0[p]), p
