"""Packed stateful inference on the GPU: wkv6_op.rwkv6.forward_varlen_bf16 / _fp16 / _fp32 (include/wkv6_amd.h: rwkv6_forward_varlen_*),
wkv.RUN_RWKV_6_VARLEN and infctx.tmix_forward_packed / cmix_forward_packed.

Contract: for every sequence of the packed batch, y and the state left in its slot of the pool equal BIT FOR BIT one dense
rwkv6.forward_<io>(B = 1, T = len, ...) call on that sequence alone with the slot's state.  Oracle tolerances are the suite's
(oracle/contract.py; `check` of tests/test_wkv6_gpu.py); final states F32_TOL where the exact scan served the sequence and 2e-4 where the
chunked kernel did (bf16, 32 tokens and more), the bound test_rwkv6_stateful_inference_kernel holds the dense op to."""
import numpy as np
import pytest
import torch

from conftest import max_norm_err
from oracle.contract import F32_TOL
from test_wkv6_gpu import check

pytestmark = pytest.mark.gpu
bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
IOS = {"bf16": bf, "fp16": f16, "fp32": f32}
LENS = [1, 1, 31, 32, 33, 64, 65, 130, 0, 1]        # both sides of the routing threshold and of a 64-token group, empty, decode tokens
H, C, N_SLOTS = 2, 128, 16
CHUNK_MIN = 32                                      # the dense op's rule: bf16 calls of T >= 32 take the chunked kernel


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "the gpu suite needs a GPU"
    from rwkv_lm_ext_amd import wkv6_op
    return wkv6_op


def host(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def make(lens, io, seed, heads=H, lead=0, tail=0, n_slots=N_SLOTS):
    """A packed batch in the I/O type: `lead` rows in front of the first sequence and `tail` rows behind the last belong to no sequence.
    w is the raw decay (bf16-representable, so that the oracle sees the same numbers), eew the fp32 decay the operator takes."""
    total, ch = lead + sum(lens) + tail, 64 * heads
    g = torch.Generator(device="cuda").manual_seed(seed)
    r, k, v = (torch.randn(total, ch, device="cuda", generator=g).mul_(0.5).to(bf).to(io) for _ in range(3))
    w = (-1 + 0.5 * torch.randn(total, ch, device="cuda", generator=g)).to(bf).float()
    u = (torch.randn(heads, 64, device="cuda", generator=g) * 0.3).to(bf).to(io)
    eew = torch.exp(-torch.exp(w)).contiguous()
    pool = torch.randn(n_slots, heads, 64, 64, device="cuda", generator=g) * 0.5
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]) + lead, dtype=torch.int32, device="cuda")
    return dict(r=r, k=k, v=v, w=w, eew=eew, u=u, pool=pool, cu=cu, lens=list(lens), H=heads, total=total, io=io,
                max_seqlen=max(max(lens), 1))


def packed(ops, d, pool, slot, algo=None, max_seqlen=None, ws=None, y=None):
    fn = {bf: ops.rwkv6.forward_varlen_bf16, f16: ops.rwkv6.forward_varlen_fp16, f32: ops.rwkv6.forward_varlen_fp32}[d["io"]]
    y = torch.full_like(d["r"], float("nan")) if y is None else y
    fn(d["total"], 64 * d["H"], d["H"], pool, slot, d["r"], d["k"], d["v"], d["eew"], d["u"], y, d["cu"],
       d["max_seqlen"] if max_seqlen is None else max_seqlen, algo=algo, ws=ws)
    return y


def dense(ops, d, rows, state, piece=None):
    """One dense rwkv6.forward_<io>(1, len, ...) call on rows `rows` from `state` ([H,N,N] fp32, updated in place).  piece: the call is made
    in pieces of that many tokens (pieces below 32 tokens run the exact scan whatever the I/O type; the fp32 state carries exactly)."""
    fn = {bf: ops.rwkv6.forward_bf16, f16: ops.rwkv6.forward_fp16, f32: ops.rwkv6.forward_fp32}[d["io"]]
    n, ch = rows.stop - rows.start, 64 * d["H"]
    ys = []
    for t0 in range(0, n, piece or n):
        t1 = min(n, t0 + (piece or n))
        sl = slice(rows.start + t0, rows.start + t1)
        y = torch.empty(1, t1 - t0, ch, device="cuda", dtype=d["io"])
        fn(1, t1 - t0, ch, d["H"], state, *(d[x][sl].unsqueeze(0).contiguous() for x in ("r", "k", "v", "eew")), d["u"], y)
        ys.append(y[0])
    return torch.cat(ys)


def rows_of(d, s):
    c = d["cu"].tolist()
    return slice(c[s], c[s + 1])


PERM = [5, 12, 0, 9, 3, 15, 7, 1, 10, 14]           # state_slot of the ten sequences: a permutation of a part of the 16 slots


@pytest.mark.parametrize("variant", ["routed", "algo_scan", "no_state_slot"])
@pytest.mark.parametrize("io", sorted(IOS))
def test_bit_identity_with_the_dense_op_per_sequence(ops, io, variant):
    d = make(LENS, IOS[io], seed=1)
    slots = list(range(len(LENS))) if variant == "no_state_slot" else PERM
    slot = None if variant == "no_state_slot" else torch.tensor(slots, dtype=torch.int32, device="cuda")
    pool = d["pool"].clone()
    y = packed(ops, d, pool, slot, algo="scan" if variant == "algo_scan" else None)
    torch.cuda.synchronize()
    for s, n in enumerate(LENS):
        if n == 0:
            assert same(pool[slots[s]], d["pool"][slots[s]]), (s, "an empty sequence leaves its slot alone")
            continue
        state = d["pool"][slots[s]].clone()
        want = dense(ops, d, rows_of(d, s), state, piece=31 if variant == "algo_scan" and d["io"] == bf else None)
        assert same(y[rows_of(d, s)], want), (io, variant, s, n, "y")
        assert same(pool[slots[s]], state), (io, variant, s, n, "state")
    named = set(slots)
    for p in range(N_SLOTS):
        if p not in named:
            assert same(pool[p], d["pool"][p]), p


def oracle_one(oracle, d, rows, s0):
    f = lambda t: host(t[rows])[None]
    y, so = oracle.forward(f(d["r"]), f(d["k"]), f(d["v"]), f(d["w"]), host(d["u"]), host(s0), return_state=True)
    return y[0], so.reshape(d["H"], 64, 64)


def state_tol(io, served_by_chunk):
    return 2e-4 if (io == bf and served_by_chunk) else F32_TOL


@pytest.mark.parametrize("io", ["bf16", "fp32"])
def test_oracle_parity(ops, oracle, io):
    d = make(LENS, IOS[io], seed=1)
    slot = torch.tensor(PERM, dtype=torch.int32, device="cuda")
    pool = d["pool"].clone()
    y = packed(ops, d, pool, slot)
    torch.cuda.synchronize()
    for s, n in enumerate(LENS):
        if n == 0:
            continue
        yo, so = oracle_one(oracle, d, rows_of(d, s), d["pool"][PERM[s]])
        check(y[rows_of(d, s)], yo, d["io"], f"packed rwkv6 {io} seq {s} (len {n}) y")
        e = max_norm_err(host(pool[PERM[s]]), so)
        print(f"packed rwkv6 {io} seq {s} (len {n}) state: {e:.2e}")
        assert e <= state_tol(d["io"], n >= CHUNK_MIN), (s, n, e)


@pytest.mark.parametrize("io", ["bf16", "fp32"])
def test_continuation_across_calls(ops, oracle, io):
    """Three sequences A, B, C in three calls: prefill of 70 / 5 / 33 tokens; one decode token each with the sequences in another order;
    then 4 more tokens of A and 40 more of C while B is absent.  The pieces and the pool equal the oracle on the whole sequences."""
    whole = {"A": 70 + 1 + 4, "B": 5 + 1, "C": 33 + 1 + 40}
    full = make([whole[n] for n in "ABC"], IOS[io], seed=2)
    start = dict(zip("ABC", full["cu"].tolist()[:3]))
    home = {"A": 3, "B": 0, "C": 7}
    pool = full["pool"].clone()
    got = {n: [] for n in "ABC"}
    done = {n: 0 for n in "ABC"}
    chunked = set()
    for step in ((("A", 70), ("B", 5), ("C", 33)), (("C", 1), ("A", 1), ("B", 1)), (("A", 4), ("C", 40))):
        idx = torch.cat([torch.arange(start[n] + done[n], start[n] + done[n] + m) for n, m in step]).cuda()
        d = dict(full, lens=[m for _, m in step], total=int(idx.numel()), max_seqlen=max(m for _, m in step),
                 cu=torch.tensor(np.concatenate([[0], np.cumsum([m for _, m in step])]), dtype=torch.int32, device="cuda"))
        for x in ("r", "k", "v", "eew"):
            d[x] = full[x][idx].contiguous()
        y = packed(ops, d, pool, torch.tensor([home[n] for n, _ in step], dtype=torch.int32, device="cuda"))
        t0 = 0
        for n, m in step:
            got[n].append(y[t0:t0 + m])
            t0 += m
            done[n] += m
            if m >= CHUNK_MIN:
                chunked.add(n)
    torch.cuda.synchronize()
    assert done == whole
    for i, n in enumerate("ABC"):
        yo, so = oracle_one(oracle, full, rows_of(full, i), full["pool"][home[n]])
        check(torch.cat(got[n]), yo, full["io"], f"continued {io} {n} y")
        e = max_norm_err(host(pool[home[n]]), so)
        print(f"continued {io} {n} state: {e:.2e}")
        assert e <= state_tol(full["io"], n in chunked), (n, e)


@pytest.mark.parametrize("io", sorted(IOS))
def test_nothing_else_is_touched(ops, io):
    """Gap rows (before cu[0], behind cu[n_seq], what max_seqlen cuts off) are +0 and never read; unnamed slots, the empty sequence's slot
    and the memory around the pool (a slot of -1 or n_slots + 5 would land there) keep their bits, NaN included."""
    lens, cut = [20, 50, 0, 35, 7], 40
    slots = [2, -1, 9, N_SLOTS + 5, 4]
    d = make(lens, IOS[io], seed=3, lead=3, tail=5)
    c = d["cu"].tolist()
    gaps = [slice(0, c[0]), slice(c[1] + cut, c[2]), slice(c[5], d["total"])]
    assert [g.stop - g.start for g in gaps] == [3, 10, 5]
    for x in ("r", "k", "v", "eew"):
        for g in gaps:
            d[x][g] = float("nan")
    guard = 8                                                            # slots of other memory on either side of the pool
    buf = torch.full((guard + N_SLOTS + guard, H, 64, 64), float("nan"), device="cuda")
    pool = buf[guard:guard + N_SLOTS]
    for p in (2, 4):
        pool[p] = d["pool"][p]
    before = buf.clone()
    y = packed(ops, d, pool, torch.tensor(slots, dtype=torch.int32, device="cuda"), max_seqlen=cut)
    torch.cuda.synchronize()
    for g in gaps:
        assert not bool(bits(y[g]).any()), g                              # +0 bitwise
    touched = torch.zeros(buf.shape[0], dtype=torch.bool, device="cuda")
    touched[[guard + 2, guard + 4]] = True
    assert same(buf[~touched], before[~touched])
    zero = torch.zeros(H, 64, 64, device="cuda")
    for s, state in ((0, d["pool"][2].clone()), (1, zero.clone()), (3, zero.clone()), (4, d["pool"][4].clone())):
        n = min(lens[s], cut)
        rows = slice(c[s], c[s] + n)
        want = dense(ops, d, rows, state)
        assert bool(torch.isfinite(y[rows]).all()) and same(y[rows], want), (io, s)
        if slots[s] in (2, 4):
            assert same(pool[slots[s]], state), (io, s)


@pytest.mark.parametrize("io", sorted(IOS))
def test_two_calls_are_bit_identical(ops, io):
    d = make(LENS, IOS[io], seed=4)
    slot = torch.tensor(PERM, dtype=torch.int32, device="cuda")
    p1, p2 = d["pool"].clone(), d["pool"].clone()
    y1, y2 = packed(ops, d, p1, slot), packed(ops, d, p2, slot)
    torch.cuda.synchronize()
    assert same(y1, y2) and same(p1, p2)


def test_a_decode_step_replays_from_a_graph(ops):
    """max_seqlen = 1, 8 sequences, caller-owned workspace: one preparation launch and one scan launch, a straight line."""
    n = 8
    d = make([1] * n, bf, seed=5)
    slot = torch.tensor([6, 1, 13, 4, 0, 9, 15, 2], dtype=torch.int32, device="cuda")
    ws = ops.new_rwkv6_varlen_workspace(n, "cuda")
    eager_pool, eager_y = d["pool"].clone(), []
    for _ in range(3):
        eager_y.append(packed(ops, d, eager_pool, slot, ws=ws).clone())
    torch.cuda.synchronize()
    assert not same(eager_y[0], eager_y[2])                              # the state moves from step to step
    pool, y = d["pool"].clone(), torch.empty_like(d["r"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        packed(ops, d, pool, slot, ws=ws, y=y)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            packed(ops, d, pool, slot, ws=ws, y=y)
    torch.cuda.current_stream().wait_stream(side)
    pool.copy_(d["pool"])
    for i in range(3):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same(y, eager_y[i]), i
    assert same(pool, eager_pool)


def test_many_workgroups(ops):
    """H = 32, C = 2048, 40 sequences (30 decode tokens, 10 prompts of 33..200 tokens): 1280 workgroups per launch, both routes."""
    long = [33, 50, 64, 65, 100, 127, 128, 129, 177, 200]
    lens = []
    for n in long:
        lens += [1, n, 1, 1]
    assert len(lens) == 40 and lens.count(1) == 30
    d = make(lens, bf, seed=6, heads=32, n_slots=48)
    perm = torch.randperm(48, generator=torch.Generator().manual_seed(7))[:40]
    pool = d["pool"].clone()
    y = packed(ops, d, pool, perm.to(torch.int32).cuda())
    torch.cuda.synchronize()
    for s in (0, 1, 22, 37, 39):                                        # lengths 1, 33, 1, 200, 1
        state = d["pool"][perm[s]].clone()
        want = dense(ops, d, rows_of(d, s), state)
        assert same(y[rows_of(d, s)], want) and same(pool[perm[s]], state), (s, lens[s])
    assert {lens[s] for s in (0, 1, 22, 37, 39)} == {1, 33, 200}


def test_layer_level_packed_serving_step():
    """infctx.tmix_forward_packed + cmix_forward_packed on four sequences, two of them continuing from earlier calls, against
    tmix_forward_infctx / cmix_forward_infctx per sequence with the same carried states.  Bound: OP_TOL of tests/test_callers_gpu.py, the
    rule of test_time_mix_module_on_a_packed_batch (the GEMMs around the operator see other shapes packed than alone); the carried tokens
    are copies and compare bitwise."""
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import callers, infctx
    from rwkv_lm_ext_amd.wkv import RUN_RWKV_6
    from test_callers_gpu import OP_TOL
    tm = callers.Tmix_x060(cw.N_EMBD, cw.DIM_ATT)
    tm.load_state_dict(cw.tmix_weights(torch.Generator().manual_seed(11), layer_id=1), strict=True)
    tm = tm.cuda().to(bf)
    cm = callers.CMix_x060(cw.N_EMBD, cw.DIM_FFN)
    cm.load_state_dict(cw.cmix_weights(torch.Generator().manual_seed(12)), strict=True)
    cm = cm.cuda().to(bf)
    E, heads = cw.N_EMBD, tm.n_head
    lens, slots, n_slots = [40, 1, 0, 70, 5], [4, 1, 6, 0, 5], 8
    g = torch.Generator().manual_seed(13)
    x = torch.randn(1, sum(lens), E, generator=g).cuda().to(bf)
    assert tm._use_fused(x) and cm._use_fused(x)
    shift_t, shift_c = (torch.zeros(n_slots, E, dtype=bf).cuda() for _ in range(2))
    wkv_pool = torch.zeros(n_slots, heads, 64, 64).cuda()
    for p in (1, 0):                                                     # sequences 1 and 3 continue; the others start fresh
        shift_t[p] = torch.randn(E, generator=g).to(bf).cuda()
        shift_c[p] = torch.randn(E, generator=g).to(bf).cuda()
        wkv_pool[p] = (torch.randn(heads, 64, 64, generator=g) * 0.3).cuda()
    for p in (2, 3, 6, 7):                                               # slots nobody names (6: an empty sequence's) keep what they hold
        shift_t[p], shift_c[p], wkv_pool[p] = 7.0, -3.0, 0.25
    before = (shift_t.clone(), shift_c.clone(), wkv_pool.clone())
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).cuda()
    slot = torch.tensor(slots, dtype=torch.int32).cuda()
    dense_wkv = lambda B, T, C_, H_, r, k, v, w, u, s: RUN_RWKV_6(B, T, C_, H_, s, *(t.contiguous() for t in (r, k, v, w)), u.to(r.dtype))
    with torch.no_grad():
        att = infctx.tmix_forward_packed(tm, x, cu, max(lens), shift_t, wkv_pool, slot)
        ffn = infctx.cmix_forward_packed(cm, x, cu, shift_c, slot)
        torch.cuda.synchronize()
        t0 = 0
        for s, n in enumerate(lens):
            p = slots[s]
            if n == 0:
                continue
            xs = x[:, t0:t0 + n].contiguous()
            want, st = infctx.tmix_forward_infctx(tm, xs, infctx.TimeMixState(before[0][p:p + 1], before[2][p:p + 1]), wkv_state=dense_wkv)
            e = max_norm_err(host(att[:, t0:t0 + n]), host(want))
            es = max_norm_err(host(wkv_pool[p]), host(st.wkv_state[0]))
            print(f"time-mix seq {s} (len {n}): out {e:.2e}, state {es:.2e}")
            assert e <= OP_TOL and es <= OP_TOL, (s, e, es)
            assert same(shift_t[p], st.shift_state[0]) and same(shift_t[p], x[0, t0 + n - 1])
            want, st = infctx.cmix_forward_infctx(cm, xs, infctx.ChannelMixState(before[1][p:p + 1]))
            e = max_norm_err(host(ffn[:, t0:t0 + n]), host(want))
            print(f"channel-mix seq {s} (len {n}): {e:.2e}")
            assert e <= OP_TOL, (s, e)
            assert same(shift_c[p], st.shift_state[0])
            t0 += n
    for p in (2, 3, 6, 7):
        assert same(shift_t[p], before[0][p]) and same(shift_c[p], before[1][p]) and same(wkv_pool[p], before[2][p]), p
