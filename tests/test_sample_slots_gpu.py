"""The device-side sampler on the GPU: rwkv6_sample_slots_* (include/wkv6_amd.h) through mix_op.sample_slots, infctx.sample_packed and
infctx.decode_step_packed, against the numpy oracle of tests/sample_numpy.py.

Integer results are compared exactly on the rows the oracle calls decisive (and the share of the others is bounded in
test_sample_slots_cpu.py).  Log-probabilities within 1e-5: the kernel's z, its difference to the maximum and the division by the temperature
are fp32 (3 roundings of 2^-24 relative on an exponent of at most ~30 in these rows: 5e-6), W is exact to 2^-46 per term.  The new occurrence
row is bit-equal to fp32 o * decay (+ 1)."""
import numpy as np
import pytest
import torch

import sample_numpy as sn

pytestmark = pytest.mark.gpu
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
NAN, INF = float("nan"), float("inf")


def i32(x):
    return torch.tensor([int(v) for v in x], dtype=torch.int32, device="cuda")


def ibits(t):
    return t.contiguous().view(torch.int32)


def call(logits, occ, params, u, dtype, ld=None, slots=None, out_slots=None):
    """logits [n_seq,V] and occ [n_slots,V] as fp32 numpy values; both are padded to ld with a sentinel the kernel must neither use nor
    change.  Returns (tokens, logprob, the pool after the call [n_slots,ld]) as numpy arrays."""
    from rwkv_lm_ext_amd import mix_op
    n_seq, V = logits.shape
    ld = (V + 7) // 8 * 8 if ld is None else ld
    lg = torch.full((n_seq, ld), 77.0, dtype=dtype, device="cuda")
    lg[:, :V] = torch.from_numpy(np.asarray(logits, np.float32)).to(dtype)
    pool = torch.full((occ.shape[0], ld), -5.0, device="cuda")
    pool[:, :V] = torch.from_numpy(np.asarray(occ, np.float32))
    tok, lp = mix_op.sample_slots(lg[:, :V], pool[:, :V], slots, torch.from_numpy(np.asarray(params, np.float32)).cuda().contiguous(),
                                  torch.tensor(np.asarray(u, np.float32)).cuda(), out_slots=out_slots, want_logprob=True)
    torch.cuda.synchronize()
    assert torch.equal(lg[:, V:], torch.full_like(lg[:, V:], 77.0)) and torch.equal(pool[:, V:], torch.full_like(pool[:, V:], -5.0))
    return tok.cpu().numpy(), lp.cpu().numpy(), pool.cpu().numpy()


# ---- 1. the oracle's decisive rows, exactly
@pytest.mark.parametrize("dname,V,ld,n_seq", sn.CASES)
def test_decisive_rows_match_the_oracle(dname, V, ld, n_seq):
    rows = sn.case_rows(dname, V, n_seq)
    logits, occ, params = (np.stack([r[i] for r in rows]) for i in range(3))
    u = np.array([r[3] for r in rows], np.float32)
    tok, lp, pool = call(logits, occ, params, u, DTYPES[dname], ld=ld)
    for s, r in enumerate(rows):
        want = sn.sample_row(*r)
        print(dname, V, n_seq, s, "decisive" if want["decisive"] else "open", tok[s], want["token"], lp[s], want["logprob"])
        if not want["decisive"]:
            continue
        assert tok[s] == want["token"], (s, r[2], r[3])
        assert abs(lp[s] - want["logprob"]) <= 1e-5, (s, lp[s], want["logprob"])
        assert np.array_equal(pool[s, :V].view(np.int32), want["occ"].view(np.int32)), s


# ---- 2. ties: rows where u sweeps every kept token -- the drawn set is the oracle's kept set
def sweep(logits, o, params, dtype, grid=64):
    """The set of tokens the kernel draws for u at the middle of every kept token's CDF interval and on a uniform grid, and the oracle's
    kept set."""
    V = logits.shape[0]
    ref = sn.sample_row(logits, o, params, 0.5)
    kept = np.nonzero(ref["kept"])[0]
    z2 = sn.repeat_penalised(sn.penalised(logits, o, params[3], params[4]), o, params[6]).astype(np.float64)
    w = np.where(ref["kept"], np.exp((z2 - z2[kept].max()) / params[0]), 0.0)
    cdf = np.cumsum(w) / w.sum()
    mids = (cdf[kept] - 0.5 * w[kept] / w.sum())
    u = np.concatenate([mids, (np.arange(grid) + 0.5) / grid, [0.0, 1 - 2.0 ** -24]]).astype(np.float32)
    n = u.size
    tok, _, _ = call(np.repeat(logits[None], n, 0), np.repeat(o[None], n, 0), np.repeat(params[None], n, 0), u, dtype)
    return set(tok.tolist()), set(kept.tolist()), tok[:kept.size], kept


def tie_row(V, n_top, n_tied, n_low, rng):
    """n_top tokens at 2, n_tied at 1, n_low at 0 (exact in bf16), the rest at -30, at random ids."""
    ids = rng.permutation(V)[:n_top + n_tied + n_low]
    logits = np.full(V, -30.0, np.float32)
    logits[ids[:n_top]], logits[ids[n_top:n_top + n_tied]], logits[ids[n_top + n_tied:]] = 2.0, 1.0, 0.0
    return logits, np.sort(ids[:n_top]), np.sort(ids[n_top:n_top + n_tied])


@pytest.mark.parametrize("V,n_top,n_tied,n_low", [(64, 2, 4, 3), (997, 3, 40, 20), (65536, 2, 300, 50)])
def test_ties_that_straddle_the_nucleus_cutoff_are_all_kept(V, n_top, n_tied, n_low):
    rng = np.random.default_rng(V)
    logits, top, tied = tie_row(V, n_top, n_tied, n_low, rng)
    p = np.exp(logits.astype(np.float64))
    p /= p.sum()
    top_p = p[top].sum() + 0.4 * p[tied].sum()             # the cutoff falls inside the tied group
    params = np.array([1.0, top_p, 0, 0, 0, 1, 1, 0], np.float32)
    drawn, kept, _, _ = sweep(logits, np.zeros(V, np.float32), params, torch.bfloat16)
    assert kept == set(top.tolist()) | set(tied.tolist())
    assert drawn == kept


@pytest.mark.parametrize("V,n_top,n_tied,n_low,k", [(64, 2, 4, 3, 4), (997, 3, 40, 20, 24), (65536, 2, 300, 50, 151), (65536, 2, 300, 50, 302)])
def test_ties_that_straddle_the_top_k_boundary_keep_the_lowest_ids(V, n_top, n_tied, n_low, k):
    rng = np.random.default_rng(V + k)
    logits, top, tied = tie_row(V, n_top, n_tied, n_low, rng)
    params = np.array([1.0, 1.0, k, 0, 0, 1, 1, 0], np.float32)
    drawn, kept, at_mids, kept_ids = sweep(logits, np.zeros(V, np.float32), params, torch.bfloat16)
    assert kept == set(top.tolist()) | set(tied[:k - n_top].tolist())
    assert drawn == kept
    assert np.array_equal(at_mids, kept_ids)               # and u in the middle of a token's interval draws that token


def test_top_k_and_top_p_together_keep_the_intersection():
    V = 997
    rng = np.random.default_rng(5)
    logits = sn.round_to(rng.permutation(V).astype(np.float32) * -0.05, torch.float32)
    for top_p, k, n_kept in ((0.9, 5, 5), (0.3, 20, None)):
        params = np.array([1.0, top_p, k, 0, 0, 1, 1, 0], np.float32)
        drawn, kept, _, _ = sweep(logits, np.zeros(V, np.float32), params, torch.float32)
        assert drawn == kept and len(kept) <= k
        if n_kept is None:
            assert len(kept) < k                           # the nucleus is the smaller set here
        else:
            assert len(kept) == n_kept


# ---- 3. dense rows: the oracle's fp64 CDF brackets u at the returned token
@pytest.mark.parametrize("dname", list(DTYPES))
def test_dense_rows_draw_where_the_fp64_cdf_brackets_u(dname):
    """randn logits at V = 65536, top_p = 1, top_k = 0.  eps: the bound of fp32 lane partials of 64 terms plus a 1024-way tree (80 * 2^-24 = 5e-6, taken
    four times); this kernel's integer sums stay far inside it (65536 * 2^-46 of the largest weight)."""
    V, n_seq, eps = 65536, 3, 2e-5
    rng = np.random.default_rng(11)
    logits = sn.round_to(rng.standard_normal((n_seq, V)), DTYPES[dname])
    params = np.tile(np.array([1.0, 1.0, 0, 0, 0, 1, 1, 0], np.float32), (n_seq, 1))
    params[1, 0], params[2, 0] = 0.7, 1.5
    u = np.array([0.03, 0.5, 0.97], np.float32)
    tok, lp, _ = call(logits, np.zeros((n_seq, V), np.float32), params, u, DTYPES[dname])
    for s in range(n_seq):
        z = logits[s].astype(np.float64)
        w = np.exp((z - z.max()) / params[s, 0])
        cdf = np.cumsum(w) / w.sum()
        t = int(tok[s])
        lo, hi = cdf[t] - w[t] / w.sum(), cdf[t]
        print(dname, s, t, lo, float(u[s]), hi, lp[s], np.log(w[t] / w.sum()))
        assert 0 <= t < V and lo - eps <= u[s] <= hi + eps, (s, t, lo, u[s], hi)
        assert abs(lp[s] - np.log(w[t] / w.sum())) <= 1e-5


# ---- 4. top-k alone
def test_top_k_alone_draws_exactly_the_k_largest():
    V, k = 65536, 50
    rng = np.random.default_rng(13)
    logits = (rng.permutation(V).astype(np.float32) * np.float32(2.0 ** -12)).astype(np.float32)       # distinct, 16 apart at most
    params = np.array([1.0, 1.0, k, 0, 0, 1, 1, 0], np.float32)
    drawn, kept, _, _ = sweep(logits, np.zeros(V, np.float32), params, torch.float32, grid=128)
    assert kept == set(np.argsort(-logits.astype(np.float64), kind="stable")[:k].tolist())           # compared on z, not on p
    assert drawn == kept


# ---- 5. greedy
def test_greedy_is_the_exact_argmax_with_the_lowest_id_on_ties_and_penalties_move_it():
    V = 50277
    rng = np.random.default_rng(17)
    logits = sn.round_to(rng.standard_normal((4, V)), torch.bfloat16)
    best = logits.max() + 1.0
    logits[1, [40000, 77, 50276]] = best                   # a tie: the lowest id wins
    logits[2, 123], logits[2, 456] = best, best - 0.25      # 123 has occurred: presence + frequency push it under 456
    logits[3, 9], logits[3, 10] = best, best - 0.25         # ... and here the repetition penalty alone does
    occ = np.zeros((4, V), np.float32)
    occ[2, 123], occ[3, 9] = 2.0, 1.0
    logits = sn.round_to(logits, torch.bfloat16)
    params = np.tile(np.array([0.0, 0.5, 7, 0, 0, 0.5, 1, 0], np.float32), (4, 1))
    params[2, 3:5] = 0.1, 0.1
    params[3, 6] = 1.5
    tok, lp, pool = call(logits, occ, params, np.zeros(4, np.float32), torch.bfloat16)
    assert tok.tolist() == [int(np.argmax(logits[0])), 77, 456, 10]
    assert [sn.sample_row(logits[s], occ[s], params[s], 0.0)["token"] for s in range(4)] == tok.tolist()
    assert lp.tolist() == [0.0] * 4
    assert pool[2, 123] == 1.0 and pool[2, 456] == 1.0 and pool[3, 9] == 0.5 and pool[3, 10] == 1.0


# ---- 6. slots
def test_slots_fan_out_in_place_and_outside_the_pool():
    V, ld, n_slots = 997, 1000, 7
    rng = np.random.default_rng(19)
    rows = [sn.make_case(rng, V, torch.float32) for _ in range(6)]
    logits, params = np.stack([r[0] for r in rows]), np.stack([r[2] for r in rows])
    u = np.array([r[3] for r in rows], np.float32)
    occ = np.zeros((n_slots, V), np.float32)
    for p in range(n_slots):
        occ[p, rng.permutation(V)[:9]] = rng.choice([0.5, 1.0, 2.0], 9)
    # sequences 0-2 fan out of slot 5 into 0, 1, 2; 3 is in place on slot 3; 4 reads outside the pool and writes 6; 5 reads 4, writes outside
    src, dst = [5, 5, 5, 3, -1, 4], [0, 1, 2, 3, 6, n_slots]
    tok, lp, pool = call(logits, occ, params, u, torch.float32, ld=ld, slots=i32(src), out_slots=i32(dst))
    for s in range(6):
        o = occ[src[s]] if 0 <= src[s] < n_slots else np.zeros(V, np.float32)
        want = sn.sample_row(logits[s], o, params[s], u[s])
        if want["decisive"]:
            assert tok[s] == want["token"] and abs(lp[s] - want["logprob"]) <= 1e-5, s
        if 0 <= dst[s] < n_slots:
            mine = (o * np.float32(params[s, 5])).astype(np.float32)
            mine[tok[s]] += np.float32(1)
            assert np.array_equal(pool[dst[s], :V].view(np.int32), mine.view(np.int32)), s
    for p in (4, 5):                                        # only read
        assert np.array_equal(pool[p, :V].view(np.int32), occ[p].view(np.int32)), p
    # NULL slots: sequence s on row s, in place; the rows behind n_seq keep their bits
    tok2, _, pool2 = call(logits[:3], occ, params[:3], u[:3], torch.float32, ld=ld)
    for s in range(3):
        mine = (occ[s] * np.float32(params[s, 5])).astype(np.float32)
        mine[tok2[s]] += np.float32(1)
        assert np.array_equal(pool2[s, :V].view(np.int32), mine.view(np.int32)), s
    assert np.array_equal(pool2[3:, :V].view(np.int32), occ[3:].view(np.int32))


# ---- 7. poisoned rows
def test_poisoned_rows_give_minus_one_and_nan_and_leave_everything_else_alone():
    V, n = 50277, 7
    rng = np.random.default_rng(23)
    rows = [sn.make_case(rng, V, torch.bfloat16) for _ in range(n)]
    logits, occ, params = (np.stack([r[i] for r in rows]) for i in range(3))
    u = np.array([r[3] for r in rows], np.float32)
    clean = call(logits, occ, params, u, torch.bfloat16)
    logits[1, 31337] = NAN
    logits[3, :] = -INF
    params[5, 0] = -1.0
    params[6, 4] = INF
    tok, lp, pool = call(logits, occ, params, u, torch.bfloat16)
    for s in (1, 3, 5, 6):
        assert tok[s] == -1 and np.isnan(lp[s]), s
        assert np.array_equal(pool[s, :V].view(np.int32), occ[s].view(np.int32)), s
        assert sn.sample_row(logits[s], occ[s], params[s], u[s])["poisoned"]
    for s in (0, 2, 4):
        assert tok[s] == clean[0][s] and lp[s].view(np.int32) == clean[1][s].view(np.int32), s
        assert np.array_equal(pool[s].view(np.int32), clean[2][s].view(np.int32)), s


def test_banned_tokens_are_never_drawn():
    V = 64
    logits = np.full(V, -INF, np.float32)
    logits[[5, 9]] = 0.0, -1.0
    params = np.array([1.0, 1.0, 0, 0, 0, 1, 1, 0], np.float32)
    drawn, kept, _, _ = sweep(logits, np.zeros(V, np.float32), params, torch.float32)
    assert drawn == {5, 9}


# ---- 8. determinism
def test_the_same_call_twice_gives_the_same_bits():
    V, n = 65536, 5
    rng = np.random.default_rng(29)
    logits = sn.round_to(rng.standard_normal((n, V)) * 2, torch.bfloat16)
    occ = (rng.random((n, V)) < 0.01).astype(np.float32) * 1.5
    params = np.tile(np.array([0.9, 0.85, 0, 0.3, 0.2, 0.996, 1.1, 0], np.float32), (n, 1))
    params[1, 2], params[2, 1], params[3, 0] = 50, 1.0, 0.0
    u = rng.random(n).astype(np.float32)
    a, b = call(logits, occ, params, u, torch.bfloat16), call(logits, occ, params, u, torch.bfloat16)
    assert np.array_equal(a[0], b[0]) and (a[0] >= 0).all()
    assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32)) and np.array_equal(a[2].view(np.int32), b[2].view(np.int32))


def test_sample_packed_chooses_the_kernel_and_equals_the_eager_restatement():
    from rwkv_lm_ext_amd import infctx
    V, ld, n = 997, 1000, 9
    rng = np.random.default_rng(31)
    rows = [sn.make_case(rng, V, torch.bfloat16) for _ in range(n)]
    lg = torch.zeros(n, ld, dtype=torch.bfloat16, device="cuda")
    lg[:, :V] = torch.from_numpy(np.stack([r[0] for r in rows])).to(torch.bfloat16)
    params, u = torch.from_numpy(np.stack([r[2] for r in rows])).cuda(), torch.tensor([r[3] for r in rows]).cuda()
    pools = [infctx.SamplingPool.create(n, V, "cuda", ld=ld) for _ in range(3)]
    for p in pools:
        p.occ[:, :V] = torch.from_numpy(np.stack([r[1] for r in rows]))
    out = [infctx.sample_packed(lg, p, None, params, u, kernels=k) for p, k in zip(pools, (None, True, False))]
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(ibits(out[0][1]), ibits(out[1][1])) and torch.equal(pools[0].occ, pools[1].occ)
    decisive = torch.tensor([sn.sample_row(*r)["decisive"] for r in rows]).cuda()
    assert torch.equal(out[0][0][decisive], out[2][0][decisive])
    assert torch.allclose(out[0][1][decisive], out[2][1][decisive], atol=1e-5, rtol=0)
    assert torch.equal(pools[0].occ[decisive], pools[2].occ[decisive])
    with pytest.raises(RuntimeError, match="ld"):          # a head that is not padded: the kernel cannot serve it, and True says so
        infctx.sample_packed(lg[:, :V].contiguous(), infctx.SamplingPool.create(n, V, "cuda", ld=ld), None, params, u, kernels=True)


# ---- 9. the closed loop
def test_decode_step_packed_replays_from_a_graph():
    """emb -> two blocks -> ln_out -> head -> sample, captured once; tokens and u are refilled in place and the graph replayed four times: the
    replays equal four eager steps in tokens and in all four pools, bit for bit."""
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import infctx
    from test_packed_shift_gpu import two_blocks
    bf = torch.bfloat16
    blocks = two_blocks()
    E, heads, V, n_seq, n_slots, steps = cw.N_EMBD, cw.DIM_ATT // 64, 512, 5, 8, 4
    g = torch.Generator().manual_seed(91)
    emb = torch.nn.Embedding(V, E).cuda().to(bf)
    ln_out = torch.nn.LayerNorm(E).cuda().to(bf)
    head = torch.nn.Linear(E, V, bias=False).cuda().to(bf)
    with torch.no_grad():
        emb.weight.copy_(torch.randn(V, E, generator=g))
        head.weight.copy_(torch.randn(V, E, generator=g) * 0.2)
    slots, cu = i32([4, 1, 6, 0, 3]), i32(range(n_seq + 1))
    params = infctx.sampling_params(n_seq, "cuda", temperature=1.0, top_p=0.9, alpha_presence=0.3, alpha_frequency=0.3, alpha_decay=0.996)
    params[1, 2], params[2, 0], params[3, 6] = 20, 0.0, 1.2          # one sequence on top-k, one greedy, one with a repetition penalty
    start = torch.randint(0, V, (n_seq,), generator=g).int().cuda()
    draws = torch.rand(steps + 1, n_seq, generator=g).cuda()
    fields = ("shift_att", "shift_ffn", "wkv")

    def fresh():
        return infctx.PackedPools.create(2, n_slots, E, heads, "cuda", bf), infctx.SamplingPool.create(n_slots, V, "cuda")

    def step(tokens, u, pools, spool):
        return infctx.decode_step_packed(emb, blocks, ln_out, head, tokens, pools, spool, slots, params, u, cu, pool_kernels=True, kernels=True)

    with torch.no_grad():
        pools, spool = fresh()
        tokens, eager = start.clone(), []
        for i in range(steps):
            tokens = step(tokens, draws[i + 1], pools, spool)
            eager.append(tokens.clone())
        torch.cuda.synchronize()
        assert all((t >= 0).all() and (t < V).all() for t in eager)
        gpools, gspool = fresh()
        tokens, u = start.clone(), draws[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            warm = fresh()
            step(tokens, u, *warm)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                new = step(tokens, u, gpools, gspool)
        torch.cuda.current_stream().wait_stream(side)
        for t in (gpools.shift_att, gpools.shift_ffn, gpools.wkv, gspool.occ):
            t.zero_()
        for i in range(steps):
            u.copy_(draws[i + 1])
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(new, eager[i]), i
            tokens.copy_(new)
    assert all(torch.equal(getattr(gpools, f).view(torch.int16 if getattr(gpools, f).dtype == bf else torch.int32),
                           getattr(pools, f).view(torch.int16 if getattr(pools, f).dtype == bf else torch.int32)) for f in fields)
    assert torch.equal(ibits(gspool.occ), ibits(spool.occ)) and spool.occ.sum() > 0
