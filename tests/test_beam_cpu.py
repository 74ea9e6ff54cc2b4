"""CPU tier of the beam search on the packed serving step (infctx.beam_candidates, BeamSearch, beam_advance, beam_step_packed, beam_finalize):
the eager restatement of the candidate selection agrees with the fp64 oracle of tests/beam_numpy.py on CPU tensors; beam_advance agrees
with a plain Python restatement (eos routing, eviction, the done rule, the slot halves alternating, dead rows staying dead); a whole search
on a tiny model (C = 128, H = 2, 2 layers, V = 264; W = 3, 2 requests, 12 steps) agrees with a brute-force Python beam search that keeps
explicit sequences and a state slot of its own per beam, which also checks the backtracking of beam_finalize.

The WKV operator has no CPU path, so the searches run with a few-line torch stand-in for the one-token-per-sequence call (both sides use
it: what is compared is the search, not the operator)."""
import numpy as np
import pytest
import torch

import beam_numpy as bn

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
i32 = lambda v: torch.tensor(list(v), dtype=torch.int32)


# ---- 1. the eager restatement against the oracle
def eager(d, K, dname, ld=None):
    from rwkv_lm_ext_amd import infctx
    n_rows, V = d["logits"].shape
    ld = (V + 7) // 8 * 8 if ld is None else ld
    lg = torch.full((n_rows, ld), 77.0, dtype=DTYPES[dname])
    lg[:, :V] = torch.from_numpy(d["logits"]).to(DTYPES[dname])
    pool = slots = penalty = None
    if d["occ"] is not None:
        pool = infctx.SamplingPool.create(d["occ"].shape[0], V, "cpu", ld=ld)
        pool.occ.fill_(5.0)
        pool.occ[:, :V] = torch.from_numpy(d["occ"])
        slots = None if d["slot"] is None else torch.from_numpy(d["slot"])
        penalty = torch.from_numpy(d["penalty"])
    parent, token, score = infctx.beam_candidates(lg, torch.from_numpy(d["cum"]), torch.from_numpy(d["cu"]), K, pool=pool, slots=slots,
                                                  penalty=penalty, vocab=V, kernels=False)
    assert parent.dtype == torch.int32 and token.dtype == torch.int32 and score.dtype == torch.float32
    assert tuple(parent.shape) == tuple(token.shape) == tuple(score.shape) == (len(d["cu"]) - 1, K)
    return parent.numpy(), token.numpy(), score.numpy()


CU = {"one": [0, 1], "three": [0, 3], "empty+one": [0, 0, 1], "uneven": [0, 2, 2, 7], "sixty-four": [0, 64], "seventy": [0, 70, 71]}


@pytest.mark.parametrize("V,cu", [(V, cu) for V in (1, 7, 9, 1000) for cu in CU if V < 1000 or CU[cu][-1] < 64])      # large groups: small V
@pytest.mark.parametrize("penalty", [False, True])
def test_eager_restatement_matches_the_oracle(V, cu, penalty):
    for K, dname in ((1, "bf16"), (5, "fp32"), (64, "bf16")):
        d = bn.make_inputs(V + K + len(cu), CU[cu], V, dname, penalty=penalty)
        got = eager(d, K, dname)
        bn.check_band(bn.oracle_of(d, K), *got, K, exact=dname == "fp32")


def test_eager_ties_dead_and_poisoned_rows():
    V, K = 40, 12
    rng = np.random.default_rng(5)
    z = rng.integers(-3, 2, V).astype(np.float32)                       # heavy ties, on a grid that survives every rounding here
    # one row: (z descending, id ascending)
    d = dict(logits=z[None], cum=np.zeros(1, np.float32), cu=np.array([0, 1], np.int32), occ=None, slot=None, penalty=None)
    p, t, s = eager(d, K, "fp32")
    assert t[0].tolist() == np.lexsort((np.arange(V), -z))[:K].tolist() and (p == 0).all()
    # identical rows with equal cum: by row, then token; with widely separated cum: the best row first
    for cum, rows in (([-1.0, -1.0, -1.0], [0, 1, 2]), ([-1024.0, 0.0, -512.0], [1, 2, 0])):
        d = dict(logits=np.stack([z] * 3), cum=np.array(cum, np.float32), cu=np.array([0, 3], np.int32), occ=None, slot=None, penalty=None)
        want = bn.oracle_of(d, K)
        p, t, s = eager(d, K, "fp32")
        assert p.tolist() == want["parent"].tolist() and t.tolist() == want["token"].tolist()
        if cum[0] != cum[1]:
            assert (p[0] == rows[0]).all()
    # -inf logits, fewer than K candidates, a dead row full of NaN, a poisoned row beside a healthy one
    lg = rng.normal(0, 2, (5, V)).astype(np.float32)
    lg[0, 5:] = -np.inf
    lg[1] = np.nan
    lg[2, 3] = np.inf
    lg[3] = -np.inf
    d = dict(logits=lg, cum=np.array([-1, -np.inf, -2, -3, -4], np.float32), cu=np.array([0, 2, 4, 5], np.int32), occ=None, slot=None, penalty=None)
    want = bn.oracle_of(d, K)
    p, t, s = eager(d, K, "fp32")
    bn.check_band(want, p, t, s, K, exact=True)
    assert (p[0, :5] == 0).all() and sorted(t[0, :5].tolist()) == [0, 1, 2, 3, 4] and (p[0, 5:] == -1).all() and (p[1] == -1).all()
    alone = eager(dict(d, logits=lg[4:], cum=d["cum"][4:], cu=np.array([0, 1], np.int32)), K, "fp32")
    assert np.array_equal(alone[1][0], t[2]) and np.array_equal(alone[2][0].view(np.int32), s[2].view(np.int32))
    for bad in (np.nan, np.inf):
        q = eager(dict(d, cum=np.array([-1, -np.inf, -2, -3, bad], np.float32)), K, "fp32")
        assert (q[0][2] == -1).all() and np.array_equal(q[1][0], t[0])


# ---- 2. beam_advance against a plain Python restatement
def f32pow(n, lp):
    return float(torch.tensor(float(n)) ** lp)


def advance_py(s, parent, token, score):
    """`s`: a dict of lists with the fields of BeamSearch; the candidates as lists [n_groups][K]"""
    G, W, K, t = s["G"], s["W"], s["K"], s["step"]
    length = np.float32(f32pow(t + 1, s["lp"]))
    nxt_tok, nxt_cum, nxt_par, alive = [], [], [], []
    for g in range(G):
        cont = []
        for rank in range(K):
            if parent[g][rank] < 0:
                continue
            if token[g][rank] in s["eos"]:
                if rank < W:
                    hs = float(np.float32(score[g][rank]) / length)
                    table = s["hyp"][g]
                    if len(table) < W or hs > table[-1][0]:
                        table.append((hs, t, parent[g][rank]))
                        table.sort(key=lambda e: -e[0])              # stable: of equal scores the older one stays in front
                        del table[W:]
            elif len(cont) < W:
                cont.append(rank)
        best = score[g][0] if parent[g][0] >= 0 else -np.inf
        table = s["hyp"][g]
        s["done"][g] = s["done"][g] or (len(table) == W and table[-1][0] >= float(np.float32(best) / length))
        for j in range(W):
            have = j < len(cont)
            ok = have and not s["done"][g]
            nxt_par.append(parent[g][cont[j]] if have else g * W)
            nxt_tok.append(token[g][cont[j]] if have else 0)
            nxt_cum.append(float(np.float32(score[g][cont[j]])) if ok else -np.inf)
            alive.append(ok)
    s["hist_parent"].append(list(nxt_par))
    s["hist_token"].append([tk if a else -1 for tk, a in zip(nxt_tok, alive)])
    s["slots_in"] = [s["slots_out"][p] for p in nxt_par]
    s["slots_out"] = [s["base"] + 2 * W * (r // W) + W * ((t + 1) % 2) + r % W for r in range(G * W)]
    s["tokens"], s["cum"], s["step"] = nxt_tok, nxt_cum, t + 1


def state_py(st, prompt):
    G, W = st.n_groups, st.W
    return dict(G=G, W=W, K=st.K, step=0, lp=st.length_penalty, eos=set(st.eos_ids.tolist()), base=st.slot_base, hyp=[[] for _ in range(G)],
                done=[False] * G, hist_parent=[], hist_token=[], tokens=st.tokens.tolist(), cum=st.cum.tolist(),
                slots_in=[prompt[r // W] for r in range(G * W)], slots_out=st.slots_out.tolist())


def same_state(st, s):
    G, W, t = s["G"], s["W"], s["step"]
    assert int(st.step) == t
    assert st.tokens.tolist() == s["tokens"] and st.cum.tolist() == s["cum"], t
    assert st.slots_in.tolist() == s["slots_in"] and st.slots_out.tolist() == s["slots_out"] and st.slots_occ.tolist() == s["slots_out" if t else "slots_in"], t
    assert st.done.tolist() == s["done"], t
    assert st.hist_parent[:t].tolist() == s["hist_parent"] and st.hist_token[:t].tolist() == s["hist_token"], t
    for g in range(G):
        n = len(s["hyp"][g])
        assert st.hyp_score[g, :n].tolist() == [float(np.float32(e[0])) for e in s["hyp"][g]] and (st.hyp_score[g, n:] == -np.inf).all(), (t, g)
        assert st.hyp_step[g, :n].tolist() == [e[1] for e in s["hyp"][g]] and st.hyp_row[g, :n].tolist() == [e[2] for e in s["hyp"][g]], (t, g)


@pytest.mark.parametrize("W,eos,lp", [(3, (0, 1), 0.5), (2, (7,), 1.0), (4, (), 0.0), (1, (0, 1, 2), 2.0)])
def test_beam_advance_matches_the_python_restatement(W, eos, lp):
    from rwkv_lm_ext_amd import infctx
    G, T, base, prompt = 3, 14, 10, [3, 5, 4]
    rng = np.random.default_rng(W)
    st = infctx.BeamSearch.create(G, W, T, eos, lp, 1.0, [9, 8, 7], prompt, base, "cpu")
    K = st.K
    assert K == (1 + len(eos)) * W and st.cum.view(G, W)[:, 0].tolist() == [0.0] * G and (st.cum.view(G, W)[:, 1:] == -np.inf).all()
    assert st.slots_in.tolist() == [p for p in prompt for _ in range(W)] and st.tokens.tolist() == [t for t in (9, 8, 7) for _ in range(W)]
    s = state_py(st, prompt)
    same_state(st, s)
    for t in range(T):
        parent, token, score = np.full((G, K), -1), np.full((G, K), -1), np.full((G, K), -np.inf, np.float32)
        for g in range(G):
            live = [r for r in range(g * W, g * W + W) if s["cum"][r] > -np.inf]
            if not live:
                continue
            n = K if not (g == 2 and t % 5 == 4) else int(rng.integers(0, W + 1))     # now and then a request finds fewer than W
            parent[g, :n] = rng.choice(live, n)
            token[g, :n] = rng.integers(0, 12, n)                                      # eos ids come up often
            base_score = max(s["cum"][r] for r in live)
            score[g, :n] = np.sort((base_score - rng.uniform(0, 1.5, n) * (1 + 0.2 * rng.integers(0, 3, n))).astype(np.float32))[::-1]
        advance_py(s, parent.tolist(), token.tolist(), score.tolist())
        infctx.beam_advance(st, torch.from_numpy(parent).int(), torch.from_numpy(token).int(), torch.from_numpy(score))
        same_state(st, s)
        for g in range(G):                                                             # a done request's rows are dead and stay dead
            if s["done"][g]:
                assert all(c == -np.inf for c in s["cum"][g * W:g * W + W])
        half = (t + 1) % 2                                                             # the halves alternate; children read the other one
        assert all((so - base) % (2 * W) // W == half for so in s["slots_out"])
        assert all((si - base) % (2 * W) // W == 1 - half for si in s["slots_in"])
    with pytest.raises(RuntimeError, match="must be"):
        infctx.beam_advance(st, torch.zeros(G, K + 1).int(), torch.zeros(G, K + 1).int(), torch.zeros(G, K + 1))
    for bad in (dict(W=3, eos=(0, 1), K=8), dict(W=33, eos=(0,), K=None), dict(W=3, eos=(0,), K=65)):
        with pytest.raises(ValueError):
            infctx.BeamSearch.create(1, bad["W"], 4, bad["eos"], 1.0, 1.0, [0], [0], 1, "cpu", K=bad["K"])


def test_beam_advance_eviction_and_the_done_rule_by_hand():
    from rwkv_lm_ext_amd import infctx
    st = infctx.BeamSearch.create(1, 2, 6, (0,), 0.0, 1.0, [5], [9], 1, "cpu")           # length_penalty 0: a hypothesis scores its cum
    ninf = -np.inf

    def step(cands):
        parent, token, score = (torch.tensor([[c[i] for c in cands]]) for i in range(3))
        infctx.beam_advance(st, parent.int(), token.int(), score.float())

    step([(0, 0, -1.0), (0, 5, -1.5), (0, 6, -2.0), (0, 7, -2.5)])                      # an eos at rank 0; two continuations
    assert st.hyp_score.tolist() == [[-1.0, ninf]] and st.tokens.tolist() == [5, 6] and st.cum.tolist() == [-1.5, -2.0] and not st.done.any()
    assert st.slots_in.tolist() == [1, 1] and st.slots_out.tolist() == [3, 4]            # both children read row 0's slot of half 0
    step([(0, 8, -1.55), (0, 0, -1.6), (1, 9, -2.25), (1, 0, -2.5)])                    # an eos at rank 1 fills the table, one at rank 3 is ignored
    assert st.hyp_score.tolist() == [[-1.0, np.float32(-1.6)]] and st.hyp_step.tolist() == [[0, 1]] and not st.done.any()
    assert st.tokens.tolist() == [8, 9] and st.slots_in.tolist() == [3, 4] and st.slots_out.tolist() == [1, 2]
    step([(0, 2, -1.5625), (1, 0, -1.59375), (0, 3, -1.75), (1, 4, -2.5)])              # a better eos evicts the worst; the best cum is ahead
    assert st.hyp_score.tolist() == [[-1.0, -1.59375]] and st.hyp_step.tolist() == [[0, 2]] and st.hyp_row.tolist() == [[0, 1]] and not st.done.any()
    step([(0, 0, -1.625), (0, 3, -1.75), (1, 4, -2.5), (1, 5, -3.0)])                   # a worse eos is not added; nothing left can beat the table
    assert st.hyp_score.tolist() == [[-1.0, -1.59375]] and st.done.tolist() == [True] and st.cum.tolist() == [ninf, ninf]
    assert st.hist_token[:4].tolist() == [[5, 6], [8, 9], [2, 3], [-1, -1]] and st.hist_parent[:3].tolist() == [[0, 0], [0, 1], [0, 0]]
    step([(-1, -1, ninf)] * 4)                                                          # dead rows stay dead
    assert st.done.tolist() == [True] and st.cum.tolist() == [ninf, ninf] and int(st.step) == 5


# ---- 3. a whole search against a brute-force Python beam search
def wkv_one_token(total_T, C, H, pool, slot, r, k, v, w, u, cu_seqlens, max_seqlen, state_slot_out=None, **_):
    """wkv.RUN_RWKV_6_VARLEN for one token per sequence, in torch (S[key, value] per head)"""
    shape, N, n = r.shape, C // H, pool.shape[0]
    r, k, v, w = (t.reshape(total_T, H, N).float() for t in (r, k, v, w))
    src = slot.long()
    S = pool[src.clamp(0, n - 1)] * ((src >= 0) & (src < n)).view(-1, 1, 1, 1)
    kv = k.unsqueeze(3) * v.unsqueeze(2)
    y = ((S + u.float().view(1, H, N, 1) * kv) * r.unsqueeze(3)).sum(2)
    dst = (slot if state_slot_out is None else state_slot_out).long()
    assert ((dst >= 0) & (dst < n)).all()
    pool.index_copy_(0, dst, torch.exp(-torch.exp(w)).unsqueeze(3) * S + kv)
    return y.reshape(shape).to(v.dtype), pool


def brute_force(model, first, prefill, G, W, K, T, eos, lp, pen, n_return):
    """Explicit sequences, one state slot per beam and step (its parent's is copied by reading it), candidates by a full sort."""
    from rwkv_lm_ext_amd import infctx
    emb, blocks, ln_out, head = model
    pools = infctx.PackedPools.create(2, 2 + G * W * (T + 1), 128, 2, "cpu", torch.float32)
    prefill(pools, [0, 1])
    free = 2
    beams = [[dict(seq=[], cum=0.0, slot=g, tok=first[g])] for g in range(G)]
    hyps, done = [[] for _ in range(G)], [False] * G
    for t in range(T):
        rows = [(g, b) for g in range(G) for b in beams[g]]
        if not rows:
            break
        out = list(range(free, free + len(rows)))
        free += len(rows)
        x = emb(torch.tensor([b["tok"] for _, b in rows])).unsqueeze(0)
        x = infctx.step_packed(blocks, x, i32(range(len(rows) + 1)), 1, pools, i32(b["slot"] for _, b in rows), out_slots=i32(out))
        lps = torch.log_softmax(head(ln_out(x[0])).double(), 1).numpy()
        length = np.float32(f32pow(t + 1, lp))
        at = 0
        for g in range(G):
            cands = []
            for bi, b in enumerate(beams[g]):
                l = lps[at].copy()
                if pen != 1:
                    seen = sorted(set(b["seq"]))
                    l[seen] = np.where(l[seen] < 0, l[seen] * pen, l[seen] / pen)
                cands += [(-(np.float64(np.float32(b["cum"])) + l[n]), bi, n, out[at]) for n in range(l.size)]
                at += 1
            if not cands:
                continue
            cands.sort()
            cands = cands[:K]
            nxt = []
            for rank, (neg, bi, n, slot) in enumerate(cands):
                score = float(np.float32(-neg))
                if n in eos:
                    if rank < W:
                        hs = float(np.float32(score) / length)
                        if len(hyps[g]) < W or hs > hyps[g][-1][0]:
                            hyps[g].append((hs, list(beams[g][bi]["seq"])))
                            hyps[g].sort(key=lambda e: -e[0])
                            del hyps[g][W:]
                elif len(nxt) < W:
                    nxt.append(dict(seq=beams[g][bi]["seq"] + [n], cum=score, slot=slot, tok=n))
            done[g] = done[g] or (len(hyps[g]) == W and hyps[g][-1][0] >= float(np.float32(np.float32(-cands[0][0])) / length))
            beams[g] = [] if done[g] else nxt
        steps = t + 1
    res = []
    for g in range(G):
        pool = list(hyps[g]) + [(float(np.float32(b["cum"]) / np.float32(f32pow(steps, lp))), b["seq"]) for b in beams[g]]
        pool.sort(key=lambda e: -e[0])
        res.append(pool[:n_return])
    return res, done


@pytest.mark.parametrize("pen", [1.0, 1.3])
def test_a_whole_search_matches_the_brute_force(monkeypatch, pen):
    from rwkv_lm_ext_amd import infctx, wkv
    monkeypatch.setattr(wkv, "RUN_RWKV_6_VARLEN", wkv_one_token)
    G, W, T, eos, lp, n_return = 2, 3, 12, (132, 107), 0.5, 5          # ids the tiny model does produce
    model = bn.tiny_model("cpu", torch.float32)
    emb, blocks, ln_out, head = model
    prompts = [[5, 17, 200, 3], [9, 9, 42]]
    first = [p[-1] for p in prompts]

    def prefill(pools, slots):
        for p, s in zip(prompts, slots):
            for tok in p[:-1]:
                infctx.step_packed(blocks, emb(torch.tensor([tok])).unsqueeze(0), i32([0, 1]), 1, pools, i32([s]))

    with torch.no_grad():
        want, want_done = brute_force(model, first, prefill, G, W, (1 + len(eos)) * W, T, eos, lp, pen, n_return)
        pools = infctx.PackedPools.create(2, 2 + 2 * W * G, 128, 2, "cpu", torch.float32)
        prefill(pools, [0, 1])
        prompt_state = [t[:, :2].clone() for t in (pools.shift_att, pools.shift_ffn, pools.wkv)]
        spool = infctx.SamplingPool.create(2 + 2 * W * G, bn.TINY_V, "cpu") if pen != 1 else None
        st = infctx.BeamSearch.create(G, W, T, eos, lp, pen, first, [0, 1], 2, "cpu")
        for _ in range(T):
            infctx.beam_step_packed(emb, blocks, ln_out, head, st, pools, sampling_pool=spool, kernels=False)
        seq, length, score = infctx.beam_finalize(st, n_return)
    assert all(torch.equal(a, b[:, :2]) for a, b in zip(prompt_state, (pools.shift_att, pools.shift_ffn, pools.wkv)))      # only ever read
    assert st.done.tolist() == want_done
    assert tuple(seq.shape) == (G, n_return, T) and seq.dtype == torch.int32 and length.dtype == torch.int32
    finished = 0
    for g in range(G):
        for j in range(n_return):
            if j >= len(want[g]):
                assert score[g, j] == -np.inf and length[g, j] == 0 and (seq[g, j] == -1).all()
                continue
            hs, tokens = want[g][j]
            n = int(length[g, j])
            assert seq[g, j, :n].tolist() == tokens and (seq[g, j, n:] == -1).all(), (g, j)
            assert abs(float(score[g, j]) - hs) <= 1e-4 * (1 + abs(hs)), (g, j)
            finished += n < T
    assert finished >= 3                                                 # the search met an eos somewhere


def test_beam_finalize_walks_the_parent_pointers():
    from rwkv_lm_ext_amd import infctx
    st = infctx.BeamSearch.create(1, 2, 4, (0,), 1.0, 1.0, [5], [0], 1, "cpu")
    # step 0: rows (a, b) from row 0; step 1: both from row 1; step 2: row 0 from row 1, row 1 from row 0
    st.hist_parent[:3] = torch.tensor([[0, 0], [1, 1], [1, 0]], dtype=torch.int32)
    st.hist_token[:3] = torch.tensor([[11, 12], [21, 22], [31, 32]], dtype=torch.int32)
    st.step.fill_(3)
    st.cum.copy_(torch.tensor([-3.0, -6.0]))
    st.hyp_score[0, 0], st.hyp_step[0, 0], st.hyp_row[0, 0] = -1.5, 2, 1          # an eos chosen at step 2 by row 1
    seq, length, score = infctx.beam_finalize(st, 4)
    assert seq[0].tolist() == [[12, 22, 31, -1], [12, 22, -1, -1], [12, 21, 32, -1], [-1, -1, -1, -1]]
    assert length[0].tolist() == [3, 2, 3, 0] and score[0].tolist() == [-1.0, -1.5, -2.0, -np.inf]
