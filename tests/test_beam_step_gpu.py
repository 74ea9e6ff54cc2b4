"""GPU tier of the beam search on the packed serving step (infctx.beam_step_packed with kernels=True and the slot-pool kernels) on the tiny
model of tests/beam_numpy.py in bf16: W = 3, 2 requests, 12 steps, with the repetition penalty.

  * every step's selection against the fp64 oracle on that step's own logits (band rule of beam_numpy.check_band);
  * the fork: the WKV and shift slots every final row reads equal what a fresh replay of its token sequence from the prompt slot leaves,
    bit for bit (the replay runs all rows in one batch of the same shape, so that the GEMMs see what the search showed them);
  * the step captured in a graph and replayed gives the same tokens, scores, tables, histories and pools as the uncaptured run, bitwise;
  * the prompt slots are unchanged at the end."""
import numpy as np
import pytest
import torch

import beam_numpy as bn

pytestmark = pytest.mark.gpu

bf = torch.bfloat16
G, W, T, EOS, LP, PEN = 2, 3, 12, (132, 107), 0.5, 1.3
N_SLOTS, BASE, PROMPT = 2 + 2 * W * G, 2, [0, 1]
PROMPTS = [[5, 17, 200, 3], [9, 9, 42]]
STATE_FIELDS = ("step", "tokens", "cum", "slots_in", "slots_out", "slots_occ", "hist_parent", "hist_token", "hyp_score", "hyp_step", "hyp_row", "done")


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def bits(t):
    return t.view(torch.int16) if t.dtype == bf else t.view(torch.int32) if t.dtype == torch.float32 else t


class Keep(torch.nn.Module):
    """the head, keeping the logits it last gave"""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.last = inner, None

    def forward(self, x):
        self.last = self.inner(x)
        return self.last


@pytest.fixture(scope="module")
def search():
    """The uncaptured search, run once: the model, the per-step records, the final state and pools."""
    from rwkv_lm_ext_amd import infctx
    emb, blocks, ln_out, head = bn.tiny_model("cuda", bf)
    head = Keep(head)

    def fresh():
        pools = infctx.PackedPools.create(2, N_SLOTS, 128, 2, "cuda", bf)
        with torch.no_grad():
            for p, s in zip(PROMPTS, PROMPT):
                for tok in p[:-1]:
                    infctx.step_packed(blocks, emb(i32([tok]).long()).unsqueeze(0), i32([0, 1]), 1, pools, i32([s]), pool_kernels=True)
        spool = infctx.SamplingPool.create(N_SLOTS, bn.TINY_V, "cuda")
        spool.occ[0, [5, 17, 200]] = 1.0                                  # the prompts' counts, in the prompt slots
        spool.occ[1, 9] = 2.0
        st = infctx.BeamSearch.create(G, W, T, EOS, LP, PEN, [p[-1] for p in PROMPTS], PROMPT, BASE, "cuda")
        return st, pools, spool

    def step(st, pools, spool):
        return infctx.beam_step_packed(emb, blocks, ln_out, head, st, pools, sampling_pool=spool, pool_kernels=True, kernels=True)

    st, pools, spool = fresh()
    prompt_state = [t[:, :2].clone() for t in (pools.shift_att, pools.shift_ffn, pools.wkv)] + [spool.occ[:2].clone()]
    records = []
    with torch.no_grad():
        for _ in range(T):
            before = dict(cum=st.cum.cpu().numpy(), slot=st.slots_occ.cpu().numpy(), occ=spool.occ[:, :bn.TINY_V].cpu().numpy())
            out = step(st, pools, spool)
            torch.cuda.synchronize()
            records.append(dict(before, logits=head.last.float().cpu().numpy(), out=[t.cpu().numpy() for t in out]))
    return dict(model=(emb, blocks, ln_out, head), fresh=fresh, step=step, st=st, pools=pools, spool=spool, records=records, prompt_state=prompt_state)


def test_every_step_selects_what_the_oracle_selects(search):
    st = search["st"]
    cu, penalty = np.arange(0, G * W + 1, W), np.full(G, PEN, np.float32)
    live_rows = 0
    for t, r in enumerate(search["records"]):
        want = bn.candidates(r["logits"], r["cum"], cu, st.K, r["occ"], r["slot"], penalty)
        bn.check_band(want, *r["out"], st.K)
        live_rows += int((r["cum"] > -np.inf).sum())
        assert t > 0 or (r["cum"] > -np.inf).sum() == G                   # one live row a request at the first step
    assert live_rows > G * T                                              # the beams did fan out
    assert (search["st"].hyp_score > -np.inf).any()                       # and an eos was met


def test_the_forked_slots_equal_a_fresh_replay(search):
    from rwkv_lm_ext_amd import infctx
    emb, blocks, ln_out, head = search["model"]
    st, pools = search["st"], search["pools"]
    hist_parent, hist_token = st.hist_parent.cpu().numpy(), st.hist_token.cpu().numpy()
    n_rows = G * W
    live = (st.cum > -np.inf).cpu().numpy()
    assert live.any()
    fed = np.zeros((T, n_rows), np.int64)                                 # what row r's ancestors fed at step t; dead rows feed token 0
    for r in np.nonzero(live)[0]:
        row = r
        for t in range(T - 1, -1, -1):
            row = hist_parent[t, row]                                     # the ancestor that entered step t
            fed[t, r] = hist_token[t - 1, row] if t else PROMPTS[r // W][-1]
    assert (fed >= 0).all()
    # the replay: every row a sequence of its own, slots 2 + r and 2 + n_rows + r in turn, from its request's prompt slot
    _, rpools, _ = search["fresh"]()
    with torch.no_grad():
        src = i32(PROMPT[r // W] for r in range(n_rows))
        for t in range(T):
            dst = i32(2 + (t % 2) * n_rows + r for r in range(n_rows))
            x = emb(torch.from_numpy(fed[t]).cuda()).unsqueeze(0)
            infctx.step_packed(blocks, x, i32(range(n_rows + 1)), 1, rpools, src, out_slots=dst, pool_kernels=True)
            src = dst
    torch.cuda.synchronize()
    slots_in = st.slots_in.cpu().numpy()
    for r in np.nonzero(live)[0]:
        for name in ("shift_att", "shift_ffn", "wkv"):
            a, b = getattr(pools, name)[:, int(slots_in[r])], getattr(rpools, name)[:, int(src[r])]
            assert torch.equal(bits(a), bits(b)), (r, name)


def test_the_prompt_slots_are_unchanged(search):
    pools, spool = search["pools"], search["spool"]
    now = [t[:, :2] for t in (pools.shift_att, pools.shift_ffn, pools.wkv)] + [spool.occ[:2]]
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(search["prompt_state"], now))


def test_the_captured_step_replays_the_search(search):
    from rwkv_lm_ext_amd import infctx
    step = search["step"]
    gst, gpools, gspool = search["fresh"]()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        step(*search["fresh"]())                                          # warm-up on state of its own
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = step(gst, gpools, gspool)
    torch.cuda.current_stream().wait_stream(side)
    for t in range(T):
        graph.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(a.cpu().numpy().view(np.int32), b.view(np.int32)) for a, b in zip(out, search["records"][t]["out"])), t
    st, pools, spool = search["st"], search["pools"], search["spool"]
    for f in STATE_FIELDS:
        assert torch.equal(bits(getattr(gst, f)), bits(getattr(st, f))), f
    for f in ("shift_att", "shift_ffn", "wkv"):
        assert torch.equal(bits(getattr(gpools, f)), bits(getattr(pools, f))), f
    assert torch.equal(bits(gspool.occ), bits(spool.occ))
    a, b = infctx.beam_finalize(gst, 4), infctx.beam_finalize(st, 4)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    assert (a[1][:, 0] > 0).all() and (a[0][:, 0, 0] >= 0).all()
