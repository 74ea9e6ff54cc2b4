"""The fp64 oracle of the beam-search candidate selection (include/wkv6_amd.h: rwkv6_beam_candidates_*), shared by test_beam_cpu.py,
test_beam_gpu.py and test_beam_step_gpu.py: the operation restated group by group in numpy, every value in fp64 (the inputs are the fp32
values the operation is given), and the bounds the tests hold the fp32 results to.

candidates() returns the K best of every group and, per group, every candidate there is with its fp64 score, so that a test can apply the
band rule: with tol the score bound of a candidate, whatever lies more than 2 tol above the oracle's K-th score must be selected and
nothing more than 2 tol below it may be."""
import numpy as np

f32 = np.float32
EPS = 2.0 ** -24
# |s - s64| <= K_TOL * 2^-24 * (1 + |cum| + |lp64| * max(p, 1/p)).  Six rounded fp32 operations lie between a logit and its score (z - m,
# the rounding of L, - L, the penalty, + cum, and expf inside L), so the constant may not exceed 64; it is four times the largest ratio
# measured over the inputs of test_beam_gpu.py (DESIGN.md 4.24 has the measurement).
K_TOL = 6.6


def row_state(z, cum, p):
    """'dead', 'poisoned' or 'live' (steps 1 and 2)."""
    if cum == -np.inf:
        return "dead"
    if np.isnan(z).any() or (z == np.inf).any() or not np.isfinite(z).any() or not np.isfinite(cum) or not (np.isfinite(p) and p >= 0):
        return "poisoned"
    return "live"


def row_scores(z, cum, o, p):
    """(s64 [V], tol [V]) of a live row: steps 3 to 5 in fp64; -inf where the token is no candidate."""
    z = z.astype(np.float64)
    m = z.max()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lp = (z - m) - np.log(np.exp(z - m).sum())
        width = np.abs(lp)
        if p != 1:
            pen = np.where(lp < 0, lp * p, lp / p)
            pen = np.where(np.isnan(pen), 0.0, pen)
            lp = np.where(o > 0, pen, lp)
            width = np.where(o > 0, width * max(p, 1 / p if p > 0 else np.inf), width)
        s = np.float64(cum) + lp
        tol = K_TOL * EPS * (1 + abs(np.float64(cum)) + width)
    s = np.where(z > -np.inf, s, -np.inf)
    return s, np.where(np.isfinite(tol), tol, np.inf)


def candidates(logits, cum, cu_rows, K, occ=None, slot=None, penalty=None):
    """logits [n_rows,V], cum [n_rows], cu_rows [n_groups+1], occ [n_slots,V] / slot [n_rows] / penalty [n_groups] or None.  Returns a dict:
    parent, token int [n_groups,K], score fp64 [n_groups,K] (-1, -1, -inf where missing), and `groups`: per group (rows, tokens, s64, tol)
    of the candidates, in the order (s descending, row ascending, token ascending).  Of a row with more than 64 candidates only those down
    to 4 tol under its 64th score are listed: the rest lies more than 2 tol under the K-th score of any group for any K <= 64, so check_band
    refuses it, if it is ever selected, as it refuses what is no candidate at all."""
    logits, cum = np.asarray(logits, f32), np.asarray(cum, f32)
    n_rows, V = logits.shape
    cu = np.clip(np.asarray(cu_rows, np.int64), 0, n_rows)
    n_groups = cu.size - 1
    parent, token = np.full((n_groups, K), -1), np.full((n_groups, K), -1)
    score = np.full((n_groups, K), -np.inf)
    groups = []
    for g in range(n_groups):
        p = 1.0 if penalty is None else float(f32(penalty[g]))
        rows, toks, ss, tols = [], [], [], []
        for r in range(cu[g], min(cu[g + 1], cu[g] + 64)):
            if row_state(logits[r], cum[r], p) != "live":
                continue
            sl = r if slot is None else int(slot[r])
            o = occ[sl] if occ is not None and 0 <= sl < occ.shape[0] else np.zeros(V, f32)
            s, tol = row_scores(logits[r], cum[r], np.asarray(o, f32), p)
            keep = np.nonzero(s > -np.inf)[0]
            if keep.size > 64:           # K <= 64: what lies 4 tol under the row's 64th score is more than 2 tol under any group's K-th
                floor = np.partition(s[keep], keep.size - 64)[keep.size - 64] - 4 * tol[keep].max()
                keep = keep[s[keep] >= floor]
            rows.append(np.full(keep.size, r)); toks.append(keep); ss.append(s[keep]); tols.append(tol[keep])
        if rows:
            rows, toks, ss, tols = (np.concatenate(x) for x in (rows, toks, ss, tols))
            order = np.lexsort((toks, rows, -ss))
            rows, toks, ss, tols = rows[order], toks[order], ss[order], tols[order]
        else:
            rows, toks, ss, tols = np.zeros(0, int), np.zeros(0, int), np.zeros(0), np.zeros(0)
        n = min(K, rows.size)
        parent[g, :n], token[g, :n], score[g, :n] = rows[:n], toks[:n], ss[:n]
        groups.append((rows, toks, ss, tols))
    return dict(parent=parent, token=token, score=score, groups=groups)


def check_band(want, parent, token, score, K, exact=False):
    """The checks every result goes through.  Returns the largest |s - s64| / (tol / K_TOL) seen (the measured ratio of the tolerance).
    exact: parents and tokens must equal the oracle's."""
    worst = 0.0
    for g, (rows, toks, ss, tols) in enumerate(want["groups"]):
        n = min(K, rows.size)
        got = list(zip(parent[g, :n].tolist(), token[g, :n].tolist()))
        assert (parent[g, n:] == -1).all() and (token[g, n:] == -1).all() and (score[g, n:] == -np.inf).all(), g
        assert len(set(got)) == n and all(r >= 0 and t >= 0 for r, t in got), (g, got)
        if exact:
            assert got == list(zip(rows[:n].tolist(), toks[:n].tolist())), g
        at = {(r, t): i for i, (r, t) in enumerate(zip(rows.tolist(), toks.tolist()))}
        idx = np.array([at[c] for c in got], int)                      # KeyError: something that is no candidate was selected
        s = score[g, :n].astype(np.float64)
        err = np.abs(s - ss[idx])
        assert (err <= tols[idx]).all(), (g, err.max(), tols[idx][err.argmax()])
        if n:
            worst = max(worst, float((err / (tols[idx] / K_TOL)).max()))
        assert (np.diff(s) <= 0).all(), g                              # best first
        if rows.size > K:
            kth = ss[K - 1]
            must = np.nonzero(ss - 2 * tols > kth)[0]
            assert set(must.tolist()) <= set(idx.tolist()), g
            assert (ss[idx] + 2 * tols[idx] >= kth).all(), g
    return worst


# ---- the inputs of the candidate tests (test_beam_cpu.py on the eager code, test_beam_gpu.py on the kernels)
def round_to(x, dtype_name):
    """fp32 values of x rounded to bf16 / fp16 / fp32 (as fp32 again)."""
    import torch
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dtype_name]
    return torch.from_numpy(np.ascontiguousarray(x, f32)).to(dtype).float().numpy()


def make_inputs(seed, cu, V, dtype_name, n_rows=None, penalty=False, n_slots=5):
    """logits [n_rows,V] (N(0, 3^2) rounded to the type: a 16-bit type leaves many equal logits in a row), cum in [-20, 0], and with
    `penalty` an occurrence pool with a few percent of its entries set, slots that include one on either side of the pool, and a penalty
    per group from {1, 1.3, 0.8}."""
    rng = np.random.default_rng(seed)
    n_rows = max(cu) if n_rows is None else n_rows
    d = dict(logits=round_to(rng.normal(0, 3, (n_rows, V)), dtype_name), cum=(-rng.uniform(0, 20, n_rows)).astype(f32), cu=np.asarray(cu, np.int32),
             occ=None, slot=None, penalty=None)
    if penalty:
        d["occ"] = ((rng.uniform(size=(n_slots, V)) < 0.08) * rng.choice([0.5, 1.0, 3.0], (n_slots, V))).astype(f32)
        d["slot"] = rng.integers(-1, n_slots + 1, n_rows).astype(np.int32)
        d["penalty"] = rng.choice([1.0, 1.3, 0.8], len(cu) - 1).astype(f32)
    return d


def oracle_of(d, K):
    return candidates(d["logits"], d["cum"], d["cu"], K, d["occ"], d["slot"], d["penalty"])


# ---- the tiny model of the search tests: C = 128, H = 2, 2 layers (the weights of oracle/caller_weights.py), V = 264
TINY_V = 264


def tiny_model(device, dtype):
    """(emb, blocks, ln_out, head) with seeded weights"""
    import torch
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
        blocks.append(b.to(device).to(dtype).requires_grad_(False))
    emb = torch.nn.Embedding(TINY_V, cw.N_EMBD)
    ln_out = torch.nn.LayerNorm(cw.N_EMBD)
    head = torch.nn.Linear(cw.N_EMBD, TINY_V, bias=False)
    with torch.no_grad():
        emb.weight.copy_(torch.randn(TINY_V, cw.N_EMBD, generator=g))
        head.weight.copy_(torch.randn(TINY_V, cw.N_EMBD, generator=g) * 0.3)
    emb, ln_out, head = (m.to(device).to(dtype).requires_grad_(False) for m in (emb, ln_out, head))
    return emb, blocks, ln_out, head
