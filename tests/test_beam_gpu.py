"""GPU tier of the beam-search candidate kernels (include/wkv6_amd.h: rwkv6_beam_candidates_*; csrc/wkv6_beam.hip) through
mix_op.beam_candidates, against the fp64 oracle of tests/beam_numpy.py at the smallest shapes that can go wrong: V in {1, 7, 8, 9, 1000 (row
strides 1000 and 1024), 8200 (more than one round of the 1024 threads), 65536}, K in {1, 5, 64}, groups of 0, 1, 3 and 64 rows and three
groups with uneven bounds, the three logits types, the penalty on and off.

Every result goes through beam_numpy.check_band: the scores within the bound stated there, best first, every candidate clearly above the
oracle's K-th selected and none clearly below it.  Where the order is exact by construction, tokens and parents are compared for equality.
Each case prints the largest measured share of the score bound (`pytest -s`)."""
import functools

import numpy as np
import pytest
import torch

import beam_numpy as bn

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
SHAPES = [(1, 8), (7, 8), (8, 8), (9, 16), (1000, 1000), (1000, 1024), (8200, 8200), (65536, 65536)]
LAYOUTS = {"0+1": [0, 0, 1], "3": [0, 3], "uneven": [0, 2, 2, 7], "64": [0, 64]}
KS = (1, 5, 64)


def run(d, K, dname, ld=None, fill=77.0):
    """mix_op.beam_candidates on the inputs of beam_numpy (numpy arrays); columns V .. ld - 1 of logits and pool hold values that must
    never matter."""
    from rwkv_lm_ext_amd import mix_op
    n_rows, V = d["logits"].shape
    ld = (V + 7) // 8 * 8 if ld is None else ld
    lg = torch.full((n_rows, ld), fill, dtype=DTYPES[dname], device="cuda")
    lg[:, :V] = torch.from_numpy(d["logits"]).to(DTYPES[dname])
    occ = slots = penalty = None
    if d["occ"] is not None:
        occ = torch.full((d["occ"].shape[0], ld), 5.0, device="cuda")
        occ[:, :V] = torch.from_numpy(d["occ"])
        occ = occ[:, :V]
        slots = None if d["slot"] is None else torch.from_numpy(d["slot"]).cuda()
        penalty = torch.from_numpy(d["penalty"]).cuda()
    with torch.no_grad():
        out = mix_op.beam_candidates(lg[:, :V], torch.from_numpy(d["cum"]).cuda(), torch.from_numpy(d["cu"]).cuda(), K, occ_pool=occ, slots=slots,
                                     penalty=penalty)
    torch.cuda.synchronize()
    parent, token, score = (t.cpu().numpy() for t in out)
    assert parent.dtype == np.int32 and token.dtype == np.int32 and score.dtype == np.float32
    assert parent.shape == token.shape == score.shape == (len(d["cu"]) - 1, K)
    return parent, token, score


@functools.lru_cache(maxsize=None)
def case(V, dname, layout, penalty):
    """the inputs of one case and their oracle, computed once (the oracle's candidate lists do not depend on K)"""
    d = bn.make_inputs(V + len(layout) + 7 * penalty + ord(dname[0]), LAYOUTS[layout], V, dname, penalty=penalty)
    return d, bn.oracle_of(d, 1)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("V,ld", SHAPES)
def test_candidates_match_the_oracle(V, ld, dname):
    worst = 0.0
    for layout in LAYOUTS:
        for penalty in (False, True):
            d, want = case(V, dname, layout, penalty)
            for K in KS:
                worst = max(worst, bn.check_band(want, *run(d, K, dname, ld), K))
    print(f"V = {V}, ld = {ld}, {dname}: largest |s - s64| / (2^-24 (1 + |cum| + |lp| max(p, 1/p))) = {worst:.3f} (bound {bn.K_TOL})")


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("V", [9, 1000, 65536])
def test_single_rows_come_in_the_order_of_the_logits(V, dname):
    """No penalty, one row a group: the order is (z descending, id ascending) whatever the rounding of the scores, heavy ties included (a
    16-bit type leaves thousands of equal logits in a row of 65536; the third row is made of four values only)."""
    rng = np.random.default_rng(V)
    z = bn.round_to(rng.normal(0, 3, (3, V)), dname)
    z[2] = rng.choice([-1.5, 0.0, 0.25, 2.0], V)
    z[2, rng.integers(0, V, max(1, V // 10))] = -np.inf
    d = dict(logits=z, cum=np.array([0.0, -3.5, -100.0], np.float32), cu=np.arange(4, dtype=np.int32), occ=None, slot=None, penalty=None)
    for K in KS:
        parent, token, score = run(d, K, dname)
        for r in range(3):
            n = min(K, int((z[r] > -np.inf).sum()))
            assert token[r, :n].tolist() == np.lexsort((np.arange(V), -z[r].astype(np.float64)))[:n].tolist(), (K, r)
            assert (parent[r, :n] == r).all() and (parent[r, n:] == -1).all() and (token[r, n:] == -1).all() and (score[r, n:] == -np.inf).all()
    bn.check_band(bn.oracle_of(d, 64), parent, token, score, 64)


@pytest.mark.parametrize("dname", list(DTYPES))
def test_identical_rows_tie_by_row_then_token(dname):
    V, K = 1000, 64
    rng = np.random.default_rng(11)
    z = rng.integers(-8, 3, V).astype(np.float32) * 0.5                  # a grid that every type holds: about 90 tokens share a logit
    for n_rows, cum in ((3, [-1.0, -1.0, -1.0]), (64, [-2.0] * 64), (3, [-1024.0, 0.0, -512.0]), (5, [-8.0, -4096.0, -8.0, 0.0, 0.0])):
        d = dict(logits=np.stack([z] * n_rows), cum=np.array(cum, np.float32), cu=np.array([0, n_rows], np.int32), occ=None, slot=None, penalty=None)
        want = bn.oracle_of(d, K)
        parent, token, score = run(d, K, dname)
        assert parent.tolist() == want["parent"].tolist() and token.tolist() == want["token"].tolist(), cum
        bn.check_band(want, parent, token, score, K, exact=True)


def ibits(x):
    return np.ascontiguousarray(x).view(np.int32)


@pytest.mark.parametrize("dname", list(DTYPES))
def test_dead_poisoned_and_short_rows(dname):
    V, K = 1003, 64
    rng = np.random.default_rng(3)
    lg = bn.round_to(rng.normal(0, 2, (8, V)), dname)
    lg[0, 5:] = -np.inf                         # fewer than K candidates in the group: the rest is -1 / -inf
    lg[1] = np.nan                              # dead: never read
    lg[2, 3] = np.inf                           # poisoned beside a healthy row
    lg[4] = -np.inf                             # no finite logit
    lg[5, 900] = np.nan                         # poisoned
    lg[6, ::2] = -np.inf
    cum = np.array([-1, -np.inf, -2, -3, -4, -5, -6, -7], np.float32)
    d = dict(logits=lg, cum=cum, cu=np.array([0, 2, 4, 6, 8], np.int32), occ=None, slot=None, penalty=None)
    want = bn.oracle_of(d, K)
    parent, token, score = run(d, K, dname)
    bn.check_band(want, parent, token, score, K, exact=dname == "fp32")
    assert (parent[0, :5] == 0).all() and token[0, :5].tolist() == want["token"][0, :5].tolist() and (parent[0, 5:] == -1).all()
    assert (parent[1] == 3).all() and (parent[2] == -1).all() and set(parent[3].tolist()) <= {6, 7}
    # the healthy neighbours of the poisoned rows: the same bits as alone
    for g, r in ((1, 3),):
        alone = run(dict(d, logits=lg[r:r + 1], cum=cum[r:r + 1], cu=np.array([0, 1], np.int32)), K, dname)
        assert np.array_equal(alone[1][0], token[g]) and np.array_equal(ibits(alone[2][0]), ibits(score[g]))
    # a NaN or +inf cum poisons the row, a negative or non-finite penalty the group; the other groups keep their bits
    for bad in (np.nan, np.inf):
        q = run(dict(d, cum=np.where(np.arange(8) == 3, bad, cum).astype(np.float32)), K, dname)
        assert (q[0][1] == -1).all() and np.array_equal(q[1][[0, 3]], token[[0, 3]]) and np.array_equal(ibits(q[2][[0, 3]]), ibits(score[[0, 3]]))
    occ = np.zeros((8, V), np.float32)
    for bad in (-1.0, np.nan, np.inf):
        q = run(dict(d, occ=occ, penalty=np.array([1.0, 1.0, 1.0, bad], np.float32)), K, dname)
        assert (q[0][3] == -1).all() and (q[2][3] == -np.inf).all()
        assert np.array_equal(q[1][:3], token[:3]) and np.array_equal(ibits(q[2][:3]), ibits(score[:3]))


@pytest.mark.parametrize("dname", list(DTYPES))
def test_rows_alone_and_in_a_batch_and_two_calls_give_the_same_bits(dname):
    V, K, n = 8200, 64, 5
    d = bn.make_inputs(17, list(range(n + 1)), V, dname, penalty=True, n_slots=4)
    d["slot"] = np.array([0, 3, -1, 4, 2], np.int32)                     # one slot on either side of the pool: no occurrences
    first, second = run(d, K, dname), run(d, K, dname)
    assert all(np.array_equal(ibits(a), ibits(b)) for a, b in zip(first, second))
    bn.check_band(bn.oracle_of(d, K), *first, K)
    no_occ = bn.oracle_of(dict(d, occ=np.zeros_like(d["occ"])), K)
    for r in (2, 3):
        if d["penalty"][r] != 1:
            bn.check_band(dict(groups=[no_occ["groups"][r]]), *(x[r:r + 1] for x in first), K)
    for r in range(n):
        one = dict(d, logits=d["logits"][r:r + 1], cum=d["cum"][r:r + 1], cu=np.array([0, 1], np.int32), slot=d["slot"][r:r + 1],
                   penalty=d["penalty"][r:r + 1])
        alone = run(one, K, dname)
        assert np.array_equal(alone[1][0], first[1][r]) and np.array_equal(ibits(alone[2][0]), ibits(first[2][r])), r
        assert (alone[0][0] == 0).all() and (first[0][r] == r).all()


def test_infctx_dispatch_and_padded_heads():
    """infctx.beam_candidates: kernels=True and None take the kernels on a padded head and give the eager code's candidates; a head that
    is not padded goes to the eager code under None and raises under True."""
    from rwkv_lm_ext_amd import infctx
    V, ld, K = 1003, 1008, 9
    d = bn.make_inputs(23, [0, 3, 6], V, "bf16", penalty=True, n_slots=6)
    d["slot"] = np.array([0, 1, 2, 3, 4, 5], np.int32)
    lg = torch.full((6, ld), 50.0, dtype=torch.bfloat16, device="cuda")
    lg[:, :V] = torch.from_numpy(d["logits"]).bfloat16()
    pool = infctx.SamplingPool.create(6, V, "cuda", ld=ld)
    pool.occ[:, :V] = torch.from_numpy(d["occ"])
    args = (torch.from_numpy(d["cum"]).cuda(), torch.from_numpy(d["cu"]).cuda(), K)
    kw = dict(pool=pool, slots=torch.from_numpy(d["slot"]).cuda(), penalty=torch.from_numpy(d["penalty"]).cuda())
    want = bn.oracle_of(d, K)
    outs = {k: [t.cpu().numpy() for t in infctx.beam_candidates(lg, *args, kernels=k, **kw)] for k in (True, None, False)}
    for k, out in outs.items():
        bn.check_band(want, *out, K)
    assert all(np.array_equal(ibits(a), ibits(b)) for a, b in zip(outs[True], outs[None]))
    plain = lg[:, :V].contiguous()
    bn.check_band(bn.oracle_of(dict(d, occ=None, slot=None, penalty=None), K), *(t.cpu().numpy() for t in infctx.beam_candidates(plain, *args, vocab=V)), K)
    with pytest.raises(RuntimeError, match="ld"):
        infctx.beam_candidates(plain, *args, vocab=V, kernels=True)
