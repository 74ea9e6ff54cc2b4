"""The oracle of the device-side sampler (include/wkv6_amd.h: rwkv6_sample_slots_*), shared by test_sample_slots_cpu.py and
test_sample_slots_gpu.py: the operation restated row by row in numpy.  The penalised logit z is formed in fp32, as the operation defines it
(so that order and ties are the operation's), everything behind it -- softmax, cumulative sums, weights, the draw -- in fp64.

sample_row returns the kept mask, the token, the log-probability and the new occurrence row, and `decisive`: whether the row's integer
results are beyond the reach of rounding --
  * the nucleus boundary is clear: |cum[c] - top_p| and |cum[c-1] - top_p| both exceed 1e-4;
  * u is more than 1e-4 away from every step of the kept set's CDF;
  * every o[n] that is compared with 0 is exactly 0, or at least 1e-6.
make_case is the input generator of the tests."""
import numpy as np

MARGIN = 1e-4
f32 = np.float32


def penalised(logits, o, ap, af):
    """step 1 in fp32: two roundings (the product, the sum) and the subtraction's."""
    logits, o = logits.astype(f32), o.astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        z = np.where(o > 0, logits - (f32(ap) + o * f32(af)).astype(f32), logits).astype(f32)
    return z + f32(0)          # -0 -> +0


def repeat_penalised(z, o, pen):
    """step 5 in fp32, on every n (the caller selects)."""
    if f32(pen) == f32(1):
        return z
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        y = np.where(z < 0, z * f32(pen), z / f32(pen)).astype(f32) + f32(0)
    return np.where(o > 0, y, z).astype(f32)


def sample_row(logits, o, params, u):
    """logits [V] and o [V] (the source occurrence row; zeros for a slot outside the pool) as fp32 values, params [8], u a float.
    Returns a dict: poisoned, kept [V] bool, token, logprob, occ [V] fp32 (the new row; None for a poisoned row), decisive."""
    logits, o, params = np.asarray(logits, f32), np.asarray(o, f32), np.asarray(params, f32)
    V = logits.shape[0]
    temperature, top_p, top_k, ap, af, decay, pen = (params[i] for i in range(7))
    if (np.isnan(logits).any() or (logits == np.inf).any() or not np.isfinite(logits).any()
            or not (np.isfinite(params).all() and (params >= 0).all())):
        return dict(poisoned=True, kept=np.zeros(V, bool), token=-1, logprob=np.nan, occ=None, decisive=True)
    decisive = bool(np.all((o == 0) | (o >= 1e-6)))
    z = penalised(logits, o, ap, af)
    ids = np.arange(V)
    order = np.lexsort((ids, -z.astype(np.float64)))                       # z descending, n ascending
    z64 = z.astype(np.float64)
    p = np.exp(z64 - z64.max())
    p /= p.sum()
    kept = np.ones(V, bool)
    if top_p < 1:
        cum = np.cumsum(p[order])
        reach = np.nonzero(cum >= np.float64(top_p))[0]
        if reach.size:
            c = reach[0]
            kept = z >= z[order[c]]
            decisive &= abs(cum[c] - top_p) > MARGIN and (c == 0 or abs(cum[c - 1] - top_p) > MARGIN)
        else:
            decisive = False                                               # rounding alone keeps the sum under top_p: everything stays
    if 1 <= top_k < V:
        first = np.zeros(V, bool)
        first[order[:int(top_k)]] = True
        kept &= first
    z2 = repeat_penalised(z, o, pen).astype(np.float64)
    if temperature == 0:
        token = int(np.nonzero(z2 == z2.max())[0][0])
        logprob = 0.0
    else:
        w = np.where(kept, np.exp((z2 - z2[kept].max()) / np.float64(temperature)), 0.0)
        cdf = np.cumsum(w)
        W = cdf[-1]
        hit = np.nonzero(kept & (cdf > np.float64(u) * W))[0]
        token = int(hit[0]) if hit.size else int(ids[kept][-1])
        logprob = float(np.log(w[token] / W))
        decisive &= bool(np.all(np.abs(cdf[kept] / W - np.float64(u)) > MARGIN))
    occ = (o * f32(decay)).astype(f32)
    occ[token] = occ[token] + f32(1)
    return dict(poisoned=False, kept=kept, token=token, logprob=logprob, occ=occ, decisive=bool(decisive))


def round_to(x, dtype):
    """fp32 values of x rounded to the torch dtype (as fp32 again)."""
    import torch
    return torch.from_numpy(np.asarray(x, f32)).to(dtype).float().numpy()


def make_case(rng, V, dtype, penalties=True):
    """One row of the tests' input family: a head of up to 48 tokens at random ids that always include 0 and V - 1, head logit i at
    -0.25 i +- 0.1, every other token at -40; top_p uniform in [0.3, 0.98], top_k in {0, 5, 20}, temperature in {0, 0.7, 1, 1.5};
    occurrence counts on a few head tokens.  Returns (logits [V] fp32 values of `dtype`, o [V] fp32, params [8] fp32, u)."""
    n_head = min(48, V)
    ids = np.array([0, V - 1][:min(2, V)] if V > 1 else [0])
    rest = np.setdiff1d(np.arange(V), ids)
    ids = np.concatenate([ids, rng.choice(rest, n_head - ids.size, replace=False)]) if n_head > ids.size else ids
    ids = rng.permutation(ids)
    logits = np.full(V, -40.0, f32)
    logits[ids] = -0.25 * np.arange(ids.size) + rng.uniform(-0.1, 0.1, ids.size)
    logits = round_to(logits, dtype)
    o = np.zeros(V, f32)
    params = np.zeros(8, f32)
    params[0] = rng.choice([0.0, 0.7, 1.0, 1.5])
    params[1] = rng.uniform(0.3, 0.98)
    params[2] = rng.choice([0, 5, 20])
    params[5] = 1.0
    params[6] = 1.0
    if penalties:
        seen = rng.choice(ids, min(4, ids.size), replace=False)
        o[seen] = rng.choice([0.5, 1.0, 1.996, 3.0], seen.size).astype(f32)
        params[3], params[4], params[5] = 0.3, 0.2, 0.996
        params[6] = rng.choice([1.0, 1.1])
    return logits, o, params, float(f32(rng.uniform(0, 1 - 1e-6)))


# ---- the parametrisation of the exact comparison (test_sample_slots_gpu.py runs it on the kernel, test_sample_slots_cpu.py bounds the share
# of rows in it that are not decisive)
DTYPE_NAMES = ("bf16", "fp16", "fp32")
SHAPES = [(8, 8), (64, 64), (997, 1000), (50277, 50280), (65536, 65536)]
CASES = [(d, V, ld, n) for d in DTYPE_NAMES for V, ld in SHAPES for n in ((1, 3) if V == 65536 else (1, 3, 257))]


def case_rows(dname, V, n_seq):
    """The rows of one case, from a seed of the case's own."""
    import torch
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dname]
    rng = np.random.default_rng(V + n_seq + len(dname) + ord(dname[0]))
    return [make_case(rng, V, dtype) for _ in range(n_seq)]
