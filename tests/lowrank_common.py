"""What the low-rank time-mix tests share (mix_op.tmix_inputs, mix_op.decay_lowrank; include/wkv6_amd.h): the inputs of the parity cases, the
row rule for the token in front of a row, a restatement of both operations in fp64 with their four bf16 rounding points, an
fp32-accumulating emulation of the chain under several summation orders (what the tolerance constant K_BOUND was measured with:
tools/lowrank_parity.py, profiles/lowrank_parity.txt), and the two assertions of the parity check.  torch on the CPU only; nothing here
reads a file."""
import functools
import math

import torch

F64 = torch.float64
# (C, D, Dd) of the kernels' instantiations at the widths the GPU tests run.  The shrink cuts C into 4 interleaved chunks of 32-wide steps
# and walks a chunk 4 steps at a time (the main loop), then one at a time (the remainder): C / 32 steps in all.
#   64, 128, 192       2, 4, 6 steps: fewer chunks than waves, the remainder loop alone; 1 to 3 column blocks in the expand
#   2048, 4096         64, 128 steps: the main loop alone; D = 64 / Dd = 128 at 4096
#   576 (D 64, Dd 128) 18 steps: the main loop once, then one remainder step for chunks 0 and 1 and none for 2 and 3; the wide ranks at a
#                      narrow C
#   768                24 steps: the main loop once, then two remainder steps a chunk (n_embd of the 0.1B model)
#   1088               34 steps: the main loop twice, then a remainder step for chunks 0 and 1; 17 column blocks in the expand, so the last
#                      workgroup has one live wave
#   4096 (D 32, Dd 64) the narrow ranks at the widest C
W64, W128, W192, W2048, W4096 = (64, 32, 64), (128, 32, 64), (192, 32, 64), (2048, 32, 64), (4096, 64, 128)
W576, W768, W1088, W4096_NARROW = (576, 64, 128), (768, 32, 64), (1088, 32, 64), (4096, 32, 64)
WIDTHS = (W64, W128, W192, W2048, W4096, W576, W768, W1088, W4096_NARROW)
EDGE_WIDTHS = (W64, W128, W768, W4096)                 # what the slot and row-rule tests run: both short loops, both loops in one call, the widest
NAN_WIDTHS = (W64, W128, W768, W2048, W4096)           # what the NaN containment tests run
ROWS = (1, 15, 16, 17, 33)
# (C, N, Dd) of decay_lowrank with dim_att N != C: x, D1 and the shrink go by C; D2, time_decay and the rows of w by N.  N < C behind both
# loops; N > C with a live wave count of 1 (5 blocks); the wide rank with 17 blocks behind 18 steps; the narrowest C under the widest N
DECAY_CASES = ((768, 512, 64), (128, 320, 64), (576, 1088, 128), (64, 4096, 64))
CAP = 1e-3            # at most this share of a call's elements may differ from the restatement in their bits at all
# the packed batch of the parity cases, shared by the GPU tests and the CPU measurement of K_BOUND
CU = (0, 0, 1, 4, 4, 9, 16, 33)                    # boundaries, cut at total_T: empty sequences first and in the middle (and last, below)
SLOTS = (2, 0, 0, 3, -1, 4, 1, 2)                  # live sequences 1, 2, 4, 5, 6: a duplicate, -1 and n_slots = 4 (zero tokens), slot 1
N_SLOTS = 4
# many tiles: 4100 rows (257 tiles, the last of 4 rows) at the narrowest width, 40 sequences over a pool of 8 slots
MANY_WIDTH, MANY_T, MANY_SLOTS = W64, 4100, 8


@functools.lru_cache(maxsize=None)
def many_batch():
    """(cu, slots) of the many-tiles case: 36 boundaries drawn over the whole range (not multiples of 16, by the assertions of the tests
    that use them), sequences empty first, in the middle and last, slots in [-1, MANY_SLOTS] -- duplicates, -1 and MANY_SLOTS itself, both
    outside the pool."""
    g = torch.Generator().manual_seed(41)
    cuts = sorted(set(torch.randint(1, MANY_T, (36,), generator=g).tolist()))
    half = len(cuts) // 2
    cu = [0, 0] + cuts[:half] + [cuts[half - 1]] + cuts[half:] + [MANY_T, MANY_T]
    slots = torch.randint(-1, MANY_SLOTS + 1, (len(cu) - 1,), generator=g).tolist()
    return tuple(cu), tuple(slots)


def cu_of(total_T):
    return [min(v, total_T) for v in CU] + [total_T]


def rne_bf16(v):
    """fp64 -> the nearest bf16 value (ties to even), as fp64: one rounding, not the two of a conversion through fp32."""
    m, e = torch.frexp(v)
    return torch.where(torch.isfinite(v), torch.ldexp(torch.round(m * 256) / 256, e), v)


def rne_f32(v):
    return v.to(torch.float32).to(F64)


def ident(v):
    return v


def ulp(v):
    """2^(floor(log2 |v|) - 7): the spacing of bf16 at v; 0 at 0."""
    _, e = torch.frexp(v.abs())
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - 8))


# The seed of a width's inputs, where it is not 0.  At (4096, 32, 64) the fp32-accumulating EMULATION itself (no kernel) lies 2.624, 1.002
# and 3.950 bounds (k = 1) from the restatement under seeds 0, 1 and 2 -- one flipped `low` element under 4096-term sums moves many
# outputs -- and 0.997 under seed 3, the first that can serve as a yardstick (tools/lowrank_parity.py; test_lowrank_cpu.py guards it).
SEEDS = {W4096_NARROW: 3}


def make_inputs(C, D, Dd, rows, n_front=N_SLOTS, seed=None, w2_scale=0.25, N=None):
    """The inputs of the parity cases as bf16 CPU tensors: x, front ~ N(0, 1); maa_x, maa5 ~ U(0, 1); W1, D1 ~ N(0, 1) / sqrt(C); W2 ~
    N(0, 0.25) / sqrt(D), D2 ~ N(0, 0.25) / sqrt(Dd); time_decay ~ N(-5, 1).  (N(0, s): standard deviation s.)  N: dim_att, the columns of
    D2 and the length of time_decay (None: C, and the values are those of the call without N).  seed None: SEEDS' for the width, else 0."""
    N = C if N is None else N
    seed = SEEDS.get((C, D, Dd), 0) if seed is None else seed
    g = torch.Generator().manual_seed(seed * 1000003 + C * 131 + rows + (0 if N == C else N * 8191))
    n = lambda *s: torch.randn(*s, generator=g)
    u = lambda *s: torch.rand(*s, generator=g)
    bf = torch.bfloat16
    return dict(x=n(rows, C).to(bf), front=n(n_front, C).to(bf), maa_x=u(C).to(bf), maa5=u(5, C).to(bf),
                W1=(n(C, 5 * D) / math.sqrt(C)).to(bf), W2=(n(5, D, C) * w2_scale / math.sqrt(D)).to(bf),
                D1=(n(C, Dd) / math.sqrt(C)).to(bf), D2=(n(Dd, N) * w2_scale / math.sqrt(Dd)).to(bf),
                time_decay=(n(N) - 5).to(bf))


def kernel_weights(p):
    """W1t [5 D, C], W2t [5, C, D], D1t [Dd, C], D2t [N, Dd]: the matrices in nn.Linear layout, as the C ABI takes them."""
    return (p["W1"].t().contiguous(), p["W2"].transpose(1, 2).contiguous(), p["D1"].t().contiguous(), p["D2"].t().contiguous())


def token_in_front(x, cu=None, front=None, slots=None, n_seq=None):
    """xp [rows, C] by the row rule of include/wkv6_amd.h.  cu: a list of ints (None: dense, n_seq sequences of rows / n_seq rows); front
    [n_slots, C] or None; slots: a list of ints or None (slot = sequence index)."""
    rows = x.shape[0]
    xp = torch.zeros_like(x)
    for t in range(rows):
        if cu is None:
            T = rows // n_seq
            s, first = t // T, t % T == 0
        else:
            s = max([i for i in range(len(cu) - 1) if cu[i] <= t], default=-1)
            first = s >= 0 and cu[s] == t
        if not first:
            if t > 0:
                xp[t] = x[t - 1]
        elif front is not None:
            sl = s if slots is None else slots[s]
            if 0 <= sl < front.shape[0]:
                xp[t] = front[sl]
    return xp


def _lerp(x, d, wgt, r16, r32):
    """bf16(fmaf(d, wgt, x)) with d and wgt fp32 values: the product of two fp32 values is exact in fp64."""
    return r16(r32(d * wgt + x))


def restate_tmix(p, xp, rounded=True, matmul=None):
    """(out [5, rows, C], corr [5, rows, C], d = fp32(xp - x)) in fp64.  rounded: the four rounding points to bf16 (lead, the product in
    front of tanh, low, corr) and the fp32 arithmetic of the two lerps (csrc/wkv6_mix.hip: lerp_store); False: plain fp64.  matmul(a, b):
    the contraction (default: fp64)."""
    r16, r32 = (rne_bf16, rne_f32) if rounded else (ident, ident)
    mm = matmul or (lambda a, b: a @ b)
    x, xp = p["x"].to(F64), xp.to(F64)
    rows, C = x.shape
    d = r32(xp - x)
    lead = _lerp(x, d, p["maa_x"].to(F64), r16, r32)
    low = r16(torch.tanh(r16(mm(lead, p["W1"].to(F64)))))
    low5 = low.view(rows, 5, -1).transpose(0, 1)
    corr = torch.stack([r16(mm(low5[s].contiguous(), p["W2"][s].to(F64))) for s in range(5)])
    out = _lerp(x, d, r32(p["maa5"].to(F64).view(5, 1, C) + corr), r16, r32)
    return out, corr, d


def restate_decay(p, xw, rounded=True, matmul=None, N=None):
    """(w [rows, N], corr [rows, N]) in fp64 of xw (a bf16 tensor [rows, C]).  N: dim_att, the width of D2 [Dd, N] and time_decay [N]
    (None: C)."""
    N = xw.shape[-1] if N is None else N
    assert p["D1"].shape[0] == xw.shape[-1] and p["D2"].shape[1] == N and p["time_decay"].numel() == N
    r16 = rne_bf16 if rounded else ident
    mm = matmul or (lambda a, b: a @ b)
    low = r16(torch.tanh(r16(mm(xw.to(F64), p["D1"].to(F64)))))
    corr = r16(mm(low, p["D2"].to(F64)))
    return r16(p["time_decay"].to(F64) + corr), corr


# ---- fp32-accumulating emulations of the contractions: what a kernel or a BLAS does, in three summation orders
def mm_f32_torch(a, b):
    return (a.float() @ b.float()).to(F64)


def mm_f32_reversed(a, b):
    return (a.float().flip(1).contiguous() @ b.float().flip(0).contiguous()).to(F64)


def mm_f32_chunks4(a, b):
    a, b = a.float(), b.float()
    acc = a[:, 0::4].contiguous() @ b[0::4].contiguous()
    for q in (1, 2, 3):
        acc = acc + a[:, q::4].contiguous() @ b[q::4].contiguous()
    return acc.to(F64)


ORDERS = {"torch": mm_f32_torch, "K reversed": mm_f32_reversed, "K in 4 interleaved chunks": mm_f32_chunks4}


def bound_out(b, corr, d, k):
    return ulp(b) + k * d.abs() * ulp(corr)


def bound_w(b, corr, k):
    return ulp(b) + k * ulp(corr)


# ---- the input sets of the parity checks: one place for the GPU tests, the CPU guard of the yardstick and tools/lowrank_parity.py
def tmix_case(C, D, Dd, total_T, w2_scale=0.25):
    """A parity case of the lerp pair and of the decay behind it (dim_att = C): the inputs p, the batch (cu, slots; n_front pool rows), the
    restatement's out, corr, d = fp32(xp - x), xw = bf16 of its plane 0 (the decay's input), w and corr_w.  total_T = MANY_T: the batch of
    many_batch(); every other total_T: CU / SLOTS."""
    cu, slots, n_front = (*many_batch(), MANY_SLOTS) if total_T == MANY_T else (cu_of(total_T), SLOTS, N_SLOTS)
    p = make_inputs(C, D, Dd, total_T, n_front=n_front, w2_scale=w2_scale)
    xp = token_in_front(p["x"], list(cu), p["front"], list(slots))
    out, corr, d = restate_tmix(p, xp)
    xw = out[0].to(torch.bfloat16)
    w, corr_w = restate_decay(p, xw)
    return dict(p=p, cu=list(cu), slots=list(slots), xp=xp, out=out, corr=corr, d=d, xw=xw, w=w, corr_w=corr_w)


def decay_case(C, N, Dd, rows, w2_scale=0.25):
    """A parity case of the decay alone with dim_att N: xw = the x of make_inputs(C, 32, Dd, rows, N=N)."""
    p = make_inputs(C, 32, Dd, rows, N=N, w2_scale=w2_scale)
    w, corr_w = restate_decay(p, p["x"], N=N)
    return dict(p=p, xw=p["x"], w=w, corr_w=corr_w)


TMIX_CASES = tuple((C, D, Dd, rows) for C, D, Dd in WIDTHS for rows in ROWS) + (MANY_WIDTH + (MANY_T,),)
DECAY_NC_CASES = tuple((C, N, Dd, rows) for C, N, Dd in DECAY_CASES for rows in ROWS)


def emulate_tmix(case, mm):
    """(share, ratio at k = 1) of out and of w: the chain of a tmix_case with its contractions taken by mm, against the restatement."""
    got, _, _ = restate_tmix(case["p"], case["xp"], matmul=mm)
    return compare(got, case["out"], bound_out(case["out"], case["corr"], case["d"], 1.0)) + emulate_decay(case, mm)


def emulate_decay(case, mm):
    gw, _ = restate_decay(case["p"], case["xw"], matmul=mm, N=case["w"].shape[1])
    return compare(gw, case["w"], bound_w(case["w"], case["corr_w"], 1.0))


def compare(got, b, bound1):
    """got against the restatement b (both fp64 holding bf16 values): (share of elements whose bits differ, +-0 counted as equal; the
    largest |got - b| / (bound at k = 1) among them, 0 if none)."""
    differ = got != b                                  # equal values of bf16 are equal bits, except +-0, which count as equal
    differ |= torch.isnan(got) != torch.isnan(b)
    if not bool(differ.any()):
        return 0.0, 0.0
    ratio = ((got - b).abs() / bound1)[differ]
    return float(differ.double().mean()), float(ratio.max())


def assert_parity(got, b, bound, what):
    """The two assertions of the parity check: at most CAP of the elements differ from the restatement in their bits, and each that does
    lies within its bound."""
    got = got.to(F64)
    assert not bool(torch.isnan(got).any()) and not bool(torch.isnan(b).any()), what
    differ = got != b
    share = float(differ.double().mean())
    worst = float(((got - b).abs() / bound)[differ].max()) if bool(differ.any()) else 0.0
    print(f"{what}: {share * 100:.4f} % of the elements differ from the restatement, worst |diff| / bound = {worst:.3f}")
    assert share <= CAP, f"{what}: {share * 100:.4f} % of the elements differ from the restatement in their bits (cap {CAP * 100} %)"
    assert worst <= 1.0, f"{what}: an element lies {worst:.3f} bounds from the restatement"
