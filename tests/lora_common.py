"""Inputs, rules and the fp64 restatement shared by the per-sequence LoRA tests (test_lora_packed_gpu.py, test_adapters_cpu.py): everything
here runs on the CPU; the references are computed once per shape and handed out unchanged."""
import functools

import numpy as np
import torch

bf = torch.bfloat16
INT_MIN = -(1 << 31)
# (K, N, R): the smallest sizes; a second MFMA tile of j and of n with R = 16 (half the contraction padded); a long K split over the
# waves with two contraction steps (R = 64); many column blocks per workgroup with R = 8 (three quarters padded); a long K with R = 32
SHAPES = [(64, 64, 8), (192, 192, 16), (2048, 64, 64), (128, 7168, 8), (7168, 128, 32)]
# (K, N, R) whose K runs BOTH loops of the shrink -- K / 32 steps in 4 interleaved chunks, 4 steps a pass (main loop), then singly
# (remainder) -- and whose N / 64 column blocks do not share out evenly over the expand's 16 workgroups: 24 steps (main once, two remainder
# steps a chunk) with R = 8 and 42 blocks (ten workgroups walk 3, six walk 2); 84 steps (main five times, a remainder step a chunk) with
# R = 16; 18 steps (main once, a remainder step for chunks 0 and 1 only) with R = 64's two expand steps and 17 blocks (workgroup 0 walks 2);
# 34 steps (main twice, a remainder step for two chunks) with R = 32.  768 is n_embd of the 0.1B model, 2688 = 3.5 * 768 its dim_ffn.
MIXED_SHAPES = [(768, 2688, 8), (2688, 768, 16), (576, 1088, 64), (1088, 64, 32)]
N_ADAPTERS = 5
LENS = [37, 1, 1, 0, 1, 16, 1, 1, 70, 1]          # runs cross tile edges (tiles of 16 rows), and tile 2 holds five sequences
ADAPTERS = [2, 0, -1, 3, 4, N_ADAPTERS, 1, INT_MIN, 2, 0]
LEAD = 3                                          # rows in front of cu_seqlens[0]: in no sequence
# total_T, neither a multiple of 16: 135 leaves three rows behind the last sequence; 130 cuts sequence 8 short, leaves sequence 9 no row and
# puts cu_seqlens[9] and cu_seqlens[10] past total_T
TOTALS = [135, 130]


# Sixteen groups in a tile, over a pool of MANY_ADAPTERS = 20.  Tile 0 is one sequence up to the tile edge; tile 1 (rows 16..31) is sixteen
# one-token sequences on sixteen distinct adapters, 16..19 among them; tile 2 (rows 32..47) holds nine groups -- single tokens, a two-row
# sequence and a row on no adapter between them -- the ninth a sequence of 30 rows that crosses the edges at 48 and 64; three rows behind it
# are in no sequence.
MANY_ADAPTERS = 20
GROUPS_LENS = [16] + [1] * 16 + [1, 1, 2, 1, 1, 1, 1, 1, 1, 30]
GROUPS_ADAPTERS = [3] + [19, 0, 18, 5, 17, 7, 16, 9, 1, 15, 2, 14, 3, 13, 4, 12] + [6, 8, 10, -1, 11, 19, 0, 17, 5, 16]
GROUPS_TOTAL = 75
GROUPS_SHAPES = [(192, 192, 16), (768, 64, 8)]
# Many tiles: 4100 rows (257 tiles) of K = N = 64, R = 8, about 60 sequences over the 20 adapters
MANY_TOTAL, MANY_SHAPE = 4100, (64, 64, 8)


@functools.lru_cache(maxsize=None)
def many_batch():
    """(cu, adapters) of the many-tiles case: boundaries drawn over the whole range behind LEAD rows of no sequence, an empty sequence in
    the middle, adapters in [-1, MANY_ADAPTERS] (-1 and MANY_ADAPTERS: no adapter) and one INT_MIN; the last rows are in no sequence."""
    g = torch.Generator().manual_seed(43)
    cuts = sorted(set(torch.randint(LEAD + 1, MANY_TOTAL - 5, (60,), generator=g).tolist()))
    half = len(cuts) // 2
    cu = [LEAD] + cuts[:half] + [cuts[half - 1]] + cuts[half:]
    adapters = torch.randint(-1, MANY_ADAPTERS + 1, (len(cu) - 1,), generator=g).tolist()
    adapters[7], adapters[11], adapters[23] = INT_MIN, MANY_ADAPTERS, -1
    return tuple(cu), tuple(adapters)


def cu_of(lens=LENS, lead=LEAD):
    return (lead + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64).tolist()


def rows_of(cu, adapters, total_T, n_adapters=N_ADAPTERS):
    """The header's rule, one sequence after the other on the host: int64 [total_T], the adapter that serves each row, -1 for none."""
    out = np.full(total_T, -1, dtype=np.int64)
    for s, a in enumerate(adapters):
        lo, hi = min(max(cu[s], 0), total_T), min(max(cu[s + 1], 0), total_T)
        if 0 <= a < n_adapters:
            out[lo:hi] = a
    return out


@functools.lru_cache(maxsize=None)
def case(K, N, R, total_T, seed=0, n_adapters=N_ADAPTERS):
    """(x, y0, A, B, scale) on the CPU: x ~ N(0,1), y0 ~ N(0,1), A ~ N(0,1) / sqrt(K), B ~ N(0,1) / sqrt(R), scale in [0.5, 4] -- with
    these the LoRA term is as large as y0."""
    g = torch.Generator().manual_seed(1000 * seed + K + 3 * N + 7 * R + total_T)
    x = torch.randn(total_T, K, generator=g).to(bf)
    y0 = torch.randn(total_T, N, generator=g).to(bf)
    A = (torch.randn(n_adapters, R, K, generator=g) / K ** 0.5).to(bf)
    B = (torch.randn(n_adapters, N, R, generator=g) / R ** 0.5).to(bf)
    scale = 0.5 + 3.5 * torch.rand(n_adapters, generator=g)
    return x, y0, A, B, scale


def restate(x, y0, A, B, scale, which):
    """(E, bound) in fp64 from the bf16 inputs' exact values: for a row on adapter a, e_j = sum_k x_k A_jk, S_j = sum_k |x_k A_jk|,
    E = y0 + scale sum_j e_j B_nj and bound = 2^-8 |E| + 2 |scale| sum_j |B_nj| (2^-9 |e_j| + K 2^-23 S_j); for a row of no adapter
    E = y0 and bound = 0.  `which`: int64 [total_T] as rows_of returns."""
    K = x.shape[1]
    x, y0, A, B, scale = (t.double() for t in (x, y0, A, B, scale))
    E, bound = y0.clone(), torch.zeros_like(y0)
    for a in range(A.shape[0]):
        rows = torch.from_numpy(np.nonzero(which == a)[0])
        if rows.numel() == 0:
            continue
        e = x[rows] @ A[a].T
        S = x[rows].abs() @ A[a].abs().T
        Ea = y0[rows] + scale[a] * (e @ B[a].T)
        E[rows] = Ea
        bound[rows] = 2.0 ** -8 * Ea.abs() + 2 * scale[a].abs() * ((2.0 ** -9 * e.abs() + K * 2.0 ** -23 * S) @ B[a].abs().T)
    return E, bound


@functools.lru_cache(maxsize=None)
def reference(K, N, R, total_T, seed=0):
    """restate() of case() under the mixed batch LENS / ADAPTERS, computed once."""
    x, y0, A, B, scale = case(K, N, R, total_T, seed)
    return restate(x, y0, A, B, scale, rows_of(cu_of(), ADAPTERS, total_T))


def worst_ratio(out, E, bound):
    """max over the elements of |out - E| / bound (0 / 0 counts as 0, anything / 0 as inf)."""
    err = (out.double() - E).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max())
