"""Shared by the packed variable-length ("varlen") tests: the length sets, cu_seqlens, and the expectation of a packed call -- the CPU
oracle (oracle/wkv6_oracle.py) run on every sequence alone with B = 1, T = len_s, results concatenated; per-sequence gu / gs stacked."""
import numpy as np

# the edges of the 16-token block and the 64-token group / checkpoint spacing, an empty sequence in the middle
EDGE_LENS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 0, 330]
# one long sequence among fifteen of length 1
LONG_LENS = [1] * 7 + [4096] + [1] * 8
# the packed callers test (CPU tier)
CALLER_LENS = [1, 2, 63, 64, 65, 130, 0, 7]


def bench_lens(n=48, device="cpu"):
    """Row lengths as bench.py draws them for its ragged config (randint(64, 513), seed 1) -- on the CPU generator when no GPU is there:
    the exact values differ between generators, their distribution is the point."""
    import torch
    g = torch.Generator(device=device).manual_seed(1)
    return [int(x) for x in torch.randint(64, 513, (n,), device=device, generator=g).cpu()]


def cu_of(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int32)


def exact_workspace_need(lens, H):
    """Bytes the kernels touch: sum_s ceil(len_s / 64) checkpoint slots of 16 KB per head + four int32 arrays (256-byte aligned)."""
    slots = sum((int(n) + 63) // 64 for n in lens)
    ints = (4 * len(lens) * 4 + 255) // 256 * 256
    return ints + H * slots * 64 * 64 * 4


def oracle_packed(oracle, r, k, v, w, u, gy, lens, s0=None, heads=None):
    """Expectation of a packed call from the oracle, per sequence.  r, k, v, w, gy: float32 numpy [total_T, C]; u [H,N]; s0 None, [H,N,N]
    or [n_seq,H,N,N].  heads: restrict to these heads (list), to keep the oracle's time down on wide problems.
    Returns dict y, gr, gk, gv, gw [total_T, C'], gu [n_seq, C'], s_out, gs [n_seq, H', N, N] (zero-length: s_out = s0, gu = gs = 0)."""
    C = r.shape[1]
    H = C // 64
    heads = list(range(H)) if heads is None else list(heads)
    cols = np.concatenate([np.arange(64 * h, 64 * h + 64) for h in heads])
    Hs = len(heads)
    total = r.shape[0]
    out = {n: np.zeros((total, 64 * Hs), np.float32) for n in ("y", "gr", "gk", "gv", "gw")}
    out["gu"] = np.zeros((len(lens), 64 * Hs), np.float32)
    out["s_out"] = np.zeros((len(lens), Hs, 64, 64), np.float32)
    out["gs"] = np.zeros((len(lens), Hs, 64, 64), np.float32)
    us = np.ascontiguousarray(u[heads])
    t0 = 0
    for s, n in enumerate(lens):
        s0s = None
        if s0 is not None:
            s0s = np.ascontiguousarray((s0[s] if s0.ndim == 4 else s0)[heads])
        if n == 0:
            if s0s is not None:
                out["s_out"][s] = s0s
            continue
        sl = slice(t0, t0 + n)
        a = [np.ascontiguousarray(x[sl][:, cols][None]) for x in (r, k, v, w)]
        g = np.ascontiguousarray(gy[sl][:, cols][None])
        y, so = oracle.forward(*a, us, s0=s0s, return_state=True)
        og = oracle.backward(*a, us, g, s0=s0s)
        out["y"][sl] = y[0]
        for nm in ("gr", "gk", "gv", "gw"):
            out[nm][sl] = og[nm][0]
        out["gu"][s] = og["gu_b"][0].reshape(-1)
        out["s_out"][s] = so.reshape(Hs, 64, 64)
        if s0s is not None:
            out["gs"][s] = og["gs_b"][0]
        t0 += n
    return out


# ---- many sequences: past the 256 threads of the one-workgroup preparation kernel, where a thread owns more than one sequence ----------
MANY_N_SEQ = (256, 257, 513, 600)
MANY_CHOICES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 130]


def many_lens(n_seq):
    """n_seq lengths around the 16-token block and the 64-token checkpoint spacing, about a tenth of them empty."""
    return [int(x) for x in np.random.default_rng(20).choice(MANY_CHOICES, n_seq)]


# every non-empty length equal (the ranking's tie-break `o < s` alone decides the order), a run of empty sequences at either end
TIE_LENS = [0] * 100 + [64] * 100 + [0] * 100
MANY_SETS = {**{str(n): many_lens(n) for n in MANY_N_SEQ}, "ties": TIE_LENS}


def prepare_model(cu, total_T, max_seqlen, ck_stride):
    """What the device-side preparation derives from cu_seqlens (include/wkv6_amd.h), restated in numpy:
    tok_off = clamp(cu[s], 0, total_T); lens = clamp(cu[s+1] - cu[s], 0, max_seqlen), cut so that the row ends at or before total_T;
    ck_off = exclusive prefix sum of ceil(lens / 64) (a sequence whose slots would pass ck_stride gets length 0 -- never for a
    non-decreasing cu_seqlens); order = the sequences by decreasing length, ties by index (a stable sort).
    Returns int32 arrays lens, tok_off, ck_off, order."""
    cu = np.asarray(cu, np.int64)
    n_seq = len(cu) - 1
    tok_off = np.clip(cu[:-1], 0, total_T)
    lens = np.minimum(np.clip(cu[1:] - cu[:-1], 0, max_seqlen), total_T - tok_off)
    ck_off = np.zeros(n_seq, np.int64)
    off = 0
    for s in range(n_seq):
        n = (int(lens[s]) + 63) // 64
        if off + n > ck_stride:
            lens[s], n = 0, 0
        ck_off[s] = off
        off += n
    order = np.argsort(-lens, kind="stable")
    return tuple(a.astype(np.int32) for a in (lens, tok_off, ck_off, order))
