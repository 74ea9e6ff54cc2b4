"""What the packed-pooling tests share: the lengths, the fp64 statement of the operation (include/wkv6_amd.h: wkv6_pool_packed_forward /
_backward) and the problems built from them.  Not a test module."""
import numpy as np
import torch

LENS = [1, 2, 63, 64, 65, 130, 0, 7, 300]          # a_s == 0, the waves' interleave (4) and unroll (16) edges, an empty sequence, > 256 tokens
WIDTHS = [64, 192]
KINDS = ["weightedmean", "lasttoken", "avg"]


def cu_of(lens, front=0):
    return np.concatenate([[front], front + np.cumsum(lens)]).astype(np.int32)


def spans(cu, actual, total):
    """(start, len_s, a_s) per sequence by the header's rule."""
    cu = np.clip(np.asarray(cu, np.int64), 0, total)
    out = []
    for s in range(len(cu) - 1):
        n = int(np.clip(cu[s + 1] - cu[s], 0, total - cu[s]))
        a = n - 1 if actual is None else int(np.clip(int(actual[s]), 0, n - 1)) if n else -1
        out.append((int(cu[s]), n, a))
    return out


def weights(n, a, kind):
    """fp64 weight of token t = 0 .. n - 1 of a sequence with a_s = a >= 1 (0: the token is not summed)."""
    t = np.arange(n, dtype=np.float64)
    if kind == "weightedmean":
        return np.where(t <= a, (t + 1) / a / a, 0.0)
    if kind == "avg":
        return np.where(t < a, 1.0 / a, 0.0)
    return (t == a).astype(np.float64)


def pool_ref(x, cu, actual, kind):
    """fp64 out [n_seq,C] of x [total,C] (fp64): NaN rows where a_s == 0 (the means), zero rows for empty sequences; only the summed rows of x
    are touched, so NaN anywhere else cannot reach the result."""
    total, C = x.shape
    out = np.zeros((len(cu) - 1, C))
    for s, (start, n, a) in enumerate(spans(cu, actual, total)):
        if n == 0:
            continue
        if kind == "lasttoken":
            out[s] = x[start + a]
        elif a == 0:
            out[s] = np.nan
        else:
            w = weights(n, a, kind)
            live = w != 0
            out[s] = (x[start:start + n][live] * w[live, None]).sum(0)
    return out


def pool_grad_ref(gout, cu, actual, kind, total):
    """(fp64 gx [total,C], written [total] bool: rows whose weight is not zero); the weighted mean's row 0 of an a_s == 0 sequence is NaN."""
    gx = np.zeros((total, gout.shape[1]))
    hit = np.zeros(total, bool)
    for s, (start, n, a) in enumerate(spans(cu, actual, total)):
        if n == 0:
            continue
        if a == 0 and kind != "lasttoken":
            if kind == "weightedmean":
                gx[start], hit[start] = np.nan, True
            continue
        w = weights(n, a, kind)
        gx[start:start + n] = w[:, None] * gout[s]
        hit[start:start + n] = w != 0
    return gx, hit


def problem(C, seed, lens=LENS, front=0, back=0, dtype=torch.bfloat16):
    """x [total,C] and gout [n_seq,C] in `dtype` (their fp64 values are what the reference sees), cu_seqlens int32 with `front` rows in front
    of the first sequence and `back` rows behind the last that belong to none."""
    g = torch.Generator().manual_seed(seed)
    total = front + sum(lens) + back
    x = torch.randn(total, C, generator=g).to(dtype)
    gout = torch.randn(len(lens), C, generator=g).to(dtype)
    return x, gout, torch.from_numpy(cu_of(lens, front))


def f64(t):
    return t.detach().double().cpu().numpy()
