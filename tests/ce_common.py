"""What the cross-entropy tests share (tests/test_ce_rows_cpu.py, tests/test_ce_rows_gpu.py, tests/test_head_loss_gpu.py): the fp64 numpy
statement of the operation of include/wkv6_amd.h (wkv6_ce_rows_*) -- the lowest-index argmax, the ignored-row, bad-target and NaN-row rules
included -- and the list of cases with their inputs."""
import functools

import numpy as np
import torch

IGNORE = -100
VOCABS = [1, 7, 8, 9, 1000, 8200, 65536, 65560]     # one element; the tail lane around 8; several rounds of 1024 threads; past the sampler's cap
ROWS = [1, 3, 70]
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
SUFFIX = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
# the gradient's relative bound: one rounding of the output type (half an ulp) and the relative error of p; fp32: the 1e-5 bound on z - lse
REL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2e-5}
LOSS_ATOL = 1e-5


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def ce_ref(z, targets, ce_scale=None, l2_scale=None):
    """The operation in fp64.  z [n,V] (the V columns that count), targets int [n]; returns loss, lse, zmax, imax [n] and, with the two
    scales, g [n,V].  A row with a NaN, a +inf or no finite logit has lse = NaN; zmax / imax are taken over its non-NaN logits."""
    z = np.asarray(z, np.float64)
    n, V = z.shape
    t = np.asarray(targets, np.int64)
    ignored = t == IGNORE
    bad_target = ~ignored & ((t < 0) | (t >= V))
    no_nan = np.where(np.isnan(z), -np.inf, z)
    zmax = no_nan.max(1)
    imax = no_nan.argmax(1)                                         # numpy: the first occurrence, i.e. the lowest column
    sound = ~np.isnan(z).any(1) & np.isfinite(zmax)
    with np.errstate(all="ignore"):
        lse = np.where(sound, zmax + np.log(np.exp(z - zmax[:, None]).sum(1)), np.nan)
    at = np.where(ignored | bad_target, 0, t)
    loss = np.where(ignored, 0.0, np.where(bad_target, np.nan, lse - z[np.arange(n), at]))
    out = {"loss": loss, "lse": lse, "zmax": zmax, "imax": imax}
    if ce_scale is None:
        return out
    ce, l2 = np.asarray(ce_scale, np.float64), np.asarray(l2_scale, np.float64)
    with np.errstate(all="ignore"):
        p = np.exp(z - lse[:, None])
    onehot = np.zeros_like(z)
    onehot[np.arange(n), at] = 1.0
    g = np.where(ignored[:, None], 0.0, ce[:, None] * (p - onehot))
    g[np.arange(n), imax] += l2 * zmax
    g[bad_target | np.isnan(lse)] = np.nan
    g[ignored & (l2 == 0)] = 0.0
    out["g"] = g
    return out


@functools.lru_cache(maxsize=None)
def problem(V, n_rows, dtype, seed=0, pad=0):
    """(logits [n_rows, V + pad] of dtype on the CPU, targets int64, ce_scale, l2_scale fp32, the fp64 reference, the tied columns or None).
    randn * 4 logits; targets random with row 0 -> 0; from three rows on: row 0 has a tied maximum at two known columns, row 1 is scaled to
    +-1e4 and aims at V - 1, row 2 is ignored (and so is every 9th row behind it).  Cached: the inputs and the reference are made once and
    must be left unchanged."""
    gen = torch.Generator().manual_seed(1000 * V + 10 * n_rows + seed)
    z = (torch.randn(n_rows, V, generator=gen) * 4).to(dtype)
    targets = torch.randint(0, V, (n_rows,), generator=gen)
    targets[0] = 0
    tie = None
    if n_rows >= 3:
        if V >= 2:
            tie = (V // 3, V - 1)
            z[0, tie[0]] = z[0, tie[1]] = 24.0                      # above every randn * 4 draw of these sizes, exact in every type
        z[1] = (z[1].float() * (1e4 / z[1].float().abs().max().clamp_min(1e-3))).to(dtype)
        targets[1] = V - 1
        targets[2::9] = IGNORE
    ce = torch.rand(n_rows, generator=gen) + 0.5
    l2 = torch.rand(n_rows, generator=gen) * 1e-2
    if pad:
        z = torch.cat([z, torch.full((n_rows, pad), float("nan"), dtype=dtype)], 1)
    ref = ce_ref(f64(z[:, :V]), targets.numpy(), ce.numpy(), l2.numpy())
    return z, targets, ce, l2, ref, tie


def scaled_rows(n_rows):
    """the rows of problem() that are scaled to +-1e4"""
    return (1,) if n_rows >= 3 else ()


def check_stats(got_loss, got_lse, got_zmax, got_imax, ref, scaled=()):
    """loss and lse within 1e-5, on the rows named in `scaled` (the +-1e4 row) within 1e-5 + 2^-22 |lse|; zmax and imax exact."""
    tol = np.full(ref["lse"].shape, LOSS_ATOL)
    for r in scaled:
        tol[r] += 2.0 ** -22 * abs(ref["lse"][r])
    for name, got in (("loss", got_loss), ("lse", got_lse)):
        err = np.abs(f64(got) - ref[name])
        print(f"{name}: max error {err.max():.3e}, largest share of its bound {(err / tol).max():.3f}")
        assert (err <= tol).all(), (name, err.max(), int((err / tol).argmax()))
    assert np.array_equal(f64(got_zmax), ref["zmax"])
    assert np.array_equal(got_imax.cpu().numpy().astype(np.int64), ref["imax"])


def check_grad(got, ref, ce, dtype):
    """|g - g64| <= rel |g64| + 1e-7 |ce_scale|"""
    g, g64 = f64(got), ref["g"]
    tol = REL[dtype] * np.abs(g64) + 1e-7 * np.abs(f64(ce))[:, None]
    err = np.abs(g - g64)
    share = (err / tol).max()
    print(f"gradient: max error {err.max():.3e}, largest share of its bound {share:.3f} at {np.unravel_index((err / tol).argmax(), err.shape)}")
    assert (err <= tol).all(), (share, np.unravel_index((err / tol).argmax(), err.shape))
