"""GPU tier of the LM-head cross-entropy kernels (include/wkv6_amd.h: wkv6_ce_rows_forward_* / _backward_*; csrc/wkv6_ce.hip) against
the fp64 statement of tests/ce_common.py.

Bounds: |loss_row - oracle| <= 1e-5 (+ 2^-22 |lse| for the row scaled to +-1e4), zmax and imax exact,
|g - g64| <= rel |g64| + 1e-7 |ce_scale| with rel = 2^-8 (bf16), 2^-11 (fp16), 2e-5 (fp32).  Every case prints its largest error and the
share of the bound that it takes before it asserts."""
import numpy as np
import pytest
import torch

from ce_common import DTYPES, IGNORE, ROWS, SUFFIX, VOCABS, ce_ref, check_grad, check_stats, f64, problem, scaled_rows

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _stats(n):
    f = torch.empty((3, n), device=DEV, dtype=torch.float32)
    return f[0], f[1], f[2], torch.empty(n, device=DEV, dtype=torch.int32)


def forward(z, V, targets, ce=None, l2=None, g=None):
    """(loss, lse, zmax, imax) of the rows z[:, :V] of a contiguous z [n, ld]; g: the fused mode writes the gradient there."""
    from rwkv_lm_ext_amd.mix_op import _call, _ptrs
    assert z.is_contiguous() and (g is None or g.is_contiguous())
    out = _stats(z.shape[0])
    _call("wkv6_ce_rows_forward_" + SUFFIX[z.dtype], "ce forward", z.device, z.shape[0], V, z.shape[1],
          *_ptrs(z, targets, *out, ce, l2, g), 0 if g is None else g.shape[1])
    return out


def backward(z, V, targets, stats, ce, l2, g):
    from rwkv_lm_ext_amd.mix_op import _call, _ptrs
    assert z.is_contiguous() and g.is_contiguous()
    _call("wkv6_ce_rows_backward_" + SUFFIX[z.dtype], "ce backward", z.device, z.shape[0], V, z.shape[1],
          *_ptrs(z, targets, *stats[1:], ce, l2, g), g.shape[1])
    return g


def padded(z):
    """z [n, V] as a contiguous [n, ld] with ld the next multiple of 8 (the padding holds a finite filler that must not matter)"""
    n, V = z.shape
    out = torch.full((n, (V + 7) // 8 * 8), 3.0, dtype=z.dtype)
    out[:, :V] = z
    return out


def on_gpu(V, n_rows, dtype, seed=0):
    z, targets, ce, l2, ref, tie = problem(V, n_rows, dtype, seed)
    return padded(z).to(DEV), targets.to(DEV), ce.to(DEV), l2.to(DEV), ref, tie


def bits(t):
    return t.reshape(-1).contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("dtype", DTYPES, ids=SUFFIX.get)
@pytest.mark.parametrize("n_rows", ROWS)
@pytest.mark.parametrize("V", VOCABS)
def test_statistics_and_gradient_against_fp64(V, n_rows, dtype):
    z, targets, ce, l2, ref, tie = on_gpu(V, n_rows, dtype)
    stats = forward(z, V, targets)
    check_stats(*stats, ref, scaled_rows(n_rows))
    if tie is not None:
        assert int(stats[3][0]) == tie[0] and float(stats[2][0]) == 24.0          # the lower of the two tied columns
    if n_rows >= 3:
        assert float(stats[0][2]) == 0.0 and not np.signbit(float(stats[0][2]))    # the ignored row
    g = torch.full_like(z, 7.0)
    backward(z, V, targets, stats, ce, l2, g)
    check_grad(g[:, :V], ref, ce, dtype)
    assert (g[:, V:] == 7.0).all()                                                  # columns >= V are never written


@pytest.mark.parametrize("dtype", DTYPES, ids=SUFFIX.get)
@pytest.mark.parametrize("V", [9, 8200, 65560])
def test_in_place_and_fused_give_the_bits_of_forward_then_backward(V, dtype):
    z, targets, ce, l2, _, _ = on_gpu(V, 70, dtype)
    stats = forward(z, V, targets)
    g = backward(z, V, targets, stats, ce, l2, torch.empty_like(z))[:, :V]
    # in place, from stored statistics
    zi = z.clone()
    assert same_bits(backward(zi, V, targets, stats, ce, l2, zi)[:, :V], g)
    # fused, out of place and in place
    for dst in (torch.empty_like(z), None):
        zf = z.clone()
        out = zf if dst is None else dst
        fused = forward(zf, V, targets, ce, l2, out)
        assert all(same_bits(a, b) for a, b in zip(fused, stats))
        assert same_bits(out[:, :V], g)
        assert dst is None or same_bits(zf, z)


@pytest.mark.parametrize("dtype", DTYPES, ids=SUFFIX.get)
@pytest.mark.parametrize("V", [1000, 65560])
def test_a_row_alone_has_the_bits_it_has_in_a_batch_and_two_runs_agree(V, dtype):
    z, targets, ce, l2, _, _ = on_gpu(V, 70, dtype)
    g = [torch.empty_like(z) for _ in range(2)]
    run = [forward(z, V, targets, ce, l2, g[i]) for i in range(2)]
    assert all(same_bits(a, b) for a, b in zip(run[0], run[1])) and same_bits(g[0][:, :V], g[1][:, :V])
    for r in (0, 1, 2, 37, 69):
        one = torch.empty_like(z[r:r + 1])
        alone = forward(z[r:r + 1].clone(), V, targets[r:r + 1].clone(), ce[r:r + 1].clone(), l2[r:r + 1].clone(), one)
        assert all(same_bits(a, b[r:r + 1]) for a, b in zip(alone, run[0])), r
        assert same_bits(one[:, :V], g[0][r:r + 1, :V]), r


@pytest.mark.parametrize("dtype", DTYPES, ids=SUFFIX.get)
def test_nan_in_the_padding_columns_reaches_nothing(dtype):
    V, n = 1000, 5
    zc, targets, ce, l2, ref, _ = problem(V, n, dtype, seed=1, pad=24)
    z, targets, ce, l2 = zc.to(DEV), targets.to(DEV), ce.to(DEV), l2.to(DEV)
    assert z.shape[1] == V + 24 and z[:, V:].isnan().all()
    g = torch.full_like(z, 7.0)
    stats = forward(z, V, targets, ce, l2, g)
    check_stats(*stats, ref, scaled_rows(n))
    check_grad(g[:, :V], ref, ce, dtype)
    assert g[:, :V].isfinite().all() and all(s.isfinite().all() for s in stats[:3])
    assert (g[:, V:] == 7.0).all()                                                  # the sentinel
    assert z[:, V:].isnan().all()


@pytest.mark.parametrize("dtype", DTYPES, ids=SUFFIX.get)
def test_poisoned_rows_stay_alone(dtype):
    """a NaN row, a +inf row, a row of -inf, an ignored NaN row with l2_scale == 0 and a bad target: the stated outcome on the row, equal
    bits on its neighbours against the batch without them"""
    V, n = 8200, 12
    z, targets, ce, l2, _, _ = on_gpu(V, n, dtype, seed=2)
    clean_g = torch.empty_like(z)
    clean = forward(z, V, targets, ce, l2, clean_g)
    bad, t, l2b = z.clone(), targets.clone(), l2.clone()
    NAN_ROW, INF_ROW, NEG_ROW, IGNORED_NAN, HIGH, LOW, MINUS_INF_ENTRY = 1, 3, 4, 5, 7, 8, 10
    bad[NAN_ROW, 4321] = float("nan")
    bad[INF_ROW, 17] = float("inf")
    bad[NEG_ROW, :V] = float("-inf")
    bad[IGNORED_NAN, :V] = float("nan")
    t[IGNORED_NAN] = IGNORE
    l2b[IGNORED_NAN] = 0.0
    t[HIGH], t[LOW] = V, -1
    bad[MINUS_INF_ENTRY, 5] = float("-inf")                                        # p = 0 there, the row stays sound
    t[MINUS_INF_ENTRY] = 6
    g = torch.full_like(z, 7.0)
    loss, lse, zmax, imax = forward(bad, V, t, ce, l2b, g)
    for r in (NAN_ROW, INF_ROW, NEG_ROW):
        assert loss[r].isnan() and lse[r].isnan() and g[r, :V].isnan().all(), r
    assert float(loss[IGNORED_NAN]) == 0.0 and (g[IGNORED_NAN, :V] == 0).all() and not g[IGNORED_NAN, :V].signbit().any()
    for r in (HIGH, LOW):
        assert loss[r].isnan() and g[r, :V].isnan().all(), r
        assert same_bits(lse[r], clean[1][r]) and same_bits(zmax[r], clean[2][r]) and int(imax[r]) == int(clean[3][r])
    ref = ce_ref(f64(bad[MINUS_INF_ENTRY:MINUS_INF_ENTRY + 1, :V]), [6], f64(ce[MINUS_INF_ENTRY:MINUS_INF_ENTRY + 1]),
                 f64(l2[MINUS_INF_ENTRY:MINUS_INF_ENTRY + 1]))
    check_stats(loss[10:11], lse[10:11], zmax[10:11], imax[10:11], ref)
    check_grad(g[10:11, :V], ref, ce[10:11], dtype)
    assert float(g[MINUS_INF_ENTRY, 5]) == 0.0
    for r in (0, 2, 6, 9, 11):                                                      # the neighbours
        assert all(same_bits(a[r], b[r]) for a, b in zip((loss, lse, zmax, imax), clean)), r
        assert same_bits(g[r, :V], clean_g[r, :V]), r
    assert (g[:, V:] == 7.0).all()
    # the backward from stored statistics treats the same rows the same way
    gb = backward(bad, V, t, (loss, lse, zmax, imax), ce, l2b, torch.full_like(z, 7.0))
    assert torch.equal(gb.isnan(), g.isnan()) and same_bits(gb.nan_to_num(1.0), g.nan_to_num(1.0))


@pytest.mark.parametrize("dtype", DTYPES, ids=SUFFIX.get)
def test_ce_rows_under_autograd_equals_the_two_calls(dtype):
    from rwkv_lm_ext_amd import mix_op
    V, n = 1000, 70
    z, targets, ce, l2, _, _ = on_gpu(V, n, dtype)
    stats = forward(z, V, targets)
    g = backward(z, V, targets, stats, ce, l2, torch.empty_like(z))
    zr = z.clone().requires_grad_()
    loss = mix_op.ce_rows(zr, targets, l2)
    assert same_bits(loss, stats[0])
    (loss * ce).sum().backward()                                                    # the incoming gradient is ce_scale; L2 is not scaled by it
    assert same_bits(zr.grad, g)
    # a view of the first V columns of a padded tensor is taken as it is; no l2_scale = no L2 term
    wide = torch.cat([z, torch.full((n, 8), float("nan"), device=DEV, dtype=dtype)], 1)
    zv = wide[:, :V].detach().requires_grad_()
    loss = mix_op.ce_rows(zv, targets)
    assert same_bits(loss, stats[0])
    (loss * ce).sum().backward()
    assert same_bits(zv.grad, backward(z, V, targets, stats, ce, torch.zeros_like(l2), torch.empty_like(z)))
    # the fused in-place call
    zi = z.clone()
    assert same_bits(mix_op.ce_rows_grad_(zi, targets, ce, l2), stats[0]) and same_bits(zi, g)
    with pytest.raises(RuntimeError, match="no backward"):
        mix_op.ce_rows_grad_(z.clone().requires_grad_(), targets, ce, l2)


def test_lm_loss_kernels_against_eager_on_bf16():
    """The kernels on bf16 logits against the eager branch on the same values held in fp32: on bf16 tensors the eager three lines round
    the log-softmax to bf16 (percents of p), which would be the reference's error, not the kernels'.  Bounds: those of the kernels."""
    from rwkv_lm_ext_amd import callers
    B, T, V = 3, 50, 1000
    gen = torch.Generator().manual_seed(5)
    logits = (torch.randn(B, T, V, generator=gen) * 4).bfloat16().to(DEV)
    targets = torch.randint(0, V, (B, T), generator=gen).to(DEV)
    targets[0, 5:9] = IGNORE
    mask = (torch.rand(B, T, generator=gen) < 0.6).float().to(DEV)
    for kw in ({}, {"mask": mask}, {"token_amount": 77}, {"l2wrap": 0.0}):
        z = logits.clone().requires_grad_()
        loss = callers.lm_loss(z, targets, kernels=True, **kw)
        loss.backward()
        zf = logits.float().requires_grad_()
        want = callers.lm_loss(zf, targets, kernels=False, **kw)
        want.backward()
        assert loss.dtype == torch.float32 and abs(float(loss.detach()) - float(want.detach())) <= 1e-5, (kw, float(loss.detach()), float(want.detach()))
        ce, _ = callers._row_scales(targets.reshape(-1), kw.get("mask"), None, None)
        tol = 2.0 ** -8 * zf.grad.abs() + 1e-7 * ce.view(B, T, 1)
        err = (z.grad.float() - zf.grad).abs()
        print(kw.keys(), "largest share of the gradient bound", float((err / tol.clamp_min(1e-30)).max()))
        assert (err <= tol).all(), kw


def test_one_captured_graph_of_the_fused_call_replays_the_eager_bits():
    from rwkv_lm_ext_amd import mix_op
    V, n = 8200, 70
    z, targets, ce, l2, _, _ = on_gpu(V, n, torch.bfloat16)
    want_g = z.clone()
    want = mix_op.ce_rows_grad_(want_g, targets, ce, l2)
    buf, src = z.clone(), z.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        mix_op.ce_rows_grad_(buf, targets, ce, l2)                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        buf.copy_(src)
        loss = mix_op.ce_rows_grad_(buf, targets, ce, l2)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(loss, want) and same_bits(buf, want_g)
