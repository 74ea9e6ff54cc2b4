"""The packed pooling kernels (csrc/wkv6_pool.hip through mix_op.pool_packed) against the fp64 statement of the operation
(tests/pool_common.py) under the suite's bf16 contract, forward and backward, plus what the header promises beyond the numbers: "lasttoken"
bit-exact, a sequence's row the same bits alone and in the batch, equal bits from equal calls, rows outside every sequence and past a_s
never read and written +0 by the backward, the clamping rule, a non-default stream.

Widths: 64 and 192 (one workgroup per sequence, a partly idle wave), and 2056 = 4 * 512 + 8 -- five column workgroups per sequence, the last
with one live lane, and 257 sixteen-byte chunks a row, one more than the backward's 256 threads.  Lengths: pool_common.LENS; the forward has
no token split over workgroups, its waves interleave tokens by 4 and unroll by 16, which 1, 2, 7, 63, 64, 65, 130 and 300 all cross."""
import numpy as np
import pytest
import torch

from pool_common import KINDS, LENS, WIDTHS, f64, problem, spans
from rwkv_lm_ext_amd import callers, mix_op
from test_pool_packed_cpu import check_backward, check_forward

pytestmark = pytest.mark.gpu
DEV = "cuda"
ACTUAL = [0, 1, 40, 63, 64, 77, 0, 3, 299]


def bits(t):
    return t.contiguous().view(torch.int16)


def run(x, cu, actual, kind, gout=None):
    """(out, gx) on the GPU, back on the host"""
    xg = x.to(DEV).requires_grad_(gout is not None)
    out = mix_op.pool_packed(xg, cu.to(DEV), None if actual is None else actual.to(DEV), kind)
    if gout is None:
        return out.cpu(), None
    out.backward(gout.to(DEV))
    return out.detach().cpu(), xg.grad.cpu()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", WIDTHS + [2056])
def test_forward_and_backward_against_fp64(C, kind):
    x, gout, cu = problem(C, seed=3 + C)
    for act in (None, torch.tensor(ACTUAL, dtype=torch.int32)):
        out, gx = run(x, cu, act, kind, gout)
        assert out.dtype == torch.bfloat16 and tuple(out.shape) == (len(LENS), C) and gx.shape == x.shape
        check_forward(out, x, cu, act, kind)                     # "lasttoken": bit-exact
        check_backward(gx, gout, cu, act, kind)
        again, gx2 = run(x, cu, act, kind, gout)                 # two calls, equal bits
        assert torch.equal(bits(out), bits(again)) and torch.equal(bits(gx), bits(gx2))


@pytest.mark.parametrize("kind", KINDS)
def test_a_sequence_alone_gives_the_bits_it_gives_in_the_batch(kind):
    C = 2056
    x, gout, cu = problem(C, seed=31)
    act = torch.tensor(ACTUAL, dtype=torch.int32)
    out, gx = run(x, cu, act, kind, gout)
    for s, (start, n, a) in enumerate(spans(cu.numpy(), act.numpy(), x.shape[0])):
        if n == 0:
            continue
        # alone at the front of its own buffer, and alone behind 5 rows that belong to nothing
        for front in (0, 5):
            xs = torch.cat([torch.full((front, C), float("nan"), dtype=x.dtype), x[start:start + n]])
            one, gone = run(xs, torch.tensor([front, front + n], dtype=torch.int32), act[s:s + 1], kind, gout[s:s + 1])
            assert torch.equal(bits(one[0]), bits(out[s])), (s, front)
            assert torch.equal(bits(gone[front:]), bits(gx[start:start + n])), (s, front)


@pytest.mark.parametrize("kind", KINDS)
def test_gap_rows_and_rows_past_a_are_never_read_and_written_zero(kind):
    lens, front, back, C = [7, 0, 12, 300, 3], 3, 5, 192
    x, gout, cu = problem(C, seed=32, lens=lens, front=front, back=back)
    act = torch.tensor([4, 0, 7, 150, 2], dtype=torch.int32)
    assert int(cu[0]) > 0 and int(cu[-1]) < x.shape[0]
    clean, gclean = run(x, cu, act, kind, gout)
    poisoned = x.clone()
    poisoned[:front] = float("nan")
    poisoned[-back:] = float("nan")
    dead = torch.ones(x.shape[0], dtype=torch.bool)
    for (start, n, a) in spans(cu.numpy(), act.numpy(), x.shape[0]):
        poisoned[start + a + 1:start + n] = float("nan")
        dead[start:start + a + 1] = False
    out, gx = run(poisoned, cu, act, kind, gout)
    assert torch.equal(bits(out), bits(clean)) and out.isfinite().all()
    assert torch.equal(bits(gx), bits(gclean))
    assert (bits(gx[dead]) == 0).all()                           # +0, not -0: every gap row, every row past a_s, the empty sequence
    check_forward(out, x, cu, act, kind)
    check_backward(gx, gout, cu, act, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_the_clamping_rule_as_the_eager_path_has_it(kind):
    """The cases of test_pool_packed_cpu.test_the_clamping_rule.  Against the kernels on the clamped values: equal bits.  Against the eager
    path: the same NaN rows, and values within one bf16 ulp -- both are fp32 sums of at most 9 terms rounded once, in different orders, so
    they can part only where the sum lies at a rounding boundary."""
    lens = [5, 9, 4, 6]
    x, _, cu = problem(64, seed=21, lens=lens)
    for actual in ([-1, 9, 2, 1 << 30], [4, -(1 << 31), 4, 6], [3, 8, 100, 5], None):
        act = None if actual is None else torch.tensor(actual, dtype=torch.int32)
        out, _ = run(x, cu, act, kind)
        check_forward(out, x, cu, act, kind)
        clamped = torch.tensor([n - 1 if actual is None else min(max(a, 0), n - 1) for a, n in zip(actual or lens, lens)], dtype=torch.int32)
        assert torch.equal(bits(out), bits(run(x, cu, clamped, kind)[0]))
        eager = callers.pooling_packed(x, cu, act, kind, kernels=False)
        assert torch.equal(out.isnan(), eager.isnan())
        a, b = out.float().nan_to_num(0.0), eager.float().nan_to_num(0.0)
        ulp = b.abs().clamp_min(1e-30).log2().floor().exp2() * 2.0 ** -7
        assert ((a - b).abs() <= ulp).all()
    over = cu.clone()
    over[-1] = x.shape[0] + 50                                   # an entry past total_T is clamped before anything is formed from it
    assert torch.equal(bits(run(x, over, None, kind)[0]), bits(run(x, cu, None, kind)[0]))


def test_a_zero_gives_nan_and_the_neighbours_stay_finite():
    lens = [6, 1, 8, 5]
    x, gout, cu = problem(64, seed=22, lens=lens)
    act = torch.tensor([5, 0, 0, 4], dtype=torch.int32)
    for kind in ("weightedmean", "avg"):
        out, gx = run(x, cu, act, kind, gout)
        assert out[1].isnan().all() and out[2].isnan().all() and out[0].isfinite().all() and out[3].isfinite().all()
        check_forward(out, x, cu, act, kind)
        check_backward(gx, gout, cu, act, kind)


def test_a_non_default_stream_and_the_callers_routing():
    x, gout, cu = problem(192, seed=33)
    want, gwant = run(x, cu, None, "weightedmean", gout)
    stream = torch.cuda.Stream()
    xg, cg, gg = x.to(DEV).requires_grad_(), cu.to(DEV), gout.to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        out = mix_op.pool_packed(xg, cg, None, "weightedmean")
        out.backward(gg)
    stream.synchronize()
    assert torch.equal(bits(out.detach().cpu()), bits(want)) and torch.equal(bits(xg.grad.cpu()), bits(gwant))
    # callers.pooling_packed: the kernels where they apply (None), the 3-d form, and the eager path for what they do not serve
    with torch.no_grad():
        assert torch.equal(bits(callers.pooling_packed(xg.unsqueeze(0), cg).cpu()), bits(want))
        assert torch.equal(bits(callers.pooling_packed(xg, cg, kernels=True).cpu()), bits(want))
        eager = callers.pooling_packed(xg.float(), cg)          # fp32: eager, on the GPU
        assert eager.dtype == torch.bfloat16 and eager.is_cuda
        check_forward(eager.cpu(), x, cu, None, "weightedmean")
    with pytest.raises(RuntimeError, match="x must be a bf16"):
        callers.pooling_packed(xg.float(), cg, kernels=True)
