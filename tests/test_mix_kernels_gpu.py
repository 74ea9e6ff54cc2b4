"""The fused mix kernels of csrc/wkv6_mix.hip at the row counts training uses, against the same formulas in fp64 torch on the
same bf16 inputs: the ddlerp backward's run split and register hand-over (plain stream) and its grid-stride loop (reversed
stream), the gn_gate backward's grid-stride loop, the grid-stride loops of sqrelu / sigmul past one full grid, 16- and
1024-thread workgroups, and degenerate GroupNorm heads.

Contract (as tests/test_mix_gpu.py): outputs within 1.01 bf16 ulp of RNE_bf16(fp64) in bf16_report terms (rel-rms <= 2e-3),
dx / dy within 1.5.  fp32 parameter-gradient partial rows, summed in fp64, within K_PART 2^-24 sum|terms| per channel of the
fp64 gradient; the bf16 sums mix_op returns within 1.01 ulp.

Calls that vary nparts, or need their outputs poisoned, go through the C ABI; every such call fills all its outputs with NaN
first, must leave none, must leave the partial rows of workgroups without rows at exactly 0 and must repeat bit for bit."""
import pytest
import torch

from oracle.contract import bf16_report_torch

pytestmark = pytest.mark.gpu
bf, f32, f64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
# Partial rows: each term is formed with at most two fp32 roundings (ddlerp: d (xp - x); gn: (y - mean) rstd, times d g) and the
# fp32 statistics are within a few U; a workgroup then adds its terms one after another in fp32.  For zero-mean terms the
# rounding errors of such a sum have a standard deviation of about U/2 sum|terms| whatever the number of terms, so 32 leaves a
# margin of several standard deviations over thousands of channels.  Every shape below also checks that one row omitted or
# counted twice would exceed this bound at least 10x (check_detectable).
K_PART = 32
INST = [(1, False), (5, True), (1, True), (2, False)]          # the four (NS, m given) instantiations of dispatch_lerp
EPS = 6.4e-4                                                   # ln_x eps of the model: 1e-5 * head_size_divisor^2


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(bf)


def poisoned(*shape, dtype=bf):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def close(out, ref, what, ulps=1.01, rms=2e-3):
    r, off, u = bf16_report_torch(out, ref)
    assert r <= rms and u <= ulps, f"{what}: rel-rms {r:.2e}, {u:.2f} ulp, {off * 100:.1f}% not correctly rounded"


def no_nan(what, *ts):
    for t in ts:
        if t is not None:
            assert not bool(torch.isnan(t).any()), f"{what}: NaN left in an output (a row was not written)"


def check_partials(part, terms, what, empty=()):
    """part fp32 [nparts, ..., C]; terms fp64 [rows, ..., C].  The partial rows summed in fp64 against the fp64 sum, per channel;
    the rows of workgroups that own no rows exactly 0."""
    got = part.double().sum(0)
    want = terms.sum(0)
    bound = K_PART * U * terms.abs().sum(0)
    err = (got - want).abs()
    assert bool((err <= bound).all()), f"{what}: partial sums off by {float((err / bound.clamp_min(1e-300)).max()):.1f}x the bound"
    if len(empty):
        assert bool((part[list(empty)] == 0).all()), f"{what}: partial rows of workgroups without rows are not 0"
    return bound


def check_detectable(terms, bound, what):
    """One row left out or counted twice moves some channel by at least 10x the bound."""
    flat = terms.abs().reshape(terms.shape[0], -1)
    ratio = (flat / bound.reshape(1, -1).clamp_min(1e-300)).amax(1)
    assert float(ratio.min()) >= 10.0, f"{what}: a missing row would move the sums by only {float(ratio.min()):.1f}x the bound"


# ---- ddlerp -------------------------------------------------------------------------------------------------------------------
def prev_index(B, T, rev_n):
    """[B, T] int64: the token one stream position before token t, -1 for the token in front of the row.  The stream of row b is
    its first rev_n[b] (clamped to [0, T]) tokens reversed, then the rest in place."""
    t = torch.arange(T, device="cuda").view(1, T).expand(B, T)
    if rev_n is None:
        return t - 1
    n = rev_n.long().clamp(0, T).view(B, 1)
    order = torch.where(t < n, n - 1 - t, t)                    # stream position -> token
    prev = torch.empty(B, T, dtype=torch.long, device="cuda")
    before = torch.cat([torch.full((B, 1), -1, device="cuda", dtype=torch.long), order[:, :-1]], 1)
    prev.scatter_(1, order, before)
    return prev


def ddlerp_ref(x, maa, m, s0, rev_n, dout=None):
    """fp64: out[s] = x + (xp - x) (maa[s] + m[s]) and, given dout, (dx, dm terms [rows, NS, C], d shifted0)."""
    B, T, C = x.shape
    NS = maa.shape[0]
    prev = prev_index(B, T, rev_n)
    front = torch.zeros(B, 1, C, dtype=f64, device="cuda") if s0 is None else s0.double().view(B, 1, C)
    xd = x.double()
    xpad = torch.cat([front, xd], 1)
    xx = torch.gather(xpad, 1, (prev + 1).view(B, T, 1).expand(B, T, C)) - xd
    c = maa.double().view(NS, 1, 1, C) + (0.0 if m is None else m.double())
    out = xd + xx * c
    if dout is None:
        return out
    d = dout.double()
    dx = (d * (1.0 - c)).sum(0)
    hand = torch.zeros(B, T + 1, C, dtype=f64, device="cuda")
    hand.scatter_add_(1, (prev + 1).view(B, T, 1).expand(B, T, C), (d * c).sum(0))
    dx += hand[:, 1:]
    dm = d * xx                                                 # [NS, B, T, C]: also the terms of dmaa
    return out, dx, dm, hand[:, 0]


def lerp_fwd_abi(lib, x, maa, m, s0, rev_n):
    B, T, C = x.shape
    out = poisoned(maa.shape[0], B, T, C)
    assert lib.wkv6_ddlerp_rev_forward(B, T, C, maa.shape[0], ptr(x), ptr(s0), ptr(m), ptr(maa), ptr(rev_n), ptr(out), stream()) == 0
    torch.cuda.synchronize()
    return out


def lerp_bwd_abi(lib, x, maa, m, s0, rev_n, dout, nparts):
    B, T, C = x.shape
    NS = maa.shape[0]
    dx, dm, part = poisoned(B, T, C), (None if m is None else poisoned(NS, B, T, C)), poisoned(nparts, NS, C, dtype=f32)
    rc = lib.wkv6_ddlerp_rev_backward(B, T, C, NS, ptr(x), ptr(s0), ptr(m), ptr(maa), ptr(rev_n), ptr(dout), ptr(dx), ptr(dm),
                                      ptr(part), nparts, stream())
    assert rc == 0
    torch.cuda.synchronize()
    return dx, dm, part


def empty_parts(rows, nparts, plain):
    """Workgroups that own no rows: plain stream, contiguous runs of ceil(rows / nparts); reversed stream, rows p, p + nparts, ..."""
    if plain:
        per = -(-rows // nparts)
        return [p for p in range(nparts) if p * per >= rows]
    return list(range(rows, nparts))


def lerp_inputs(B, T, C, NS, has_m, with_s0, seed):
    x = rnd(B, T, C, seed=seed)
    maa = rnd(NS, C, scale=0.5, seed=seed + 1)
    m = rnd(NS, B, T, C, scale=0.3, seed=seed + 2) if has_m else None
    s0 = rnd(B, C, seed=seed + 3) if with_s0 else None
    dout = rnd(NS, B, T, C, seed=seed + 4)
    return x, maa, m, s0, dout


def run_lerp_case(lib, x, maa, m, s0, rev_n, dout, nparts_list, what):
    """Forward and backward through the ABI at every nparts: poisoning, repeatability, fp64 bounds, partial sums; returns the
    backward results per nparts."""
    B, T, C = x.shape
    rows = B * T
    out_ref, dx_ref, dm_ref, _ = ddlerp_ref(x, maa, m, s0, rev_n, dout)
    terms = dm_ref.permute(1, 2, 0, 3).reshape(rows, maa.shape[0], C)
    out = lerp_fwd_abi(lib, x, maa, m, s0, rev_n)
    no_nan(what + " out", out)
    assert same(out, lerp_fwd_abi(lib, x, maa, m, s0, rev_n)), what + ": forward not repeatable"
    close(out, out_ref, what + " out")
    res = {}
    for nparts in nparts_list:
        tag = f"{what} nparts={nparts}"
        dx, dm, part = lerp_bwd_abi(lib, x, maa, m, s0, rev_n, dout, nparts)
        no_nan(tag, dx, dm, part)
        dx2, dm2, part2 = lerp_bwd_abi(lib, x, maa, m, s0, rev_n, dout, nparts)
        assert same(dx, dx2) and same(part, part2) and (m is None or same(dm, dm2)), tag + ": backward not repeatable"
        close(dx, dx_ref, tag + " dx", ulps=1.5)
        if m is not None:
            close(dm, dm_ref, tag + " dm")
        bound = check_partials(part, terms, tag + " dmaa", empty_parts(rows, nparts, rev_n is None))
        res[nparts] = (dx, dm, part)
    check_detectable(terms, bound, what)
    return res


LERP_SHAPES = {   # (B, T, C, nparts): runs ending inside a sequence with a short last run; runs spanning whole sequences and
    #               ending at and inside sequence boundaries; every token both first and last of its sequence
    "B1T4099": (1, 4099, 256, [1, 7, 1024, 4099, 4104]),
    "B5T7": (5, 7, 128, [1, 3, 4, 35]),
    "B4101T1": (4101, 1, 128, [1, 7, 1024, 4101, 4104]),
}


@pytest.mark.parametrize("with_s0", [False, True], ids=["zero-front", "shifted0"])
@pytest.mark.parametrize("ns,has_m", INST, ids=[f"NS{n}{'m' if h else ''}" for n, h in INST])
@pytest.mark.parametrize("shape", sorted(LERP_SHAPES))
def test_ddlerp_backward_run_split(lib, shape, ns, has_m, with_s0):
    """Plain stream: workgroup p walks rows [p per, (p + 1) per) backwards, handing each row's share of the next row's blends on in
    registers and resetting it at the last token of a sequence.  Every row's dx and dm are formed by the same operations in the
    same order whichever workgroup computes them (the hand-over fetched at the end of a run is summed as `own` is), so they are
    bit-identical across nparts."""
    B, T, C, nparts_list = LERP_SHAPES[shape]
    x, maa, m, s0, dout = lerp_inputs(B, T, C, ns, has_m, with_s0, seed=10 * ns + has_m)
    res = run_lerp_case(lib, x, maa, m, s0, None, dout, nparts_list, f"ddlerp {shape} NS={ns} m={has_m} s0={with_s0}")
    dx0, dm0, _ = res[nparts_list[0]]
    for nparts, (dx, dm, _) in res.items():
        assert same(dx, dx0), f"dx differs between nparts={nparts_list[0]} and {nparts}"
        assert m is None or same(dm, dm0), f"dm differs between nparts={nparts_list[0]} and {nparts}"


def test_ddlerp_at_the_training_split(lib):
    """B=32, T=512, C=2048, NS=5 with m through mix_op: nparts = 1024, so each workgroup walks 16 rows.  The ABI at
    nparts = rows (one row each) gives the same dx and dm bit for bit."""
    from rwkv_lm_ext_amd import mix_op
    B, T, C, NS = 32, 512, 2048, 5
    x, maa, m, s0, dout = lerp_inputs(B, T, C, NS, True, True, seed=70)
    leaves = [t.clone().requires_grad_(True) for t in (x, maa, m, s0)]
    out = mix_op.ddlerp(leaves[0], leaves[1], leaves[2], leaves[3])
    out.backward(dout)
    out_ref, dx_ref, dm_ref, ds0_ref = ddlerp_ref(x, maa, m, s0, None, dout)
    close(out.detach(), out_ref, "ddlerp out")
    del out, out_ref
    close(leaves[0].grad, dx_ref, "ddlerp dx", ulps=1.5)
    close(leaves[2].grad, dm_ref, "ddlerp dm")
    close(leaves[1].grad, dm_ref.sum((1, 2)), "ddlerp dmaa")
    close(leaves[3].grad, ds0_ref, "ddlerp dshifted0", ulps=1.5)
    terms = dm_ref.permute(1, 2, 0, 3).reshape(B * T, NS, C)
    check_detectable(terms, K_PART * U * terms.abs().sum(0), "ddlerp B32T512")
    del dm_ref, dx_ref, terms
    dx, dm, part = lerp_bwd_abi(lib, x, maa, m, s0, None, dout, B * T)
    no_nan("ddlerp nparts=rows", dx, dm, part)
    assert same(dx, leaves[0].grad) and same(dm, leaves[2].grad)


# ---- ddlerp over reversed-span streams ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,has_m", INST, ids=[f"NS{n}{'m' if h else ''}" for n, h in INST])
def test_ddlerp_reversed_path_with_nothing_reversed_equals_the_plain_path(lib, ns, has_m):
    """rev_n all 0 takes the grid-stride reversed-stream kernel (rows > nparts: every workgroup handles several rows); out, dx
    and dm equal those of rev_n = NULL bit for bit (the neighbour's hand-over is summed in the plain path's order)."""
    B, T, C, nparts = 8, 640, 256, 100
    x, maa, m, s0, dout = lerp_inputs(B, T, C, ns, has_m, True, seed=80 + ns)
    zeros = torch.zeros(B, dtype=torch.int32, device="cuda")
    res = run_lerp_case(lib, x, maa, m, s0, zeros, dout, [nparts], "ddlerp rev_n=0")[nparts]
    assert same(lerp_fwd_abi(lib, x, maa, m, s0, zeros), lerp_fwd_abi(lib, x, maa, m, s0, None))
    plain = lerp_bwd_abi(lib, x, maa, m, s0, None, dout, nparts)
    assert same(res[0], plain[0]) and (m is None or same(res[1], plain[1]))


def test_ddlerp_clamps_rev_n(lib):
    """rev_n < 0 acts as 0 and rev_n > T as T, bit for bit (partial rows included: same kernel, same row assignment)."""
    B, T, C, NS, nparts = 4, 300, 128, 5, 37
    x, maa, m, s0, dout = lerp_inputs(B, T, C, NS, True, True, seed=90)
    wild = torch.tensor([-3, T + 5, 5, -(1 << 30)], dtype=torch.int32, device="cuda")
    tame = torch.tensor([0, T, 5, 0], dtype=torch.int32, device="cuda")
    a = lerp_bwd_abi(lib, x, maa, m, s0, wild, dout, nparts)
    b = lerp_bwd_abi(lib, x, maa, m, s0, tame, dout, nparts)
    no_nan("ddlerp clamp", *a)
    assert all(same(u, v) for u, v in zip(a, b))
    assert same(lerp_fwd_abi(lib, x, maa, m, s0, wild), lerp_fwd_abi(lib, x, maa, m, s0, tame))
    _, dx_ref, _, _ = ddlerp_ref(x, maa, m, s0, tame, dout)
    close(a[0], dx_ref, "ddlerp clamp dx", ulps=1.5)


def test_ddlerp_reversed_streams_at_many_rows(lib):
    """4096 rows of streams with reversed spans of every kind (none, one token, all, random), several rows per workgroup: the
    ABI at two nparts, then mix_op with the gradient of the token in front of each stream and the bf16 dmaa."""
    from rwkv_lm_ext_amd import mix_op
    B, T, C, NS = 16, 256, 256, 5
    x, maa, m, s0, dout = lerp_inputs(B, T, C, NS, True, True, seed=100)
    g = torch.Generator().manual_seed(101)
    rev_n = torch.tensor([0, 1, 2, T - 1, T, T // 2, 7] + torch.randint(0, T + 1, (B - 7,), generator=g).tolist(),
                         dtype=torch.int32, device="cuda")
    res = run_lerp_case(lib, x, maa, m, s0, rev_n, dout, [7, 1024], "ddlerp reversed streams")
    assert same(res[7][0], res[1024][0]) and same(res[7][1], res[1024][1])
    leaves = [t.clone().requires_grad_(True) for t in (x, maa, m, s0)]
    mix_op.ddlerp(*leaves, rev_n).backward(dout)
    _, dx_ref, dm_ref, ds0_ref = ddlerp_ref(x, maa, m, s0, rev_n, dout)
    assert same(leaves[0].grad, res[1024][0]) and same(leaves[2].grad, res[1024][1])
    close(leaves[0].grad, dx_ref, "mix_op dx", ulps=1.5)
    close(leaves[1].grad, dm_ref.sum((1, 2)), "mix_op dmaa")
    close(leaves[3].grad, ds0_ref, "mix_op dshifted0", ulps=1.5)


@pytest.mark.parametrize("ns,has_m", INST, ids=[f"NS{n}{'m' if h else ''}" for n, h in INST])
@pytest.mark.parametrize("C,B,T", [(64, 2, 300), (4096, 2, 160)], ids=["C64", "C4096"])
def test_ddlerp_narrowest_and_widest_rows(lib, C, B, T, ns, has_m):
    """C = 64 (16 threads: less than one wave) and C = 4096 (1024 threads) per workgroup, forward and backward, plain and
    reversed streams."""
    x, maa, m, s0, dout = lerp_inputs(B, T, C, ns, has_m, True, seed=110 + ns)
    run_lerp_case(lib, x, maa, m, s0, None, dout, [1, 37], f"ddlerp C={C}")
    rev_n = torch.tensor([T // 3, T], dtype=torch.int32, device="cuda")
    run_lerp_case(lib, x, maa, m, s0, rev_n, dout, [37], f"ddlerp C={C} reversed")


# ---- gn_gate ------------------------------------------------------------------------------------------------------------------
def gn_ref(y, g, gamma, beta, H, eps, dout):
    """fp64 GroupNorm(H) * g and its gradients written out (F.group_norm autograd is not trusted, see test_mix_gpu.py)."""
    rows, C = y.shape
    yd = y.double().view(rows, H, 64)
    mean = yd.mean(2, keepdim=True)
    var = (yd - mean).square().mean(2, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = ((yd - mean) * rstd).view(rows, C)
    ga, be = gamma.double(), beta.double()
    no = xh * ga + be
    out = no * g.double()
    d = dout.double()
    dno = d * g.double()
    dxh = (dno * ga).view(rows, H, 64)
    xh3 = xh.view(rows, H, 64)
    dy = (rstd * (dxh - dxh.mean(2, keepdim=True) - xh3 * (dxh * xh3).mean(2, keepdim=True))).view(rows, C)
    stats = torch.cat([mean, rstd], 2)                           # [rows, H, 2]
    return out, stats, dy, d * no, dno * xh, dno


def gn_fwd_abi(lib, y, g, gamma, beta, H, eps):
    rows, C = y.shape
    out, stats = poisoned(rows, C), poisoned(rows, H, 2, dtype=f32)
    assert lib.wkv6_gn_gate_forward(rows, C, H, ptr(y), ptr(g), ptr(gamma), ptr(beta), eps, ptr(out), ptr(stats), stream()) == 0
    torch.cuda.synchronize()
    return out, stats


def gn_bwd_abi(lib, y, g, gamma, beta, stats, dout, H, nparts):
    rows, C = y.shape
    dy, dg = poisoned(rows, C), poisoned(rows, C)
    pg, pb = poisoned(nparts, C, dtype=f32), poisoned(nparts, C, dtype=f32)
    assert lib.wkv6_gn_gate_backward(rows, C, H, ptr(y), ptr(g), ptr(gamma), ptr(beta), ptr(stats), ptr(dout), ptr(dy), ptr(dg),
                                     ptr(pg), ptr(pb), nparts, stream()) == 0
    torch.cuda.synchronize()
    return dy, dg, pg, pb


def check_stats(stats, ref, y, H, what):
    """mean within 8 U mean|y| of the head (7 fp32 additions in the lane sum and the 16-lane tree, then an exact 1/64); rstd within
    16 U relative (the variance sum, + eps, rsqrt)."""
    rows = y.shape[0]
    scale = y.double().abs().view(rows, H, 64).mean(2)
    s = stats.double()
    assert bool(((s[..., 0] - ref[..., 0]).abs() <= 8 * U * scale).all()), what + ": mean"
    assert bool(((s[..., 1] - ref[..., 1]).abs() <= 16 * U * ref[..., 1]).all()), what + ": rstd"


def run_gn_case(lib, y, g, gamma, beta, dout, H, nparts_list, what, heads=None):
    """forward and backward through the ABI at every nparts; `heads`: report out / dy / dg per head (degenerate heads differ in
    scale by orders of magnitude)."""
    rows, C = y.shape
    out_ref, stats_ref, dy_ref, dg_ref, tg, tb = gn_ref(y, g, gamma, beta, H, float(torch.tensor(EPS, dtype=f32)), dout)
    out, stats = gn_fwd_abi(lib, y, g, gamma, beta, H, EPS)
    no_nan(what + " forward", out, stats)
    out2, stats2 = gn_fwd_abi(lib, y, g, gamma, beta, H, EPS)
    assert same(out, out2) and same(stats, stats2), what + ": forward not repeatable"
    check_stats(stats, stats_ref, y, H, what)
    sl = [slice(None)] if heads is None else [slice(64 * h, 64 * h + 64) for h in heads]
    for s in sl:
        close(out[:, s], out_ref[:, s], f"{what} out[{s}]")
    first = None
    for nparts in nparts_list:
        tag = f"{what} nparts={nparts}"
        dy, dg, pg, pb = gn_bwd_abi(lib, y, g, gamma, beta, stats, dout, H, nparts)
        no_nan(tag, dy, dg, pg, pb)
        again = gn_bwd_abi(lib, y, g, gamma, beta, stats, dout, H, nparts)
        assert all(same(a, b) for a, b in zip((dy, dg, pg, pb), again)), tag + ": backward not repeatable"
        if first is None:
            first = (dy, dg)
            for s in sl:
                close(dy[:, s], dy_ref[:, s], f"{what} dy[{s}]", ulps=1.5)
                close(dg[:, s], dg_ref[:, s], f"{what} dg[{s}]")
        else:
            assert same(dy, first[0]) and same(dg, first[1]), tag + ": dy / dg differ between nparts"
        empty = list(range(rows, nparts))
        bg = check_partials(pg, tg, tag + " dgamma", empty)
        bb = check_partials(pb, tb, tag + " dbeta", empty)
    check_detectable(torch.stack([tg, tb], 1), torch.stack([bg, bb], 0), what)
    return stats


def gn_inputs(rows, C, seed):
    y = rnd(rows, C, scale=2.0, seed=seed)
    g = rnd(rows, C, seed=seed + 1)
    gamma = (1 + 0.2 * rnd(C, seed=seed + 2).float()).to(bf)
    beta = rnd(C, scale=0.1, seed=seed + 3)
    dout = rnd(rows, C, seed=seed + 4)
    return y, g, gamma, beta, dout


GN_SHAPES = [(rows, C) for rows in (1, 1023, 1025, 16384) for C in (64, 2048, 4096) if rows * C <= 16384 * 2048]


@pytest.mark.parametrize("rows,C", GN_SHAPES, ids=[f"rows{r}C{c}" for r, c in GN_SHAPES])
def test_gn_gate_grid_stride_backward(lib, rows, C):
    """The backward's grid-stride loop over rows at nparts 1, 3, 1024 and rows + 3 (three workgroups without rows); then mix_op's
    bf16 dgamma / dbeta."""
    from rwkv_lm_ext_amd import mix_op
    H = C // 64
    y, g, gamma, beta, dout = gn_inputs(rows, C, seed=rows + C)
    stats = run_gn_case(lib, y, g, gamma, beta, dout, H, [1, 3, 1024, rows + 3], f"gn_gate rows={rows} C={C}")
    _, _, _, _, tg, tb = gn_ref(y, g, gamma, beta, H, float(torch.tensor(EPS, dtype=f32)), dout)
    _, _, dgamma, dbeta = mix_op.gn_gate_backward(y, g, gamma, beta, stats, dout, H)
    close(dgamma, tg.sum(0), "mix_op dgamma")
    close(dbeta, tb.sum(0), "mix_op dbeta")


def test_gn_gate_degenerate_heads(lib):
    """Per row, four heads: random; all 64 values equal (variance 0, rstd = 1/sqrt(eps)); 1024 + 8 k (a large common offset with a
    small exactly representable spread: a one-pass E[y^2] - E[y]^2 would cancel); |y| ~ 1e4."""
    rows, H = 1025, 4
    C = 64 * H
    y, g, gamma, beta, dout = gn_inputs(rows, C, seed=120)
    gen = torch.Generator(device="cuda").manual_seed(121)
    y = y.view(rows, H, 64).clone()
    y[:, 1] = rnd(rows, 1, seed=122)                            # one value per row, broadcast over the head
    y[:, 2] = (1024 + 8 * torch.randint(0, 16, (rows, 64), generator=gen, device="cuda")).to(bf)
    y[:, 3] = rnd(rows, 64, scale=1e4, seed=123)
    y = y.view(rows, C).contiguous()
    assert bool((y.view(rows, H, 64)[:, 1].float().std(1) == 0).all())
    stats = run_gn_case(lib, y, g, gamma, beta, dout, H, [3, 1024], "gn_gate degenerate heads", heads=range(H))
    assert bool((stats[:, 1, 0] == y.view(rows, H, 64)[:, 1, 0].float()).all())       # the mean of equal values is exact
    assert bool((stats[:, 2, 0] == y.view(rows, H, 64)[:, 2].double().mean(1).float()).all())


# ---- sqrelu / sigmul ----------------------------------------------------------------------------------------------------------
BF_MAX = float(torch.finfo(bf).max)
EDGES = [0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 200.0, -200.0, BF_MAX, -BF_MAX]
GRID = 8192 * 256 * 8                                          # elements one full grid of launch_flat covers per pass
FLAT_N = [8, 2056, GRID + 8, 3 * GRID + 7 * 2048 + 37 * 8]   # the last: four passes, its tail a partial 256-lane block


def plant_edges(t):
    """The edge values at the start, across the end of the first grid pass and at the end of a flat tensor."""
    e = torch.tensor(EDGES, dtype=bf, device="cuda")
    n, k = t.numel(), len(EDGES)
    for at in {0, max(min(GRID - k // 2, n - k), 0), max(n - k, 0)}:
        m = min(k, n - at)
        t[at:at + m] = e[:m]
    return t


def flat_call(lib, name, n, *args):
    outs = [poisoned(n) for _ in range({"sqrelu_forward": 1, "sqrelu_backward": 1, "sigmul_forward": 1, "sigmul_backward": 2}[name])]
    assert getattr(lib, "wkv6_" + name)(n, *(ptr(a) for a in args), *(ptr(o) for o in outs), stream()) == 0
    torch.cuda.synchronize()
    no_nan(name, *outs)
    return outs


def rne(ref):
    return ref.to(f32).to(bf)


@pytest.mark.parametrize("n", FLAT_N)
def test_sqrelu_grid_stride(lib, n):
    """relu(x)^2 and 2 relu(x) dout of bf16 values are exact in fp32 (at most 16 significant bits; beyond the fp32 range both
    sides are inf), so the kernel's only rounding is its bf16 store: the outputs are RNE_bf16 of the fp64 result, bit for bit."""
    x = plant_edges(rnd(n, scale=1.5, seed=130))
    d = rnd(n, seed=131)
    (out,) = flat_call(lib, "sqrelu_forward", n, x)
    assert same(out, flat_call(lib, "sqrelu_forward", n, x)[0])
    r = x.double().clamp_min(0)
    assert torch.equal(out, rne(r * r))
    (dx,) = flat_call(lib, "sqrelu_backward", n, x, d)
    assert same(dx, flat_call(lib, "sqrelu_backward", n, x, d)[0])
    assert torch.equal(dx, rne(2 * r * d.double()))
    if n >= 64:
        assert bool(torch.isinf(out[:len(EDGES)][torch.tensor(EDGES, device="cuda") == BF_MAX]).all())


@pytest.mark.parametrize("n", FLAT_N)
def test_sigmul_grid_stride(lib, n):
    """sigmoid(r) kv and its gradients.  The kernel's sigmoid is rcp(1 + exp(-r)): exp overflows to inf below r ~ -88.7, which
    must give 0 and finite gradients; r = +-max bf16 saturates to 1 and 0."""
    r = plant_edges(rnd(n, scale=2.0, seed=140))
    kv, d = rnd(n, seed=141), rnd(n, seed=142)
    (out,) = flat_call(lib, "sigmul_forward", n, r, kv)
    dr, dkv = flat_call(lib, "sigmul_backward", n, r, kv, d)
    assert same(out, flat_call(lib, "sigmul_forward", n, r, kv)[0])
    assert all(same(a, b) for a, b in zip((dr, dkv), flat_call(lib, "sigmul_backward", n, r, kv, d)))
    for t in (out, dr, dkv):
        assert bool(torch.isfinite(t).all())
    s = torch.sigmoid(r.double())
    close(out, s * kv.double(), "sigmul out")
    close(dr, d.double() * kv.double() * s * (1 - s), "sigmul dr", ulps=1.5)
    close(dkv, d.double() * s, "sigmul dkv")
    tiny = 2.0 ** -126
    lo, hi = r.float() <= -89, r.float() == BF_MAX
    assert bool(lo.any() and hi.any()) or n < len(EDGES)
    assert all(bool((t[lo].float().abs() < tiny).all()) for t in (out, dr, dkv))
    assert same(out[hi], kv[hi]) and same(dkv[hi], d[hi]) and bool((dr[hi] == 0).all())


def test_fusable_on_device_tensors():
    from rwkv_lm_ext_amd import mix_op
    a = torch.zeros(3, 8, device="cuda", dtype=bf)
    assert mix_op.fusable(a, a[:1])
    assert not mix_op.fusable(a, torch.zeros(3, 5, device="cuda", dtype=bf))
    assert not mix_op.fusable(a.float())


# ---- the modules at a production-like split -----------------------------------------------------------------------------------
def test_channel_mix_module_at_2048_rows():
    """CMix_x060 fused against eager on 2048 rows (two per ddlerp workgroup), tolerances of
    test_mix_gpu.test_channel_mix_module_fused_equals_eager."""
    from rwkv_lm_ext_amd import callers
    torch.manual_seed(3)
    C, F_ = 256, 896
    cm = callers.CMix_x060(C, F_).cuda().to(bf)
    with torch.no_grad():
        cm.time_maa_k.uniform_(0.1, 0.9)
        cm.time_maa_r.uniform_(0.1, 0.9)
    x = rnd(8, 256, C, seed=150)
    outs = []
    for fused in (True, False):
        cm.fused = fused
        xi = x.clone().requires_grad_(True)
        y = cm(xi)
        y.backward(rnd(8, 256, C, seed=151))
        outs.append((y.detach().float(), xi.grad.float(), cm.key.weight.grad.float().clone(), cm.time_maa_k.grad.float().clone()))
        cm.zero_grad()
    for a_, b_, what in zip(outs[0], outs[1], ("y", "dx", "dW_key", "d time_maa_k")):
        assert float((a_ - b_).abs().max()) <= 3e-2 * float(b_.abs().max()), what
    ref = callers.CMix_x060(C, F_)
    ref.load_state_dict({k: v.float().cpu() for k, v in cm.state_dict().items()})
    want = ref(x.float().cpu())
    want = want.detach()
    err = lambda a: float((a.cpu() - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt())
    e_fused, e_eager = err(outs[0][0]), err(outs[1][0])
    assert e_fused <= 1.1 * e_eager + 1e-4 and e_fused <= 1e-2, (e_fused, e_eager)


def test_time_mix_module_fused_against_unfused_at_2048_rows():
    """Tmix_x060 on the HIP path (bf16 on the GPU: ddlerp backward with two rows per workgroup, gn_gate backward's loop over two
    rows) against the unfused module in fp32 on the CPU (oracle WKV) with the same bf16-rounded weights and input, tolerances of
    test_mix_gpu.test_time_mix_module_fused_matches_reference_vectors_and_unfused."""
    from oracle import caller_weights as cw
    from oracle.contract import max_norm_err
    from oracle.wkv6_torch_naive import wkv6_naive
    from rwkv_lm_ext_amd import callers
    weights = {k: v.to(bf).float() for k, v in cw.tmix_weights(torch.Generator().manual_seed(11), layer_id=1).items()}
    x = torch.randn(8, 256, cw.N_EMBD, generator=torch.Generator().manual_seed(160)).to(bf).float()
    res = []
    for fused in (True, False):
        if fused:
            tm = callers.Tmix_x060(cw.N_EMBD, cw.DIM_ATT, fused=True)
            tm.load_state_dict(weights, strict=True)
            tm = tm.cuda().to(bf)
            xi = x.cuda().to(bf).requires_grad_(True)
        else:
            tm = callers.Tmix_x060(cw.N_EMBD, cw.DIM_ATT, fused=False, wkv=lambda B, T, C, H, r, k, v, w, u: wkv6_naive(r, k, v, w, u))
            tm.load_state_dict(weights, strict=True)
            xi = x.clone().requires_grad_(True)
        out = tm(xi)
        out.float().pow(2).sum().backward()
        res.append({n: p.grad.float().cpu() for n, p in tm.named_parameters()} | {"x": xi.grad.float().cpu(),
                                                                                    "out": out.detach().float().cpu()})
    assert max_norm_err(res[0]["out"].numpy(), res[1]["out"].numpy()) <= 3e-2
    # the parameter gradients the mix kernels sum (ddlerp: time_maa_*, with the low-rank pair feeding m; gn_gate: ln_x.*).  The
    # gradients that pass through the WKV operator's backward (x, key, time_faaaa, ...) exceed 8e-2 at this length against fp32
    # and are not judged here.
    errs = {n: max_norm_err(res[0][n].numpy(), res[1][n].numpy()) for n in res[0] if n.startswith(("time_maa", "ln_x"))}
    assert len(errs) == 10 and max(errs.values()) <= 8e-2, errs
