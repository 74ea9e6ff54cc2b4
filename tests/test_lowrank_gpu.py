"""The fused low-rank time-mix inputs on the GPU: wkv6_tmix_lerp_lowrank_bf16 and wkv6_decay_lowrank_bf16 (include/wkv6_amd.h) through
mix_op.tmix_inputs and mix_op.decay_lowrank.

Bit for bit, no tolerance: (a) a batch equals its sequences served one call at a time, through the pool and through carried tokens;
(b) the dense, shifted0 and shift_pool forms agree, slots = None included; (c) duplicate slots, slot = -1 and slot = n_slots (a zero
token); (d) rows outside every sequence follow the row rule; (e) a NaN or Inf in a row of x reaches only that row and the next row of the
same sequence; (f) a NaN in a pool row reaches only the first rows of the sequences that name it; (g) two runs give the same bits;
(h) decay_lowrank: a batch equals its pieces, a NaN row stays in its row, two runs agree.  The batch of (a): CU, sequences empty first, in
the middle and last, boundaries inside a 16-row tile, total_T in lowrank_common.ROWS.

Parity against the fp64 restatement of tests/lowrank_common.py (the four bf16 rounding points of the chain), on the five planes of out
and on w: an element passes if its bits equal the restatement's b (+-0 counted as equal), else within
    out:  ulp(b) + K_BOUND |xp - x| ulp(corr_r)          w:  ulp(b) + K_BOUND ulp(corr_r),        ulp(v) = 2^(floor(log2 |v|) - 7)
and at most 0.1 % of a call's elements may differ in their bits at all.  The same two assertions are applied to the chain the fused calls
stand for (ddlerp_slots, the torch matmuls, ddlerp_slots): they check the yardstick.

(C, D, Dd), lowrank_common.WIDTHS -- the shrink walks C / 32 steps in 4 interleaved chunks, 4 steps a pass (main loop), then singly
(remainder): 64, 128, 192: the smallest sizes, the remainder loop alone, 1 to 3 column blocks; 2048 and 4096 (D 64, Dd 128): the main
loop alone; 576 (D 64, Dd 128): the main loop once, then one remainder step for two of the four chunks, and the wide ranks at a narrow
C; 768: the main loop once, then two remainder steps a chunk; 1088: the main loop twice, a remainder for two chunks, and 17 column blocks
(the last expand workgroup has one live wave); 4096 (D 32, Dd 64): the narrow ranks at the widest C.  The tests of (c)-(f) run
EDGE_WIDTHS / NAN_WIDTHS, named selections of these.
(C, N, Dd), lowrank_common.DECAY_CASES -- decay_lowrank with dim_att N != C, bitwise (h), against the restatement, and into a buffer
with sentinel bits on either side of w [rows, N]: (768, 512): N < C behind both loops; (128, 320): N > C, 5 blocks, one live wave in the
last workgroup; (576, 1088, Dd 128): the wide rank, 17 blocks; (64, 4096): the narrowest C under the widest N.
Many tiles -- 4100 rows (257 tiles) at C = 64 under lowrank_common.many_batch(): 40 sequences whose boundaries fall inside tiles over
the whole range, empty ones, duplicate slots and slots outside the pool; (a), two runs, and the parity of out and w."""
import pytest
import torch

import lowrank_common as lc

pytestmark = pytest.mark.gpu
bf = torch.bfloat16

# Measured on the CPU with tools/lowrank_parity.py (profiles/lowrank_parity.txt) on exactly the inputs of the parity cases below
# (lc.TMIX_CASES, lc.DECAY_NC_CASES): the fp32-accumulating emulation of the chain under torch's own summation order, K reversed and K in
# 4 interleaved chunks lay at most 0.999 bounds (k = 1) from the restatement on out (C = 4096, D = 64, 15 rows) and 0.985 on w (C = 4096,
# Dd = 128, 17 rows); the largest figures of the added inputs are 0.997 on out (C = 4096, D = 32, 17 rows), 0.970 on w (C = 768, 16 rows),
# 0.962 at 4100 rows and 0 (the same bits) with N != C.  K_BOUND is twice the largest ratio, rounded up to a power of two: 2 * 0.999 -> 2.
# test_lowrank_cpu.py asserts ratio <= K_BOUND / 2 and share <= CAP for every one of these input sets.
K_BOUND = 2.0

CU, SLOTS, N_SLOTS, cu_of = lc.CU, lc.SLOTS, lc.N_SLOTS, lc.cu_of      # the batch of the parity cases (and of most bitwise ones)


def i32(v):
    return torch.tensor([int(a) for a in v], dtype=torch.int32, device="cuda")


def bits(t):
    return t.contiguous().view(torch.int16)


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


_inputs = {}


def inputs(C, D, Dd, rows, N=None):
    """(CPU inputs, the same on the GPU with the weights in nn.Linear layout): made once per shape and left unchanged.  N: dim_att of the
    decay (None: C).  MANY_T rows: the pool of the many-tiles case."""
    key = (C, D, Dd, rows, N)
    if key not in _inputs:
        p = lc.make_inputs(C, D, Dd, rows, n_front=lc.MANY_SLOTS if rows == lc.MANY_T else N_SLOTS, N=N)
        g = {k: v.cuda() for k, v in p.items()}
        g["W1t"], g["W2t"], g["D1t"], g["D2t"] = (t.cuda() for t in lc.kernel_weights(p))
        _inputs[key] = (p, g)
    return _inputs[key]


def tmix(g, x, cu=None, shifted0=None, pool=None, slots=None):
    from rwkv_lm_ext_amd import mix_op
    with torch.no_grad():
        out = mix_op.tmix_inputs(x, g["maa_x"], g["W1t"], g["W2t"], g["maa5"], None if cu is None else i32(cu), shifted0, pool,
                                 None if slots is None else i32(slots))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (5,) + tuple(x.shape) and out.dtype == bf
    return out


def decay(g, xw):
    from rwkv_lm_ext_amd import mix_op
    with torch.no_grad():
        w = mix_op.decay_lowrank(xw, g["D1t"], g["D2t"], g["time_decay"])
    torch.cuda.synchronize()
    assert tuple(w.shape) == tuple(xw.shape[:-1]) + (g["D2t"].shape[0],) and w.dtype == bf
    return w


def carried(front, slots):
    """[n_seq, C]: front[slot], zero for a slot outside the pool."""
    out = torch.zeros((len(slots), front.shape[1]), dtype=bf, device=front.device)
    for s, sl in enumerate(slots):
        if 0 <= sl < front.shape[0]:
            out[s] = front[sl]
    return out


@pytest.mark.parametrize("C,D,Dd", lc.WIDTHS)
def test_batch_equals_one_call_per_sequence_bitwise(C, D, Dd):
    for total_T in lc.ROWS:
        _, g = inputs(C, D, Dd, total_T)
        batch_equals_one_call_per_sequence(g, total_T, C, cu_of(total_T), SLOTS)


def batch_equals_one_call_per_sequence(g, total_T, C, cu, slots):
    x = g["x"].view(1, total_T, C)
    mixed = tmix(g, x, cu, pool=g["front"], slots=slots)
    assert same(mixed, tmix(g, x, cu, pool=g["front"], slots=slots))                           # two runs, the same bits
    assert same(mixed, tmix(g, x, cu, shifted0=carried(g["front"], slots)))                   # carried tokens instead of the pool
    joined, served = torch.zeros_like(mixed), 0
    for s in range(len(cu) - 1):
        a, b = cu[s], cu[s + 1]
        if b == a:
            continue
        alone = tmix(g, x[:, a:b].contiguous(), [0, b - a], pool=g["front"], slots=[slots[s]])
        joined[:, :, a:b] = alone
        served += b - a
    assert served == total_T and same(mixed, joined), total_T
    assert not bool(torch.isnan(mixed).any())


def test_many_tiles_batch_equals_one_call_per_sequence_bitwise():
    """4100 rows, 257 tiles: row * C, row * DT and (s * rows + row) * C from rows in the thousands, and boundaries inside tiles all the way."""
    (C, D, Dd), total_T = lc.MANY_WIDTH, lc.MANY_T
    cu, slots = (list(v) for v in lc.many_batch())
    lens = [b - a for a, b in zip(cu, cu[1:])]
    live = [s for s, n in enumerate(lens) if n]
    assert total_T >= 4096 and len(cu) - 1 >= 40 and cu[0] == 0 and cu[-1] == total_T and min(lens) == 0
    assert lens[0] == 0 and lens[-1] == 0 and 0 in lens[1:-1]                                  # empty first, last and in the middle
    assert sum(1 for v in cu[1:-1] if v % 16) >= 30 and len({v // 16 for v in cu}) >= 30       # boundaries inside tiles, over many tiles
    assert min(v for v in cu if v) < 512 and max(v for v in cu if v < total_T) > total_T - 512
    named = [slots[s] for s in live]
    assert len(set(named)) < len(named) and -1 in named and lc.MANY_SLOTS in named             # duplicates and both kinds of slot outside the pool
    _, g = inputs(C, D, Dd, total_T)
    batch_equals_one_call_per_sequence(g, total_T, C, cu, slots)


@pytest.mark.parametrize("C,D,Dd", lc.WIDTHS)
def test_dense_shifted0_and_pool_forms_agree_bitwise(C, D, Dd):
    B = 3
    for T in (1, 5, 11):                                                    # 3, 15 and 33 rows
        _, g = inputs(C, D, Dd, B * T)
        x, first = g["x"].view(B, T, C), g["front"][:B].contiguous()
        cu = [0, T, 2 * T, 3 * T]
        dense = tmix(g, x, shifted0=first)
        packed = tmix(g, x.view(1, B * T, C), cu, shifted0=first)
        assert same(dense.view(5, 1, B * T, C), packed)
        assert same(packed, tmix(g, x.view(1, B * T, C), cu, pool=first))                       # slots = None: slot = sequence index
        assert same(packed, tmix(g, x.view(1, B * T, C), cu, pool=g["front"], slots=[0, 1, 2]))
        assert same(packed.view(5, B * T, C), tmix(g, x.view(B * T, C), cu, pool=g["front"]))   # [total_T, C], a larger pool
        zero = tmix(g, x)                                                                       # no token in front: zero
        assert same(zero, tmix(g, x, shifted0=torch.zeros_like(first)))
        assert same(zero.view(5, 1, B * T, C), tmix(g, x.view(1, B * T, C), cu))
        assert same(zero.view(5, 1, B * T, C), tmix(g, x.view(1, B * T, C), cu, pool=g["front"], slots=[-1, N_SLOTS, -(1 << 31)]))
        assert not same(zero, dense)


@pytest.mark.parametrize("C,D,Dd", lc.EDGE_WIDTHS)
def test_slots_outside_the_pool_are_zero_tokens_and_duplicates_share_a_row(C, D, Dd):
    total_T = 33
    _, g = inputs(C, D, Dd, total_T)
    cu, x = cu_of(total_T), g["x"].view(1, total_T, C)
    got = tmix(g, x, cu, pool=g["front"], slots=SLOTS)
    wide = torch.cat([g["front"], torch.zeros(1, C, dtype=bf, device="cuda")])                  # slot 4: a row of zeros that exists
    assert same(got, tmix(g, x, cu, pool=wide, slots=[4 if s in (-1, N_SLOTS) else s for s in SLOTS]))
    assert same(got, tmix(g, x, cu, pool=g["front"], slots=[(1 << 31) - 1 if s == -1 else s for s in SLOTS]))
    lone = [i for i in range(len(SLOTS)) if cu[i + 1] > cu[i]]
    assert len({SLOTS[i] for i in lone}) < len(lone)                                            # two live sequences name one slot


@pytest.mark.parametrize("C,D,Dd", lc.EDGE_WIDTHS)
def test_rows_outside_every_sequence_follow_the_row_rule(C, D, Dd):
    total_T = 33
    _, g = inputs(C, D, Dd, total_T)
    x = g["x"].view(1, total_T, C)
    # rows 0..2 lie in front of cu[0], rows 20.. behind cu[-1]: row 0 takes zero, every other one of them the row in front of it
    got = tmix(g, x, [3, 9, 20], pool=g["front"], slots=[1, 3])
    assert same(got, tmix(g, x, [0, 3, 9, total_T], pool=g["front"], slots=[-1, 1, 3]))
    assert same(got, tmix(g, x, [3, 9, 1 << 30], pool=g["front"], slots=[1, 3]))
    garbage = tmix(g, x, [1 << 30, -5, -(1 << 31), 7], pool=g["front"], slots=[1 << 20, 2, -9])  # memory-safe whatever the arrays hold
    assert tuple(garbage.shape) == tuple(got.shape)


@pytest.mark.parametrize("C,D,Dd", lc.NAN_WIDTHS)
def test_a_nan_or_inf_row_reaches_only_itself_and_the_next_row_of_its_sequence(C, D, Dd):
    total_T = 33
    _, g = inputs(C, D, Dd, total_T)
    cu = cu_of(total_T)                                                     # rows 3 | 4, 8 | 9 and 15 | 16 are boundaries
    clean = tmix(g, g["x"].view(1, total_T, C), cu, pool=g["front"], slots=SLOTS)
    for bad in (float("nan"), float("inf")):
        for row, hit in ((5, (5, 6)), (8, (8,)), (15, (15,)), (17, (17, 18)), (32, (32,)), (0, (0,))):
            x = g["x"].clone()
            x[row, (7 * row + 3) % C] = bad
            got = tmix(g, x.view(1, total_T, C), cu, pool=g["front"], slots=SLOTS)
            others = [t for t in range(total_T) if t not in hit]
            assert same(got[:, 0, others], clean[:, 0, others]), (bad, row)
            if bad != bad:
                assert bool(torch.isnan(got[:, 0, list(hit)]).all()), row


@pytest.mark.parametrize("C,D,Dd", lc.NAN_WIDTHS)
def test_a_nan_pool_row_reaches_only_the_first_rows_of_the_sequences_that_name_it(C, D, Dd):
    total_T = 33
    _, g = inputs(C, D, Dd, total_T)
    cu, x = cu_of(total_T), g["x"].view(1, total_T, C)
    clean = tmix(g, x, cu, pool=g["front"], slots=SLOTS)
    for slot in range(N_SLOTS):
        pool = g["front"].clone()
        pool[slot, 5] = float("nan")
        got = tmix(g, x, cu, pool=pool, slots=SLOTS)
        hit = [cu[s] for s in range(len(SLOTS)) if SLOTS[s] == slot and cu[s + 1] > cu[s]]
        others = [t for t in range(total_T) if t not in hit]
        assert same(got[:, 0, others], clean[:, 0, others]), slot
        assert all(bool(torch.isnan(got[:, 0, t]).all()) for t in hit), slot
    assert [cu[s] for s in range(len(SLOTS)) if SLOTS[s] == 0 and cu[s + 1] > cu[s]] == [0, 1]    # (slot 0 is named twice; 2 and 3 by empty sequences only)


@pytest.mark.parametrize("C,D,Dd", lc.WIDTHS)
def test_decay_lowrank_bitwise(C, D, Dd):
    for rows in lc.ROWS:
        _, g = inputs(C, D, Dd, rows)
        decay_bitwise(g, rows, cu_of(rows))


def decay_bitwise(g, rows, cu):
    """(h): two runs, a leading dimension, the pieces of cu one call each, a NaN row.  Returns w."""
    xw = g["x"]
    C, N = xw.shape[1], g["D2t"].shape[0]
    w = decay(g, xw)
    assert tuple(w.shape) == (rows, N)
    assert same(w, decay(g, xw))                                            # two runs
    assert same(w.view(1, rows, N), decay(g, xw.view(1, rows, C)))
    joined = torch.zeros_like(w)
    for s in range(len(cu) - 1):
        if cu[s + 1] > cu[s]:
            joined[cu[s]:cu[s + 1]] = decay(g, xw[cu[s]:cu[s + 1]].contiguous())
    assert same(w, joined), rows
    bad = xw.clone()
    bad[rows // 2, 9] = float("nan")
    got = decay(g, bad)
    others = [t for t in range(rows) if t != rows // 2]
    assert same(got[others], w[others]) and bool(torch.isnan(got[rows // 2]).all())
    assert not bool(torch.isnan(w).any())
    return w


SENTINEL = 0x7FA5                                                           # a NaN's bits: no element of w has them


def decay_between_sentinels(g, xw):
    """The decay through the C symbol (mix_op.decay_lowrank allocates w itself) with w [rows, N] in the middle of a wider buffer that holds
    SENTINEL everywhere, rows * max(C, N) elements on either side: (w, the bits in front of it, the bits behind it)."""
    from rwkv_lm_ext_amd import _lib
    from rwkv_lm_ext_amd._args import _ptr, _stream_ptr
    lib = _lib.load()
    (rows, C), (N, Dd) = xw.shape, g["D2t"].shape
    side = rows * max(C, N)
    buf = torch.full((2 * side + rows * N,), SENTINEL, dtype=torch.int16, device="cuda")
    w = buf[side:side + rows * N].view(bf).view(rows, N)
    nbytes = lib.wkv6_lowrank_workspace_bytes(rows, Dd)
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.wkv6_decay_lowrank_bf16(rows, C, Dd, N, _ptr(xw), _ptr(g["D1t"]), _ptr(g["D2t"]), _ptr(g["time_decay"]), _ptr(w), _ptr(work), nbytes,
                                     _stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return w, buf[:side], buf[side + rows * N:]


@pytest.mark.parametrize("C,N,Dd", lc.DECAY_CASES)
def test_decay_lowrank_with_dim_att_unlike_n_embd_bitwise(C, N, Dd):
    """(h) with N != C, and the rows of w are N wide: in a buffer of sentinel bits the call writes every element of [rows, N] and nothing in
    front of or behind it (rows of width C would leave sentinels inside w or write behind it, whichever of the two is larger)."""
    assert N != C
    for rows in lc.ROWS:
        _, g = inputs(C, 32, Dd, rows, N=N)
        assert tuple(g["D2t"].shape) == (N, Dd) and tuple(g["D1t"].shape) == (Dd, C) and g["time_decay"].numel() == N
        w = decay_bitwise(g, rows, cu_of(rows))
        held, front, behind = decay_between_sentinels(g, g["x"])
        assert bool((front == SENTINEL).all()) and bool((behind == SENTINEL).all()), rows
        assert not bool((bits(held) == SENTINEL).any()) and same(held, w), rows


def test_many_tiles_decay_lowrank_bitwise():
    (C, D, Dd), rows = lc.MANY_WIDTH, lc.MANY_T
    _, g = inputs(C, D, Dd, rows)
    decay_bitwise(g, rows, list(lc.many_batch()[0]))


# ---- parity against the restatement
def chain_today(g, x, cu, slots):
    """The chain of Tmix_x060.jit_func that the fused calls stand for: ddlerp_slots, the torch matmuls, ddlerp_slots."""
    from rwkv_lm_ext_amd import mix_op
    total_T, C = x.shape[1], x.shape[2]
    with torch.no_grad():
        cu_t, sl_t = i32(cu), i32(slots)
        lead = mix_op.ddlerp_slots(x, g["maa_x"].view(1, C), None, g["front"], sl_t, cu_t)[0]
        low = torch.tanh(lead @ g["W1"]).view(total_T, 5, -1).transpose(0, 1)
        corr = torch.bmm(low, g["W2"]).view(5, 1, total_T, C)
        out = mix_op.ddlerp_slots(x, g["maa5"], corr, g["front"], sl_t, cu_t)
    torch.cuda.synchronize()
    return out


def decay_today(g, xw):
    with torch.no_grad():
        w = g["time_decay"] + torch.tanh(xw @ g["D1"]) @ g["D2"]
    torch.cuda.synchronize()
    return w


_restated = {}


def restated(C, D, Dd, total_T):
    """The restatement of a parity case, computed once: out, its bound, xw = bf16 of its plane 0 (the decay's input), w, its bound."""
    key = (C, D, Dd, total_T)
    if key not in _restated:
        assert key in lc.TMIX_CASES                                         # the yardstick was measured on exactly these
        p, _ = inputs(C, D, Dd, total_T)
        c = lc.tmix_case(C, D, Dd, total_T)
        assert all(torch.equal(p[k].view(torch.int16), c["p"][k].view(torch.int16)) for k in p)
        _restated[key] = (c["out"], lc.bound_out(c["out"], c["corr"], c["d"], K_BOUND), c["xw"], c["w"], lc.bound_w(c["w"], c["corr_w"], K_BOUND))
    return _restated[key]


def parity(path, C, D, Dd, total_T, cu, slots):
    _, g = inputs(C, D, Dd, total_T)
    out_r, out_bound, xw, w_r, w_bound = restated(C, D, Dd, total_T)
    x = g["x"].view(1, total_T, C)
    if path == "fused":
        out, w = tmix(g, x, cu, pool=g["front"], slots=slots), decay(g, xw.cuda())
    else:
        out, w = chain_today(g, x, cu, slots), decay_today(g, xw.cuda())
    what = f"{path} C={C} D={D} Dd={Dd} total_T={total_T}"
    lc.assert_parity(out.cpu().view(5, total_T, C), out_r, out_bound, what + " out")
    lc.assert_parity(w.cpu(), w_r, w_bound, what + " w")


@pytest.mark.parametrize("total_T", lc.ROWS)
@pytest.mark.parametrize("C,D,Dd", lc.WIDTHS)
@pytest.mark.parametrize("path", ["fused", "today"])
def test_parity_with_the_fp64_restatement(path, C, D, Dd, total_T):
    parity(path, C, D, Dd, total_T, cu_of(total_T), SLOTS)


@pytest.mark.parametrize("path", ["fused", "today"])
def test_many_tiles_parity_with_the_fp64_restatement(path):
    cu, slots = (list(v) for v in lc.many_batch())
    parity(path, *lc.MANY_WIDTH, lc.MANY_T, cu, slots)


_restated_decay = {}


@pytest.mark.parametrize("rows", lc.ROWS)
@pytest.mark.parametrize("C,N,Dd", lc.DECAY_CASES)
@pytest.mark.parametrize("path", ["fused", "today"])
def test_decay_parity_with_dim_att_unlike_n_embd(path, C, N, Dd, rows):
    """w [rows, N] of xw [rows, C], N != C, against the restatement (lc.decay_case: xw = the x of the inputs): the same two assertions."""
    key = (C, N, Dd, rows)
    assert key in lc.DECAY_NC_CASES and N != C
    p, g = inputs(C, 32, Dd, rows, N=N)
    if key not in _restated_decay:
        c = lc.decay_case(C, N, Dd, rows)
        assert all(torch.equal(p[k].view(torch.int16), c["p"][k].view(torch.int16)) for k in p) and c["xw"] is c["p"]["x"]
        _restated_decay[key] = (c["w"], lc.bound_w(c["w"], c["corr_w"], K_BOUND))
    w_r, w_bound = _restated_decay[key]
    w = decay(g, g["x"]) if path == "fused" else decay_today(g, g["x"])
    assert tuple(w.shape) == (rows, N)
    lc.assert_parity(w.cpu(), w_r, w_bound, f"{path} decay C={C} N={N} Dd={Dd} rows={rows} w")
