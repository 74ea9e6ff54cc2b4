"""The persistent wkv6_bi launches' row walk at every chaining and routing edge.

Both passes of wkv6_bi run as ONE persistent launch each (chunk_fwd_bi_kernel, chunk_bwd12k_bi_kernel): workgroup slot s walks rows
s, 2 S - 1 - s, 2 S + s, ... of the (batch, head) rows ordered by decreasing length (length_order_kernel, 1 < B <= 4096; natural order
otherwise) -- even rounds forward, odd rounds backward -- and every call prepares the next one (carried producer registers, LDS ring
offsets, the next row's first loads, its checkpoint) whenever the slot has a next row.  A wrong carried value corrupts one row of many, on
a schedule set by B, H and the slot count, so the slot count is pinned here (wkv6_op.dispatch(bi_slots=n)) and every case is checked
three ways, forward and backward, for both decay kinds (raw bf16 w; the reference's fp32 ew = -exp(w)), each with a kept workspace
(BI_KEEP_CKPT, then CKPT_VALID) and self-contained:
  * BIT FOR BIT against the same call on the two-launch kernels (dispatch(bi_fused=0)): every wave of the persistent launches does the
    arithmetic of those kernels, whatever the schedule;
  * against the exact scan kernels (algo="scan") at the suite's bounds: 2 bf16 ulps of the tensor scale, 4 for gw / gu;
  * tokens t >= lens[b] are exactly zero;
and on a few (batch, head) slices against the fp64 oracle, which catches what both kernel families might share.

The size routing (bi_route: (T + 128) C >= 2^29, fp32 byte offsets past 2^31, goes to the exact scan kernels before anything is
enqueued) is tested at its threshold: the first routed T through every entry point, the formerly chunked T = 2^24 - 129, and the last
chunked T -- where the fp32 side buffers' byte offsets come closest to 2^31 -- forward and backward against the scan kernels under both
dispatch modes and against the oracle on windows.

Memory: the fixtures `big` (inputs of 2^24 - 128 tokens, raw w and fp32 ew: about 16 GiB) and `last_scan` (the scan kernels' outputs at
the last chunked T: about 5 GiB) are module-scoped and live until the module ends, so the routed tests peak near 58 GiB of torch memory
(plus the library's scratch).  A test added behind them runs with that memory held: put it in front of section 5, or in another module.
"""
import numpy as np
import pytest
import torch

from conftest import bf16_report, max_norm_err

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
STG = 32                                   # tokens per stage of the wkv6_bi backward (csrc/wkv6_chunk_bwd12k.hip)
NAMES = ("y", "gr", "gk", "gv", "gw", "gu")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "the gpu suite needs a GPU"
    from rwkv_lm_ext_amd import wkv6_op
    assert wkv6_op.selftest() == 0
    return wkv6_op


def host(t):
    return t.detach().float().cpu().numpy()


def gen(seed, B, T, H, ew):
    """r, k, v, w, u, gy on the device (the suite's "stress" statistics: decays exp(-exp(-1 +- 0.5))); w is fp32 ew = -exp(w) for the
    reference's decay kind.  Also returns the raw bf16 w, which the oracle takes."""
    C = H * 64
    g = torch.Generator(device="cuda").manual_seed(seed)
    r, k, v = (torch.randn(B, T, C, device="cuda", generator=g).mul_(0.5).to(BF) for _ in range(3))
    w = torch.randn(B, T, C, device="cuda", generator=g).mul_(0.5).sub_(1.0).to(BF)
    u = torch.randn(H, 64, device="cuda", generator=g).mul_(0.3).to(BF)
    gy = torch.randn(B, T, C, device="cuda", generator=g).to(BF)
    wk = (-torch.exp(w.float())).contiguous() if ew else w
    return [r, k, v, wk, u, gy], w


def clamp_lens(lens, T):
    return np.clip(np.asarray(lens, np.int64), 0, T)


def mask_of(lens, T, rng=None):
    """int32 [B,T] mask whose first zero sits at lens[b] - 1 (none for lens[b] >= T); behind the first zero random bits when rng is
    given (only the first zero counts), zeros otherwise.  lens[b] >= 1."""
    B = len(lens)
    m = np.zeros((B, T), np.int32) if rng is None else rng.integers(0, 2, (B, T)).astype(np.int32)
    for b, L in enumerate(lens):
        assert L >= 1
        if L < T:
            m[b, :L - 1] = 1
            m[b, L - 1] = 0
        else:
            m[b] = 1
    return m


# ---- a host model of the persistent launches' row walk (chunk_fwd_bi_kernel / chunk_bwd12k_bi_kernel: row_of, lookup, chain2n):
# it states which chaining cases a test reaches, so that the assertions below fail if a shape stops covering what its docstring says.
def row_walks(lens, H, slots, T, ordered):
    B = len(lens)
    n = B * H
    L = clamp_lens(lens, T)
    # (the order kernel compares the lengths as passed, unclamped: ties by index)
    order = sorted(range(B), key=lambda b: (-int(lens[b]), b)) if ordered else list(range(B))
    walks = []
    for j in range(slots):
        walk, it = [], 0
        while it * slots < n:
            row = it * slots + (slots - 1 - j if it & 1 else j)
            if row < n:
                b = order[row // H]
                walk.append(dict(round=it, row=row, b=b, h=row % H, stages=-(-int(L[b]) // STG)))
            it += 1
        walks.append(walk)
    return walks


def walk_facts(walks, n):
    """Facts of a row walk: stage counts visited, (cur -> next) pairs of consecutive rows in one slot that the backward chains (both >= 2
    stages), whether the next row changes the batch index, the parity of a short last round, rows per slot."""
    facts = dict(stages=set(), chained=set(), b_change=False, b_same=False, short_to_long=False, rows=[len(w) for w in walks],
                 short_round=None)
    for w in walks:
        for cur, nx in zip(w, w[1:]):
            facts["stages"].add(cur["stages"])
            if cur["stages"] >= 2 and nx["stages"] >= 2:
                facts["chained"].add((cur["stages"] % 2, nx["stages"] % 2))
            facts["b_change"] |= cur["b"] != nx["b"]
            facts["b_same"] |= cur["b"] == nx["b"]
            facts["short_to_long"] |= nx["stages"] > cur["stages"]
        if w:
            facts["stages"].add(w[-1]["stages"])
    slots = len(walks)
    if n % slots:
        facts["short_round"] = "even" if (n // slots) % 2 == 0 else "odd"
    return facts


# ---- one forward + backward, and the three checks
def bi_pass(ops, d, H, ew, keep, lens=None, mask=None, algo=None):
    """[y, gr, gk, gv, gw, gu] of one wkv6_bi forward + backward; keep: the forward keeps its checkpoints in an exactly
    wkv6bi_kept_bytes() workspace (the side buffers are then scratch of each call) for the backward; otherwise both calls are
    self-contained on full workspaces."""
    r, k, v, w, u, gy = d
    B, T, C = r.shape
    ws = ops.bi_new_kept(B, T, C, H, r.device) if keep else None
    y = ops.bi_forward_ex(mask, r, k, v, w, u, H, w_is_ew=ew, algo=algo, ws=ws, lens=lens)
    g = ops.bi_backward_ex(mask, r, k, v, w, u, gy, H, w_is_ew=ew, algo=algo, ws=ws, lens=lens)
    return [y, *g]


def first_difference(a, b):
    """(b, h, token, stage) of the first element where two [B,T,C] tensors differ, for the failure message."""
    idx = torch.nonzero(a != b)[0].tolist()
    if len(idx) == 3:
        return dict(b=idx[0], h=idx[2] // 64, t=idx[1], stage=idx[1] // STG)
    return dict(b=idx[0], h=idx[1] // 64)


def assert_bitwise(got, want, what):
    for n, a, b in zip(NAMES, got, want):
        if not torch.equal(a, b):
            diff = float((a.float() - b.float()).abs().max())
            pytest.fail(f"{what} {n}: persistent launch != two launches (max |diff| {diff:.3e}) first at {first_difference(a, b)}")


def assert_vs_scan(got, ref, what):
    for n, a, s in zip(NAMES, got, ref):
        a, s = a.float(), s.float()
        scale = max(float(s.abs().max()), 1e-2 if n == "gw" else 1e-3)
        err = float((a - s).abs().max())
        assert err <= (4.0 if n in ("gw", "gu") else 2.0) * 2.0 ** -8 * scale, (what, n, err / scale)


def assert_zero_tail(got, lens, T, what):
    L = torch.as_tensor(clamp_lens(lens, T), device="cuda")
    tail = torch.arange(T, device="cuda").view(1, T) >= L.view(-1, 1)          # [B,T]
    if not bool(tail.any()):
        return
    for n, t in zip(NAMES[:5], got[:5]):
        assert float(t[tail].float().abs().max()) == 0.0, (what, n)


def check_oracle_slices(oracle, got, d, w_raw, lens, T, slices, what, masks=None):
    """(b, h) slices against the fp64 oracle (its mask: row b of `masks`, or ones with the first zero at lens[b] - 1); the bf16 contract
    of the suite."""
    y, gr, gk, gv, gw, gu = got
    r, k, v, _, u, gy = d
    L = clamp_lens(lens, T)
    for (b, h) in slices:
        assert L[b] >= 1, "the reference's mask cannot express an empty row"
        sl = (slice(b, b + 1), slice(None), slice(64 * h, 64 * h + 64))
        m = masks[b:b + 1] if masks is not None else mask_of([int(L[b])], T)
        rs, ks, vs, ws, gys = (host(x[sl]) for x in (r, k, v, w_raw, gy))
        us = host(u[h:h + 1])
        checks = [("y", y, oracle.bi_forward(m, rs, ks, vs, ws, us))]
        og = oracle.bi_backward(m, rs, ks, vs, ws, us, gys)
        checks += [(n, t, og[n]) for n, t in (("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw))]
        for n, t, ref in checks:
            rms, off, ulps = bf16_report(host(t[sl]), ref, floor=0.1 if n == "gw" else 1e-3)
            assert rms <= 1e-3 and ulps <= 2.0 and off <= (0.10 if n == "gw" else 0.05), (what, b, h, n, rms, ulps, off)
        assert max_norm_err(host(gu[b, 64 * h:64 * h + 64]), og["gu_b"][0]) <= 1e-3, (what, b, h, "gu")


def run_case(ops, oracle, d, w_raw, H, ew, lens=None, mask=None, slots=None, slices=(), zero_lens=None, oracle_masks=None):
    """The three checks, kept and self-contained, plus the oracle slices; returns the persistent launches' kept-workspace outputs."""
    B, T, _ = d[0].shape
    zero_lens = zero_lens if zero_lens is not None else (host(lens).astype(np.int64) if lens is not None else None)
    ref = bi_pass(ops, d, H, ew, keep=False, lens=lens, mask=mask, algo="scan")
    kept = None
    for keep in (True, False):
        what = f"{'kept' if keep else 'self-contained'} {'ew' if ew else 'raw w'}"
        with ops.dispatch(split=0, bi_slots=slots):
            got = bi_pass(ops, d, H, ew, keep, lens=lens, mask=mask)
        with ops.dispatch(split=0, bi_fused=0):
            plain = bi_pass(ops, d, H, ew, keep, lens=lens, mask=mask)
        assert_bitwise(got, plain, what)
        assert_vs_scan(got, ref, what)
        assert_zero_tail(got, zero_lens, T, what)
        kept = kept or got
        del plain
    assert len(slices) >= 3
    check_oracle_slices(oracle, kept, d, w_raw, zero_lens, T, slices, "oracle", masks=oracle_masks)
    return kept


# ---- 1. long chains in one slot -------------------------------------------------------------------------------------------------
# 24 row lengths (T = 352) with 0, 1, 2, 3, 4, 5 .. 8, 10 and 11 stages (32 tokens each), ties included; placed on shuffled batch indices
LENS24 = [352, 321, 330, 224, 200, 193, 256, 289, 160, 161, 192, 128, 100, 97, 96, 65, 70, 64, 33, 40, 32, 1, 0, 0]
LENS18 = [352, 321, 224, 192, 128, 100, 96, 65, 64, 40, 33, 32, 1, 0, 0, 193, 160, 97]
CHAIN_CASES = {
    # id: (lens, H, slots, rows per slot, parity of the short last round)
    "48rows_3slots": (LENS24, 2, 3, (16, 16), None),       # 16 rows per slot, every round full
    "48rows_5slots": (LENS24, 2, 5, (9, 10), "odd"),       # 9 full rounds + 3 rows: the short round is an odd (backward-walking) one
    "48rows_7slots": (LENS24, 2, 7, (6, 7), "even"),       # 6 full rounds + 6 rows: the short round is an even (forward-walking) one
    "23rows_5slots": (LENS24[:23], 1, 5, (4, 5), "even"),  # 4 full rounds + 3 rows on round 4
    "18rows_5slots": (LENS18, 1, 5, (3, 4), "odd"),        # 3 full rounds + 3 rows on round 3
}


def placed(lens, seed):
    """lens on a fixed random permutation of the batch indices (so that the order kernel's permutation is not the identity)."""
    p = np.random.default_rng(seed).permutation(len(lens))
    out = np.empty(len(lens), np.int64)
    out[p] = lens
    return out


@pytest.mark.parametrize("ew", [False, True], ids=["raw_w", "fp32_ew"])
@pytest.mark.parametrize("case", list(CHAIN_CASES))
def test_long_chains_in_one_slot(ops, oracle, case, ew):
    """Chaining: each slot (pinned: dispatch(split=0, bi_slots=3/5/7)) walks 3 .. 16 rows of mixed stage counts -- 0, 1, 2, 3, 4, 7 and 11
    stages among them, odd into even and even into odd, the next row in another batch and in the same one -- so that the carried registers,
    ring offsets, in-flight loads and prefetched checkpoint of a call meet every kind of successor.  Round parity: the short last round
    (n mod slots != 0) falls on an even (forward-walking) round in 48rows_7slots / 23rows_5slots and on an odd (backward-walking) round in
    48rows_5slots / 18rows_5slots; the slots it skips end their walk on a call that must not chain."""
    lens_l, H, slots, (lo, hi), parity = CHAIN_CASES[case]
    T = 352
    lens_np = placed(lens_l, 11 + len(lens_l))
    B = len(lens_np)
    facts = walk_facts(row_walks(lens_np, H, slots, T, ordered=True), B * H)
    assert {0, 1, 2, 3, 4, 7, 11} <= facts["stages"], facts["stages"]
    assert min(facts["rows"]) == lo and max(facts["rows"]) == hi, facts["rows"]
    assert facts["short_round"] == parity
    assert facts["b_change"]
    if H == 2:
        assert facts["b_same"]
    assert {(1, 0), (0, 1)} <= facts["chained"], facts["chained"]          # odd -> even, even -> odd, both chained
    d, w_raw = gen(100 + B * H + slots, B, T, H, ew)
    lens = torch.tensor(lens_np, dtype=torch.int32, device="cuda")
    by_len = sorted(range(B), key=lambda b: -lens_np[b])
    slices = [(by_len[0], 0), (by_len[B // 3], H - 1), (by_len[B // 2], 0), (by_len[(2 * B) // 3], H - 1),
              (by_len[-4], 0)]
    run_case(ops, oracle, d, w_raw, H, ew, lens=lens, slots=slots, slices=[s for s in slices if lens_np[s[0]] >= 1])


# ---- 2. the unordered walk (B > 4096) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ew", [False, True], ids=["raw_w", "fp32_ew"])
@pytest.mark.parametrize("slots", [None, 7], ids=["cu_slots", "7slots"])
def test_unordered_walk_above_the_order_cap(ops, oracle, slots, ew):
    """Chaining short -> long: B = 4101 > 4096 rows are walked in natural order (length_order_kernel does not run: the workspace's order
    area stays untouched), so a slot chains from a short row into a longer one -- never the case under length ordering.  Random lengths
    with 0, 1, 64, 65 and T among them, on the library's slot count (min(B H, CUs)) and on 7 slots (586 rows each)."""
    B, T, H = 4101, 200, 1
    rng = np.random.default_rng(4101)
    lens_np = rng.integers(0, T + 1, B)
    lens_np[[5, 17, 300, 1234, 4100]] = [0, 1, 64, 65, T]
    n_slots = slots or min(B * H, torch.cuda.get_device_properties(0).multi_processor_count)
    facts = walk_facts(row_walks(lens_np, H, n_slots, T, ordered=False), B * H)
    assert facts["short_to_long"] and {(1, 0), (0, 1)} <= facts["chained"]
    d, w_raw = gen(4101 + (slots or 0), B, T, H, ew)
    lens = torch.tensor(lens_np, dtype=torch.int32, device="cuda")
    # the order area of the workspace (bi_carve: int32 lens[0:B], order[0:B]) is not written above the cap
    ws = ops.bi_new_kept(B, T, H * 64, H, "cuda").fill_(0xff)
    with ops.dispatch(split=0, bi_slots=slots):
        ops.bi_forward_ex(None, *d[:5], H, w_is_ew=ew, ws=ws, lens=lens)
    assert bool((ws[4 * B:8 * B].view(torch.int32) == -1).all())
    slices = [(b, 0) for b in (1, 17, 300, 1234, 4000, 4100) if lens_np[b] >= 1]
    run_case(ops, oracle, d, w_raw, H, ew, lens=lens, slots=slots, slices=slices)


# ---- 3. the order and lens kernels, read back from the workspace ------------------------------------------------------------------
def special_masks(T):
    """Rows whose first zero sits at 0, 255, 256, 257, T - 1, nowhere, and an isolated zero followed by ones (what the row length is:
    1 + index of the first zero, T without one)."""
    rows, want = [], []
    for z in (0, 255, 256, 257, T - 1):
        m = np.ones(T, np.int32)
        m[z] = 0
        m[z + 1:] = np.arange(T - z - 1) % 3 != 0          # a zero every third token behind the first one: not an all-zero tail
        rows.append(m)
        want.append(min(z + 1, T))
    rows.append(np.ones(T, np.int32))
    want.append(T)
    m = np.ones(T, np.int32)
    m[100] = 0                                             # an isolated zero, ones behind it
    rows.append(m)
    want.append(101)
    return rows, want


def tied_masks(B, T, seed):
    """B mask rows: the special rows at random positions, the rest with lengths from a small set (many ties) and random bits behind the
    first zero; returns (mask, expected lens, positions of the special rows)."""
    rng = np.random.default_rng(seed)
    want = rng.choice([1, 2, 64, 65, 101, 256, 257, T], B)
    mask = mask_of(want, T, rng)
    rows, lens = special_masks(T)
    pos = rng.permutation(B)[:len(rows)]
    for p, m, L in zip(pos, rows, lens):
        mask[p], want[p] = m, L
    return np.ascontiguousarray(mask), want.astype(np.int64), [int(p) for p in pos]


@pytest.mark.parametrize("B", [2, 257, 1000, 4096])
def test_order_and_lens_kernels_read_back(ops, B):
    """length_order_kernel and mask_to_lens_kernel on their own: after bi_forward_ex(mask, ..., ws=ws) the workspace holds int32 lens[0:B]
    then order[0:B].  lens = 1 + index of the first zero (T without one) for T = 300 > 256 (the 256-thread reduction over token strides:
    first zeros at 0, 255, 256, 257, T - 1, none, an isolated zero with ones behind it); order = the rows by decreasing length, ties by
    index, with many ties, for B = 2, 257 (several rows per thread), 1000 and 4096 (the cap: still ordered)."""
    T, H = 300, 1
    mask_np, want, _ = tied_masks(B, T, B)
    if B == 2:
        mask_np, want = np.stack(special_masks(T)[0][4:6]), np.array([T, T])     # first zero at T - 1 and none: a tie at T
    mask = torch.tensor(mask_np, device="cuda")
    d, _ = gen(B, B, T, H, False)
    ws = ops.bi_new_kept(B, T, 64 * H, H, "cuda").fill_(0xff)
    ops.bi_forward_ex(mask, *d[:5], H, ws=ws)
    got = ws[:8 * B].view(torch.int32).cpu().numpy().astype(np.int64)
    assert np.array_equal(got[:B], want), np.nonzero(got[:B] != want)
    order = got[B:]
    assert np.array_equal(np.sort(order), np.arange(B))
    assert np.array_equal(order, np.argsort(-want, kind="stable")), np.nonzero(order != np.argsort(-want, kind="stable"))


@pytest.mark.parametrize("ew", [False, True], ids=["raw_w", "fp32_ew"])
def test_non_monotone_masks_vs_oracle(ops, oracle, ew):
    """Row lengths from masks whose first zero is not the start of an all-zero tail (bits behind it, an isolated zero followed by ones;
    first zeros at 0, 255, 256, 257, T - 1, none), B = 257 rows with ties on the library's slot count (one slot walks two rows): the
    three checks, and all seven special rows (placed by tied_masks) against the fp64 oracle, which stops at the first zero as the reference
    does."""
    B, T, H = 257, 300, 1
    mask_np, want, special = tied_masks(B, T, 257)
    mask = torch.tensor(mask_np, device="cuda")
    d, w_raw = gen(257, B, T, H, ew)
    ws = ops.bi_new_kept(B, T, 64, H, "cuda")
    ops.bi_forward_ex(mask, *d[:5], H, ws=ws, w_is_ew=ew)
    assert np.array_equal(ws[:4 * B].view(torch.int32).cpu().numpy(), want)
    slices = [(b, 0) for b in special]                         # (special_masks order: first zero 0, 255, 256, 257, T - 1, none, isolated)
    run_case(ops, oracle, d, w_raw, H, ew, mask=mask, slices=slices, zero_lens=want, oracle_masks=mask_np)


# ---- 4. row lengths outside [0, T] ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ew", [False, True], ids=["raw_w", "fp32_ew"])
def test_lengths_outside_the_row_equal_the_clamped_ones(ops, oracle, ew):
    """lens = -3 and T + 5 passed directly: kernels, scan path and order kernel each clamp or compare them on their own (the order kernel
    ranks the raw values, so the rows land on other slots than with the clamped lengths).  Persistent launches on 3 slots (chained), two
    launches and the scan kernels must all give exactly what lens 0 and T give; plus the three checks and oracle slices."""
    B, T, H = 10, 200, 2
    bad = np.array([-3, 200, 205, 64, 0, 205, 33, -3, 129, 1])
    good = clamp_lens(bad, T)
    d, w_raw = gen(205, B, T, H, ew)
    lb, lg = (torch.tensor(x, dtype=torch.int32, device="cuda") for x in (bad, good))
    got = run_case(ops, oracle, d, w_raw, H, ew, lens=lb, slots=3, slices=[(1, 0), (2, 1), (5, 0), (8, 1)], zero_lens=good)
    with ops.dispatch(split=0, bi_slots=3):
        clamped = bi_pass(ops, d, H, ew, True, lens=lg)
    assert_bitwise(got, clamped, "lens outside [0, T] vs clamped")
    assert_bitwise(bi_pass(ops, d, H, ew, False, lens=lb, algo="scan"), bi_pass(ops, d, H, ew, False, lens=lg, algo="scan"),
                   "scan: lens outside [0, T] vs clamped")


# ---- 5. the size routing at its threshold ----------------------------------------------------------------------------------------
T_ROUTED = (1 << 23) - 128          # the first T bi_route sends to the exact scan kernels: (T + 128) * 64 >= 2^29
T_LAST = T_ROUTED - 1               # the last T on the chunked path: its fp32 [T][64] byte offsets stay below 2^31
T_OLD = (1 << 24) - 129             # chunked before the threshold was halved, and wrong there (gr, gw of the backward): now routed
T_ALLOC = (1 << 24) - 128           # the inputs are allocated once at this length; every T above is a contiguous prefix of them
ROW_LEN = 1000                      # routed rows: short, so that the serial scan stays cheap


@pytest.fixture(scope="module")
def big(ops):
    """B = 1, H = 1, C = 64 inputs of T_ALLOC tokens, allocated once (x[:, :T_LAST] of a [1, T, 64] tensor is contiguous).  Raw w in
    (0.02, 2.12): every token's decay exp(-exp(w)) is at most e^-1, so that an output depends only on nearby tokens (windows below)."""
    g = torch.Generator(device="cuda").manual_seed(16777088)
    shape = (1, T_ALLOC, 64)
    d = {n: torch.empty(shape, device="cuda", dtype=BF).normal_(0.0, 0.5, generator=g) for n in ("r", "k", "v")}
    d["w"] = torch.empty(shape, device="cuda", dtype=BF).uniform_(0.02, 2.12, generator=g)
    d["u"] = torch.empty((1, 64), device="cuda", dtype=BF).normal_(0.0, 0.3, generator=g)
    d["gy"] = torch.empty(shape, device="cuda", dtype=BF).normal_(0.0, 1.0, generator=g)
    d["ew"] = (-torch.exp(d["w"].float())).contiguous()
    torch.cuda.synchronize()
    yield d
    d.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def big_inputs(big, T, ew):
    return [big[n][:, :T] if n != "u" else big[n] for n in ("r", "k", "v", "ew" if ew else "w", "u", "gy")]


def routed_mask(T):
    """int32 [1, T]: first zero at 1499 (row length 1500), ones again behind it."""
    m = torch.ones((1, T), dtype=torch.int32, device="cuda")
    m[0, 1499] = 0
    m[0, 1600:1700] = 0
    return m


def report_memory(what):
    print(f"\n[{what}] torch peak allocated {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB, "
          f"free now {torch.cuda.mem_get_info()[0] / 2**30:.1f} GiB")


@pytest.mark.parametrize("src", ["lens", "mask"])
@pytest.mark.parametrize("ew", [False, True], ids=["raw_w", "fp32_ew"])
@pytest.mark.parametrize("T", [T_ROUTED, T_OLD], ids=["first_routed", "old_last_chunked"])
def test_routed_T_ex_entry_points_equal_scan_bit_for_bit(ops, big, T, ew, src):
    """Routing side: scan.  T = 2^23 - 128, the first T whose fp32 byte offsets reach 2^31, and T = 2^24 - 129, where the chunked backward
    was wrong: bi_forward_ex / bi_backward_ex must run the exact scan kernels -- the forward drops BI_KEEP_CKPT, the backward ignores
    CKPT_VALID -- so that a kept workspace and a self-contained call both equal algo="scan" bit for bit (row length 1000 passed as lens, or
    1500 from a mask)."""
    torch.cuda.reset_peak_memory_stats()
    d = big_inputs(big, T, ew)
    kw = dict(lens=torch.tensor([ROW_LEN], dtype=torch.int32, device="cuda")) if src == "lens" else dict(mask=routed_mask(T))
    ref = bi_pass(ops, d, 1, ew, False, algo="scan", **kw)
    for keep in (True, False):
        got = bi_pass(ops, d, 1, ew, keep, **kw)
        for n, a, b in zip(NAMES, got, ref):
            assert torch.equal(a, b), (keep, n)
        del got
    L = ROW_LEN if src == "lens" else 1500
    assert float(ref[0][0, :L].float().abs().max()) > 0 and float(ref[0][0, L:].float().abs().max()) == 0.0
    report_memory(f"routed ex T={T} {'ew' if ew else 'raw'} {src}")


def test_routed_T_reference_signature_equals_scan_bit_for_bit(ops, big):
    """Routing side: scan, through the reference-signature symbols wkv6bi_cuda_forward / wkv6bi_cuda_backward (fp32 ew, mask, bf16 gu
    partials) at T = 2^23 - 128: bit for bit the scan kernels' results."""
    from rwkv_lm_ext_amd import _lib
    T = T_ROUTED
    torch.cuda.reset_peak_memory_stats()
    r, k, v, ew, u, gy = big_inputs(big, T, True)
    mask = routed_mask(T)
    C = 64
    y = torch.empty_like(r)
    ops.wkv6_bi_cuda.forward(1, T, C, 1, mask, r, k, v, ew, u, y)
    g = [torch.empty_like(r) for _ in range(4)] + [torch.empty((1, C), device="cuda", dtype=BF)]
    ops.wkv6_bi_cuda.backward(1, T, C, 1, mask, r, k, v, ew, u, gy, *g)
    ys = ops.bi_forward_ex(mask, r, k, v, ew, u, 1, w_is_ew=True, algo="scan")
    assert torch.equal(y, ys)
    del y, ys
    gs = [torch.empty_like(r) for _ in range(4)] + [torch.empty((1, C), device="cuda", dtype=BF)]
    ws = ops.bi_new_workspace(1, T, C, 1, "cuda")
    p = lambda t: t.data_ptr()
    with torch.cuda.device(0):
        rc = _lib.load().wkv6bi_backward_ex(1, T, C, 1, p(mask), None, p(r), p(k), p(v), p(ew), p(u), p(gy), *(p(t) for t in gs),
                                            p(ws), ws.numel(), _lib.W_EW_F32 | _lib.ALGO_SCAN,
                                            torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "wkv6_bi backward_ex (scan)")
    for n, a, b in zip(NAMES[1:], g, gs):
        assert torch.equal(a, b), n
    report_memory("routed reference signature")


def test_routed_T_autograd_equals_scan_bit_for_bit(ops, big):
    """Routing side: scan, through the WKV_6_BI autograd function (raw w, mask; its forward keeps a wkv6bi_kept_bytes() workspace and
    its backward passes CKPT_VALID) at T = 2^23 - 128: bit for bit the scan kernels' results."""
    from rwkv_lm_ext_amd import wkv
    T = T_ROUTED
    torch.cuda.reset_peak_memory_stats()
    d = big_inputs(big, T, False)
    mask = routed_mask(T)
    leaves = [x.detach().requires_grad_(True) for x in d[:5]]
    y = wkv.RUN_CUDA_RWKV6_BI(1, T, 64, 1, mask, *leaves)
    y.backward(d[5])
    ref = bi_pass(ops, d, 1, False, False, mask=mask, algo="scan")
    assert torch.equal(y.detach(), ref[0])
    for n, t, s in zip(NAMES[1:5], leaves[:4], ref[1:5]):
        assert torch.equal(t.grad, s), n
    assert torch.equal(leaves[4].grad, wkv._sum_bf16(ref[5], (1, 64)))
    del y, leaves
    report_memory("routed autograd")


def window_check(oracle, got, d, w_raw, t0, t1, T, what, names=NAMES[:5]):
    """Tokens [t0, t1) against the fp64 oracle run on the window padded by 256 tokens each side (all-ones mask: the row runs on past
    the window): with every decay <= e^-1 the truncation is below e^-256."""
    a, b = max(t0 - 256, 0), min(t1 + 256, T)
    sl = (slice(0, 1), slice(a, b), slice(None))
    rs, ks, vs, ws, gys = (host(x[sl]) for x in (d[0], d[1], d[2], w_raw, d[5]))
    us = host(d[4])
    m = np.ones((1, b - a), np.int32)
    inner = slice(t0 - a, t1 - a)
    refs = {"y": oracle.bi_forward(m, rs, ks, vs, ws, us)}
    if len(names) > 1:
        refs.update(oracle.bi_backward(m, rs, ks, vs, ws, us, gys))
    for n, t in zip(NAMES, got):
        if n not in names:
            continue
        rms, off, ulps = bf16_report(host(t[0, t0:t1]), refs[n][0, inner], floor=0.1 if n == "gw" else 1e-3)
        assert rms <= 1e-3 and ulps <= 2.0 and off <= (0.10 if n == "gw" else 0.05), (what, t0, n, rms, ulps, off)


def assert_vs_scan_chunked(a, s, n, what, chunk=1 << 26):
    """assert_vs_scan for one [1, T, 64] tensor, a slice at a time (no full-size fp32 temporaries)."""
    a, s = a.reshape(-1), s.reshape(-1)
    scale = max(max(float(s[i:i + chunk].float().abs().max()) for i in range(0, s.numel(), chunk)), 1e-2 if n == "gw" else 1e-3)
    err = max(float((a[i:i + chunk].float() - s[i:i + chunk].float()).abs().max()) for i in range(0, s.numel(), chunk))
    assert err <= (4.0 if n in ("gw", "gu") else 2.0) * 2.0 ** -8 * scale, (what, n, err / scale)


WINDOWS = ((1 << 30) // (4 * 64), 3 << 21)     # centres: token 2^30 / (4 * 64) (fp32 byte offset 2^30) and 3 * 2^21; plus the row's end


@pytest.fixture(scope="module")
def last_scan(ops, big):
    """The scan kernels' forward and backward at the last chunked T (full-length row, fp32 ew, kept workspace)."""
    d = big_inputs(big, T_LAST, True)
    ref = bi_pass(ops, d, 1, True, True, lens=torch.tensor([T_LAST], dtype=torch.int32, device="cuda"), algo="scan")
    yield ref
    ref.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("split", [None, 0], ids=["two_wg_per_pair", "persistent"])
def test_last_chunked_T_vs_scan_and_oracle_windows(ops, oracle, big, last_scan, split):
    """Routing side: chunked.  T = 2^23 - 129, the last T on the chunked path, one full-length row, fp32 ew: under the library's dispatch
    (two workgroups per pair, [B,T,C] side buffers) and under split=0 (the persistent launch on one slot, compact side buffers), forward and
    backward with a kept workspace against the scan kernels over the whole row at the suite's bounds, and y, gr, gk, gv on 512-token
    windows around token 2^30 / (4 * 64), around token 3 * 2^21 and at the row's end against the fp64 oracle.  (gw is a whole-row fp32
    suffix sum in both kernel families -- DESIGN.md -- so a window of the oracle does not see what it sums, and its fp32 rounding drifts
    with the row's length: its check here is against the scan kernels over the whole row, at a bound of its own.)"""
    T = T_LAST
    torch.cuda.reset_peak_memory_stats()
    d = big_inputs(big, T, True)
    lens = torch.tensor([T], dtype=torch.int32, device="cuda")
    with ops.dispatch(split=split):
        got = bi_pass(ops, d, 1, True, True, lens=lens)
    for n, a, s_ in zip(NAMES, got, last_scan):
        if n != "gw":
            assert_vs_scan_chunked(a, s_, n, f"split={split}")
    # gw: the two kernel families sum 8.4 M fp32 terms per channel in different orders (whole-row suffix sums): 0.027 of the
    # tensor scale apart at this T (against 4 bf16 ulps = 0.016 at T = 4096).  Bounded separately at 1/16 of the scale.
    gw, gws = got[4].reshape(-1), last_scan[4].reshape(-1)
    scale = float(gws.float().abs().max())
    err = max(float((gw[i:i + (1 << 26)].float() - gws[i:i + (1 << 26)].float()).abs().max()) for i in range(0, gw.numel(), 1 << 26))
    assert err <= scale / 16, (f"split={split}", "gw", err / scale)
    names = ("y", "gr", "gk", "gv")
    for c in WINDOWS:
        window_check(oracle, got, d, big["w"][:, :T], c - 256, c + 256, T, f"split={split}", names=names)
    window_check(oracle, got, d, big["w"][:, :T], T - 512, T, T, f"split={split}", names=names)
    del got
    report_memory(f"last chunked T split={split}")
