"""Reversal maps and the pair launch on packed variable-length batches: wkv6_op.forward_varlen_rev_ex / backward_varlen_rev_ex,
forward_varlen_pair_ex / backward_varlen_pair_ex, mix_op.ddlerp(rev_n=, cu_seqlens=), wkv.WKV_6_VARLEN_REV / WKV_6_VARLEN_PAIR.

A packed row under a map runs the arithmetic of the dense *_rev_ex call on that sequence alone, so every tensor of a packed call equals the
dense call (B = 1, T = len_s) BIT FOR BIT -- chunked bf16 with both decay kinds, the scan kernels in bf16 and fp32 -- and the pair launch
equals two rev calls bit for bit, checkpoint areas included.  Parity with the CPU oracle goes through the gather formulation (gather every
sequence's tensors with its map, run the oracle per sequence, un-gather what REV_Y names) under the suite's contract (oracle/contract.py),
exactly as tests/test_varlen_gpu.py holds the plain packed call.  Bit-for-bit comparisons with dense calls run under
dispatch(split=0, tsplit=0): one workgroup per (batch, head), one scan level, as every packed row runs."""
import numpy as np
import pytest
import torch

from test_varlen_gpu import GRADS, bf, bits, check_bf16, check_f32, f32, host, same
from conftest import max_norm_err
from oracle.contract import F32_TOL
from varlen_common import EDGE_LENS, cu_of, many_lens, oracle_packed

pytestmark = pytest.mark.gpu
H, C = 2, 128
R, K, V, W, Y, ALL = 1, 2, 4, 8, 16, 31
MASKS = {"kvy": K | V | Y, "all": ALL, "rw": R | W, "y": Y, "none": 0}
assert EDGE_LENS == [1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 0, 330]


def rev_vectors(lens):
    """The reversed spans the tests run.  mixed: the span ends inside a 16-token block and across a 64-token group."""
    special = {330: 65, 129: 64, 63: 17}
    return {"len": list(lens), "len-1": [max(n - 1, 0) for n in lens], "zero": [0] * len(lens),
            "mixed": [special.get(n, n // 2) for n in lens]}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "the gpu suite needs a GPU"
    from rwkv_lm_ext_amd import wkv6_op
    return wkv6_op


def dev_i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device="cuda")


def make(lens, io=bf, seed=0, H=H):
    """Packed inputs; the fp32 tensors hold the bf16 values, so that one oracle run serves both I/O types."""
    total, C = max(sum(lens), 1), 64 * H
    g = torch.Generator(device="cuda").manual_seed(seed)
    r, k, v = (torch.randn(total, C, device="cuda", generator=g).mul_(0.5).to(bf).to(io) for _ in range(3))
    w = (-1 + 0.5 * torch.randn(total, C, device="cuda", generator=g)).to(bf).to(io)
    u = (torch.randn(H, 64, device="cuda", generator=g) * 0.3).to(bf).to(io)
    gy = torch.randn(total, C, device="cuda", generator=g).to(bf).to(io)
    return dict(r=r, k=k, v=v, w=w, u=u, gy=gy, cu=torch.from_numpy(cu_of(lens)).cuda(), lens=list(lens), H=H,
                max_seqlen=max(max(lens), 1))


def run(ops, d, rev, mask, ew=False, algo=None, keep=True, total=None):
    """Forward + backward of the packed rev call.  rev: list, tensor or None."""
    w = (-torch.exp(d["w"].float())).contiguous() if ew else d["w"]
    n_seq = d["cu"].numel() - 1
    T, C = d["r"].shape
    rev_n = rev if rev is None or isinstance(rev, torch.Tensor) else dev_i32(rev)
    ws = ops.new_varlen_workspace(T, n_seq, C, d["H"], "cuda") if keep else None
    y = ops.forward_varlen_rev_ex(d["r"], d["k"], d["v"], w, d["u"], d["H"], d["cu"], d["max_seqlen"], rev_n, mask, y=d.get("y_buf"),
                                  algo=algo, ws=ws, w_is_ew=ew)
    g = ops.backward_varlen_rev_ex(d["r"], d["k"], d["v"], w, d["u"], d["gy"], d["H"], d["cu"], d["max_seqlen"], rev_n, mask, algo=algo,
                                   ws=ws, ckpt_valid=keep, w_is_ew=ew)
    torch.cuda.synchronize()
    return dict(y=y, gr=g[0], gk=g[1], gv=g[2], gw=g[3], gu=g[4], ws=ws)


def dense_rev(d, s, rows, rev_s, mask, ew, algo):
    """wkv6_forward_rev_ex / wkv6_backward_rev_ex (the C ABI: the Python wrappers pass the raw decay only) on sequence s alone."""
    from rwkv_lm_ext_amd import _lib
    from rwkv_lm_ext_amd.wkv6_op import _ptr, _stream_ptr
    lib = _lib.load()
    io = d["r"].dtype
    wfull = (-torch.exp(d["w"].float())).contiguous() if ew else d["w"]
    r, k, v, w, gy = (t[rows].unsqueeze(0).contiguous() for t in (d["r"], d["k"], d["v"], wfull, d["gy"]))
    n = r.shape[1]
    flags = (0 if ew else _lib.W_RAW) | (_lib.IO_F32 if io == f32 else 0) | (_lib.ALGO_SCAN if algo == "scan" else 0)
    rev_n = dev_i32([rev_s])
    y = torch.empty_like(r)
    assert lib.wkv6_forward_rev_ex(1, n, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(d["u"]), _ptr(y), None, 0, _ptr(rev_n), mask, flags,
                                   _stream_ptr()) == 0
    gr, gk, gv, gw = (torch.empty_like(r) for _ in range(4))
    gu = torch.empty(1, C, device="cuda", dtype=f32)
    wsd = torch.empty(lib.wkv6_backward_workspace_bytes(1, n, C, H), dtype=torch.uint8, device="cuda")
    assert lib.wkv6_backward_rev_ex(1, n, C, H, _ptr(r), _ptr(k), _ptr(v), _ptr(w), _ptr(d["u"]), _ptr(gy), _ptr(gr), _ptr(gk), _ptr(gv),
                                    _ptr(gw), _ptr(gu), _ptr(wsd), wsd.numel(), _ptr(rev_n), mask, flags | _lib.PARTIALS_F32,
                                    _stream_ptr()) == 0
    return dict(y=y[0], gr=gr[0], gk=gk[0], gv=gv[0], gw=gw[0], gu=gu[0])


def assert_equals_dense(ops, d, got, rev, mask, ew, algo, what):
    cu = cu_of(d["lens"])
    with ops.dispatch(split=0, tsplit=0):
        for s, n in enumerate(d["lens"]):
            if n == 0:
                assert not bool(got["gu"][s].any()), (what, s)
                continue
            rows = slice(int(cu[s]), int(cu[s + 1]))
            want = dense_rev(d, s, rows, rev[s], mask, ew, algo)
            torch.cuda.synchronize()
            for name in ("y",) + GRADS:
                assert same(got[name][rows], want[name]), (what, s, n, rev[s], name)
            assert same(got["gu"][s], want["gu"]), (what, s, n, rev[s], "gu")


@pytest.mark.parametrize("ew", [False, True], ids=["w_raw", "ew_f32"])
@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("vec", ["len", "len-1", "zero", "mixed"])
def test_chunked_rev_call_equals_the_dense_rev_call_on_each_sequence(ops, vec, mask, ew):
    d = make(EDGE_LENS, seed=21)
    rev = rev_vectors(EDGE_LENS)[vec]
    for keep in (True, False):
        got = run(ops, d, rev, MASKS[mask], ew=ew, keep=keep)
        assert_equals_dense(ops, d, got, rev, MASKS[mask], ew, None, f"chunk {vec} {mask} keep={keep}")


@pytest.mark.parametrize("io", [bf, f32], ids=["bf16", "f32"])
@pytest.mark.parametrize("mask", ["kvy", "all", "rw"])
@pytest.mark.parametrize("vec", ["len", "len-1", "zero", "mixed"])
def test_scan_rev_call_equals_the_dense_rev_call_on_each_sequence(ops, vec, mask, io):
    d = make(EDGE_LENS, io=io, seed=22)
    rev = rev_vectors(EDGE_LENS)[vec]
    algo = "scan" if io == bf else None
    got = run(ops, d, rev, MASKS[mask], algo=algo)
    assert_equals_dense(ops, d, got, rev, MASKS[mask], False, algo, f"scan {io} {vec} {mask}")


@pytest.mark.parametrize("path", ["chunk_bf16", "scan_bf16", "scan_f32"])
def test_out_of_range_rev_n_is_clamped_on_the_device(ops, path):
    io = f32 if path == "scan_f32" else bf
    algo = "scan" if path == "scan_bf16" else None
    d = make(EDGE_LENS, io=io, seed=23)
    wild = [-5 if s % 2 == 0 else n + 7 for s, n in enumerate(EDGE_LENS)]
    clamped = [0 if s % 2 == 0 else n for s, n in enumerate(EDGE_LENS)]
    for mask in (K | V | Y, ALL):
        a, b = run(ops, d, wild, mask, algo=algo), run(ops, d, clamped, mask, algo=algo)
        for n in ("y",) + GRADS + ("gu",):
            assert same(a[n], b[n]), (path, mask, n)


@pytest.mark.parametrize("path", ["chunk_bf16", "scan_bf16", "scan_f32"])
def test_no_map_is_the_plain_packed_call(ops, path):
    io = f32 if path == "scan_f32" else bf
    algo = "scan" if path == "scan_bf16" else None
    d = make(EDGE_LENS, io=io, seed=24)
    got = run(ops, d, None, ALL, algo=algo)
    ws = ops.new_varlen_workspace(sum(EDGE_LENS), len(EDGE_LENS), C, H, "cuda")
    y = ops.forward_varlen_ex(d["r"], d["k"], d["v"], d["w"], d["u"], H, d["cu"], d["max_seqlen"], algo=algo, ws=ws)
    g = ops.backward_varlen_ex(d["r"], d["k"], d["v"], d["w"], d["u"], d["gy"], H, d["cu"], d["max_seqlen"], algo=algo, ws=ws, ckpt_valid=True)
    torch.cuda.synchronize()
    assert same(got["y"], y)
    for n, t in zip(GRADS + ("gu",), g):
        assert same(got[n], t), n


def stream_index(n, rev_s):
    """Token at every scan position of a sequence of n tokens whose first rev_s are reversed."""
    return np.concatenate([np.arange(rev_s - 1, -1, -1), np.arange(rev_s, n)]).astype(np.int64)


_ORACLE = {}


def gather_oracle(oracle, d, rev, mask):
    """The expectation through the gather formulation, once per mask (the fp32 inputs hold the bf16 values)."""
    if mask not in _ORACLE:
        cu = cu_of(d["lens"])
        idx = np.concatenate([int(cu[s]) + stream_index(n, rev[s]) for s, n in enumerate(d["lens"])])
        f = lambda name, bit: host(d[name])[idx] if mask & bit else host(d[name])
        want = oracle_packed(oracle, f("r", R), f("k", K), f("v", V), f("w", W), host(d["u"]), f("gy", Y), d["lens"])
        out = {"gu": want["gu"]}
        for name, bit in (("y", Y), ("gr", R), ("gk", K), ("gv", V), ("gw", W)):
            t = want[name]
            if mask & bit:                                  # un-gather: stream position p holds token idx[p]
                u = np.empty_like(t)
                u[idx] = t
                t = u
            out[name] = t
        _ORACLE[mask] = out
    return _ORACLE[mask]


@pytest.mark.parametrize("path", ["chunk_bf16", "scan_f32"])
@pytest.mark.parametrize("mask", ["kvy", "all"])
def test_oracle_parity_through_the_gather_formulation(ops, oracle, mask, path):
    io = bf if path == "chunk_bf16" else f32
    d = make(EDGE_LENS, io=io, seed=25)
    rev = rev_vectors(EDGE_LENS)["mixed"]
    got = run(ops, d, rev, MASKS[mask])
    want = gather_oracle(oracle, d, rev, MASKS[mask])
    for n in ("y",) + GRADS:
        (check_bf16 if io == bf else check_f32)(host(got[n]), want[n], f"{mask} {path} {n}")
    e = max_norm_err(host(got["gu"]), want["gu"])
    print(f"{mask} {path} gu (fp32 per-sequence partials): {e:.2e}")
    assert e <= (1e-3 if io == bf else F32_TOL), e


def run_pair(ops, d, d1, rev0, mask0, rev1, mask1):
    n_seq = d["cu"].numel() - 1
    T, C_ = d["r"].shape
    ws = [ops.new_varlen_workspace(T, n_seq, C_, d["H"], "cuda") for _ in range(2)]
    for t in ws:
        t.zero_()
    sets = [dict(r=d["r"], k=d["k"], v=d["v"], w=d["w"], ckpt=ws[0], rev_n=rev0, rev_mask=mask0, y=d.get("y_buf0")),
            dict(r=d1["r"], k=d1["k"], v=d1["v"], w=d1["w"], ckpt=ws[1], rev_n=rev1, rev_mask=mask1, y=d.get("y_buf1"))]
    y0, y1 = ops.forward_varlen_pair_ex(d["H"], d["u"], sets, d["cu"], d["max_seqlen"])
    sets[0]["gy"], sets[1]["gy"] = d["gy"], d1["gy"]
    g0, g1 = ops.backward_varlen_pair_ex(d["H"], d["u"], sets, d["cu"], d["max_seqlen"])
    torch.cuda.synchronize()
    return [dict(y=y0, gr=g0[0], gk=g0[1], gv=g0[2], gw=g0[3], gu=g0[4], ws=ws[0]),
            dict(y=y1, gr=g1[0], gk=g1[1], gv=g1[2], gw=g1[3], gu=g1[4], ws=ws[1])]


def second_problem(d, comp, seed):
    """Composition B: both problems read the same tensors; C: the reversed stream has its own projections."""
    if comp == "b":
        return d
    return dict(make(d["lens"], seed=seed, H=d["H"]), u=d["u"], cu=d["cu"])


@pytest.mark.parametrize("comp", ["b", "c"])
@pytest.mark.parametrize("case", ["edges", "many257"])
def test_pair_equals_two_rev_calls(ops, comp, case):
    lens = EDGE_LENS if case == "edges" else many_lens(257)
    if case == "many257":
        assert 2 * len(lens) * H == 1028 and 0 in lens
    d = make(lens, seed=26)
    d1 = second_problem(d, comp, 27)
    mask1 = K | V | Y if comp == "b" else ALL
    rev1 = dev_i32(rev_vectors(lens)["mixed" if case == "edges" else "len"])
    got = run_pair(ops, d, d1, None, 0, rev1, mask1)
    n_seq = len(lens)
    for res, dd, rev, mask in ((got[0], d, None, 0), (got[1], d1, rev1, mask1)):
        ws = ops.new_varlen_workspace(sum(lens), n_seq, C, H, "cuda").zero_()
        y = ops.forward_varlen_rev_ex(dd["r"], dd["k"], dd["v"], dd["w"], dd["u"], H, dd["cu"], dd["max_seqlen"], rev, mask, ws=ws)
        g = ops.backward_varlen_rev_ex(dd["r"], dd["k"], dd["v"], dd["w"], dd["u"], dd["gy"], H, dd["cu"], dd["max_seqlen"], rev, mask, ws=ws,
                                       ckpt_valid=True)
        torch.cuda.synchronize()
        assert same(res["y"], y), (comp, case, "y")
        for n, t in zip(GRADS + ("gu",), g):
            assert same(res[n], t), (comp, case, n)
        ints = (4 * n_seq * 4 + 255) // 256 * 256                      # the checkpoint area behind the int arrays (varlen_common.exact_workspace_need)
        assert torch.equal(res["ws"][ints:], ws[ints:]), (comp, case, "checkpoints")
    # the prepared int arrays live in the first problem's workspace
    assert torch.equal(got[0]["ws"][:4 * n_seq * 4], ws[:4 * n_seq * 4])


def gap_batch(seed):
    """cu[0] > 0, cu[n_seq] < total_T, and max_seqlen cuts the middle sequence: rows [0,5), [105,277), [327,340) are served by nobody."""
    total = 340
    d = make([total], seed=seed)
    d.update(cu=dev_i32([5, 55, 277, 327]), lens=None, max_seqlen=50)
    gaps = torch.zeros(total, dtype=torch.bool, device="cuda")
    gaps[:5] = True
    gaps[105:277] = True
    gaps[327:] = True
    return d, gaps


def test_rows_outside_every_sequence_are_zero_and_never_read(ops):
    d, gaps = gap_batch(28)
    rev = dev_i32([50, 17, 0])
    clean = run(ops, d, rev, ALL)
    clean_pair = run_pair(ops, d, d, None, 0, rev, K | V | Y)
    p = dict(d)
    for n in ("r", "k", "v", "w", "gy"):
        p[n] = d[n].clone()
        p[n][gaps] = float("nan")
    nan_bits = lambda: torch.full_like(d["r"], float("nan"))
    # the forward writes into NaN-filled buffers; the backward's outputs are the wrappers' fresh allocations, compared with the clean run
    got = run(ops, dict(p, y_buf=nan_bits()), rev, ALL)
    pair = run_pair(ops, dict(p, y_buf0=nan_bits(), y_buf1=nan_bits()), p, None, 0, rev, K | V | Y)
    for res, ref, what in ((got, clean, "rev"), (pair[0], clean_pair[0], "pair 0"), (pair[1], clean_pair[1], "pair 1")):
        for n in ("y",) + GRADS:
            assert not bool(bits(res[n][gaps]).any()), (what, n)                # +0, not -0, not NaN
            assert same(res[n][~gaps], ref[n][~gaps]), (what, n)
        assert same(res["gu"], ref["gu"]), what
    # the served rows are those of the three sequences alone
    with ops.dispatch(split=0, tsplit=0):
        for s, start in enumerate((5, 55, 277)):
            rows = slice(start, start + 50)
            want = dense_rev(d, s, rows, [50, 17, 0][s], ALL, False, None)
            torch.cuda.synchronize()
            for n in ("y",) + GRADS:
                assert same(clean[n][rows], want[n]), (s, n)


def test_backward_outputs_prefilled_with_nan_have_zero_gaps(ops):
    """The raw ABI on caller-owned NaN-filled gradient buffers (the wrappers allocate theirs)."""
    from rwkv_lm_ext_amd import _lib
    from rwkv_lm_ext_amd.wkv6_op import _ptr, _stream_ptr
    lib = _lib.load()
    d, gaps = gap_batch(29)
    rev = dev_i32([50, 17, 0])
    clean = run(ops, d, rev, ALL)
    total = d["r"].shape[0]
    outs = [torch.full_like(d["r"], float("nan")) for _ in range(4)]
    gu = torch.empty(3, C, device="cuda", dtype=f32)
    ws = ops.new_varlen_workspace(total, 3, C, H, "cuda")
    rc = lib.wkv6_backward_varlen_rev_ex(total, 3, 50, C, H, _ptr(d["cu"]), _ptr(d["r"]), _ptr(d["k"]), _ptr(d["v"]), _ptr(d["w"]), _ptr(d["u"]),
                                         _ptr(d["gy"]), *(_ptr(t) for t in outs), _ptr(gu), _ptr(ws), ws.numel(), _ptr(rev), ALL,
                                         _lib.W_RAW | _lib.PARTIALS_F32, _stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    for n, t in zip(GRADS, outs):
        assert not bool(bits(t[gaps]).any()), n
        assert same(t[~gaps], clean[n][~gaps]), n
    # both problems of the pair, in its one preparation launch
    sets = (_lib.SeqSet * 2)()
    wss = [ops.new_varlen_workspace(total, 3, C, H, "cuda") for _ in range(2)]
    ys = [torch.full_like(d["r"], float("nan")) for _ in range(2)]
    pouts = [[torch.full_like(d["r"], float("nan")) for _ in range(4)] for _ in range(2)]
    gus = [torch.empty(3, C, device="cuda", dtype=f32) for _ in range(2)]
    for i, e in enumerate(sets):
        e.r, e.k, e.v, e.w, e.y, e.gy = [_ptr(d[n]) for n in ("r", "k", "v", "w")] + [_ptr(ys[i]), _ptr(d["gy"])]
        e.gr, e.gk, e.gv, e.gw = (_ptr(t) for t in pouts[i])
        e.gu, e.ckpt, e.ckpt_bytes = _ptr(gus[i]), _ptr(wss[i]), wss[i].numel()
        e.rev_n, e.rev_mask = (_ptr(rev), ALL) if i else (None, 0)
    assert lib.wkv6_forward_varlen_pair_ex(total, 3, 50, C, H, _ptr(d["cu"]), _ptr(d["u"]), sets, _lib.W_RAW, _stream_ptr()) == 0
    assert lib.wkv6_backward_varlen_pair_ex(total, 3, 50, C, H, _ptr(d["cu"]), _ptr(d["u"]), sets, _lib.W_RAW | _lib.PARTIALS_F32,
                                            _stream_ptr()) == 0
    torch.cuda.synchronize()
    plain = run(ops, d, None, 0)
    for i, ref in enumerate((plain, clean)):
        for n, t in zip(("y",) + GRADS, [ys[i]] + pouts[i]):
            assert not bool(bits(t[gaps]).any()), (i, n)
            assert same(t[~gaps], ref[n][~gaps]), (i, n)


@pytest.mark.parametrize("path", ["chunk_bf16", "scan_f32"])
def test_nan_in_one_sequence_stays_there(ops, path):
    io = bf if path == "chunk_bf16" else f32
    lens = EDGE_LENS
    d = make(lens, io=io, seed=30)
    rev = rev_vectors(lens)["mixed"]
    clean = run(ops, d, rev, ALL)
    cu = cu_of(lens)
    for s in (0, 5, 9, 11):
        rows = slice(int(cu[s]), int(cu[s + 1]))
        p = dict(d)
        for n in ("r", "k", "v", "w", "gy"):
            p[n] = d[n].clone()
            p[n][rows] = float("nan")
        got = run(ops, p, rev, ALL)
        keep = torch.ones(sum(lens), dtype=torch.bool, device="cuda")
        keep[rows] = False
        for n in ("y",) + GRADS:
            assert bool(torch.isfinite(got[n][keep]).all()), (s, n)
            assert same(got[n][keep], clean[n][keep]), (s, n)
        others = [i for i in range(len(lens)) if i != s]
        assert same(got["gu"][others], clean["gu"][others]), s


def test_two_calls_are_bit_identical(ops):
    d = make(EDGE_LENS, seed=31)
    rev = dev_i32(rev_vectors(EDGE_LENS)["mixed"])
    a, b = run(ops, d, rev, K | V | Y), run(ops, d, rev, K | V | Y)
    pa, pb = run_pair(ops, d, d, None, 0, rev, K | V | Y), run_pair(ops, d, d, None, 0, rev, K | V | Y)
    for n in ("y",) + GRADS + ("gu",):
        assert same(a[n], b[n]), n
        assert same(pa[0][n], pb[0][n]) and same(pa[1][n], pb[1][n]), n


def test_forward_and_backward_replay_from_a_graph(ops):
    """One stream, no parallel branches: the graph reads cu_seqlens and rev_n on the device at replay time."""
    lens = EDGE_LENS
    d = make(lens, seed=32)
    n_seq = len(lens)
    total = sum(lens)
    rev = dev_i32(rev_vectors(lens)["mixed"])
    ws = ops.new_varlen_workspace(total, n_seq, C, H, "cuda")
    ref = run(ops, d, rev, ALL)
    y = torch.empty_like(d["r"])
    outs = {}

    def step():
        ops.forward_varlen_rev_ex(d["r"], d["k"], d["v"], d["w"], d["u"], H, d["cu"], d["max_seqlen"], rev, ALL, y=y, ws=ws)
        outs["g"] = ops.backward_varlen_rev_ex(d["r"], d["k"], d["v"], d["w"], d["u"], d["gy"], H, d["cu"], d["max_seqlen"], rev, ALL, ws=ws,
                                               ckpt_valid=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.current_stream().wait_stream(side)
    captured = outs["g"]
    y.zero_()
    for t in captured[:5]:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same(y, ref["y"])
    for n, t in zip(GRADS + ("gu",), captured):
        assert same(t, ref[n]), n
    lens2 = [330, 0, 200, 129, 128, 127, 65, 64, 63, 3, 2, 1]
    assert sum(lens2) == total
    rev2 = [n // 3 for n in lens2]
    d2 = dict(d, lens=lens2, cu=torch.from_numpy(cu_of(lens2)).cuda())
    ref2 = run(ops, d2, rev2, ALL)
    d["cu"].copy_(d2["cu"])
    rev.copy_(dev_i32(rev2))
    graph.replay()
    torch.cuda.synchronize()
    assert same(y, ref2["y"])
    for n, t in zip(GRADS + ("gu",), captured):
        assert same(t, ref2[n]), n


# ---- token shift over the reversed stream of every sequence ---------------------------------------------------------------------------
def shift_ref64(x, maa, m, s0, lens, rev, dout):
    """fp64, per sequence, through the stream order: dmaa [NS,C] and d shifted0 [n_seq,C]."""
    NS, Cx = maa.shape[0], x.shape[1]
    dmaa = torch.zeros(NS, Cx, dtype=torch.float64, device="cuda")
    ds0 = torch.zeros(len(lens), Cx, dtype=torch.float64, device="cuda")
    t0 = 0
    for s, n in enumerate(lens):
        if n == 0:
            continue
        idx = torch.from_numpy(stream_index(n, rev[s])).cuda() + t0
        xs = x[idx].double()
        front = torch.zeros(1, Cx, dtype=torch.float64, device="cuda") if s0 is None else s0[s:s + 1].double()
        xx = torch.cat([front, xs[:-1]], 0) - xs
        d = dout[:, idx].double()
        c = maa.double().view(NS, 1, Cx) + (0.0 if m is None else m[:, idx].double())
        dmaa += (d * xx).sum(1)
        ds0[s] = (d * c)[:, 0].sum(0)
        t0 += n
    return dmaa, ds0


@pytest.mark.parametrize("with_s0", [False, True], ids=["zero_front", "shifted0"])
@pytest.mark.parametrize("ns,has_m", [(1, False), (5, True), (2, False)], ids=["NS1", "NS5m", "NS2"])
@pytest.mark.parametrize("vec", ["len", "len-1", "zero", "mixed"])
def test_token_shift_equals_the_dense_reversed_shift_on_each_sequence(vec, ns, has_m, with_s0):
    from rwkv_lm_ext_amd import mix_op
    from test_mix_kernels_gpu import close, rnd
    lens = EDGE_LENS
    rev = rev_vectors(lens)[vec]
    T = sum(lens)
    cu = torch.from_numpy(cu_of(lens)).cuda()
    x, maa = rnd(T, C, seed=40 + ns), rnd(ns, C, scale=0.5, seed=41 + ns)
    m = rnd(ns, T, C, scale=0.3, seed=42 + ns) if has_m else None
    s0 = rnd(len(lens), C, seed=43 + ns) if with_s0 else None
    dout = rnd(ns, T, C, seed=44 + ns)
    xl, maal = x.view(1, T, C).clone().requires_grad_(True), maa.clone().requires_grad_(True)
    ml = None if m is None else m.view(ns, 1, T, C).clone().requires_grad_(True)
    sl = None if s0 is None else s0.clone().requires_grad_(True)
    out = mix_op.ddlerp(xl, maal, ml, sl, rev_n=dev_i32(rev), cu_seqlens=cu)
    out.backward(dout.view(ns, 1, T, C))
    torch.cuda.synchronize()
    t0 = 0
    for s, n in enumerate(lens):
        if n == 0:
            continue
        sl_ = slice(t0, t0 + n)
        xd = x[sl_].view(1, n, C).clone().requires_grad_(True)
        md = None if m is None else m[:, sl_].reshape(ns, 1, n, C).clone().requires_grad_(True)
        sd = None if s0 is None else s0[s:s + 1].clone()
        od = mix_op._DDLerp.apply(xd, maa, md, sd, dev_i32([rev[s]]))
        od.backward(dout[:, sl_].reshape(ns, 1, n, C))
        torch.cuda.synchronize()
        assert same(out.view(ns, T, C)[:, sl_], od.view(ns, n, C)), (s, "out")
        assert same(xl.grad.view(T, C)[sl_], xd.grad.view(n, C)), (s, "dx")
        if m is not None:
            assert same(ml.grad.view(ns, T, C)[:, sl_], md.grad.view(ns, n, C)), (s, "dm")
        t0 += n
    dmaa_ref, ds0_ref = shift_ref64(x, maa, m, s0, lens, rev, dout)
    close(maal.grad, dmaa_ref, f"{vec} NS{ns} dmaa")
    if sl is not None:
        close(sl.grad, ds0_ref, f"{vec} NS{ns} dshifted0", ulps=1.5)
        assert not bool(sl.grad[[i for i, n in enumerate(lens) if n == 0]].any())


@pytest.mark.parametrize("nparts", [1, 5])
@pytest.mark.parametrize("rev", [0, 1, 3, 4, 5])
def test_token_shift_ns1_with_m_on_the_smallest_packed_batch(rev, nparts):
    """NS = 1 with m, the pair the test above leaves out, through the C ABI at the smallest shapes at which the neighbour rule can go
    wrong: C = 64, sequences of 0, 1 and 4 tokens between a row in front of cu[0] and one behind cu[n_seq], every sequence with
    rev_n = rev (0, 1, len - 1, len, len + 1 of the longest), one workgroup and more workgroups than half the rows.  A row in front of
    cu[0] is a plain stream of its own with a zero token in front; the row behind cu[n_seq] continues the last sequence in place.  out,
    dx and dm equal the dense reversed call on each of those streams bit for bit; the partial rows sum to the fp64 terms."""
    from rwkv_lm_ext_amd import _lib
    from test_mix_kernels_gpu import check_partials, ddlerp_ref, lerp_bwd_abi, lerp_fwd_abi, no_nan, poisoned, ptr, rnd, stream
    lib = _lib.load()
    cu, T, Cx, n_seq = dev_i32([1, 1, 2, 6]), 7, 64, 3
    x, maa, m = rnd(T, Cx, seed=60), rnd(1, Cx, scale=0.5, seed=61), rnd(1, T, Cx, scale=0.3, seed=62)
    s0, dout, rev_n = rnd(n_seq, Cx, seed=63), rnd(1, T, Cx, seed=64), dev_i32([rev] * n_seq)
    out, dx, dm, part = poisoned(1, T, Cx), poisoned(T, Cx), poisoned(1, T, Cx), poisoned(nparts, 1, Cx, dtype=torch.float32)
    assert lib.wkv6_ddlerp_varlen_rev_forward(T, n_seq, Cx, 1, ptr(cu), ptr(x), ptr(s0), ptr(m), ptr(maa), ptr(rev_n), ptr(out),
                                              stream()) == 0
    assert lib.wkv6_ddlerp_varlen_rev_backward(T, n_seq, Cx, 1, ptr(cu), ptr(x), ptr(s0), ptr(m), ptr(maa), ptr(rev_n), ptr(dout), ptr(dx),
                                               ptr(dm), ptr(part), nparts, stream()) == 0
    torch.cuda.synchronize()
    no_nan(f"rev {rev} nparts {nparts}", out, dx, dm, part)
    terms = []
    # (first row, rows, token in front, reversed span) of every stream of the batch
    for t0, n, front, nrev in [(0, 1, None, 0), (1, 1, s0[1:2], min(rev, 1)), (2, 5, s0[2:3], min(rev, 4))]:
        sl_ = slice(t0, t0 + n)
        xd, md, dd, rd = x[sl_].view(1, n, Cx), m[:, sl_].reshape(1, 1, n, Cx), dout[:, sl_].reshape(1, 1, n, Cx), dev_i32([nrev])
        assert same(out[:, sl_], lerp_fwd_abi(lib, xd, maa, md, front, rd).view(1, n, Cx)), (t0, "out")
        dxd, dmd, _ = lerp_bwd_abi(lib, xd, maa, md, front, rd, dd, 1)
        assert same(dx[sl_], dxd.view(n, Cx)), (t0, "dx")
        assert same(dm[:, sl_], dmd.view(1, n, Cx)), (t0, "dm")
        terms.append(ddlerp_ref(xd, maa, md, front, rd, dd)[2].view(n, 1, Cx))
    check_partials(part, torch.cat(terms), f"rev {rev} nparts {nparts} dmaa", range(T, nparts))


# ---- autograd nodes ------------------------------------------------------------------------------------------------------------------
def test_autograd_nodes_give_the_raw_calls_and_survive_a_second_backward(ops):
    from rwkv_lm_ext_amd.wkv import WKV_6_VARLEN_PAIR, WKV_6_VARLEN_REV, _sum_bf16
    lens = EDGE_LENS
    total = sum(lens)
    d = make(lens, seed=50)
    d1 = second_problem(d, "c", 51)
    rev = dev_i32(rev_vectors(lens)["mixed"])
    raw = run(ops, d1, rev, ALL)
    leaves = [d1[n].clone().view(1, total, C).requires_grad_(True) for n in ("r", "k", "v", "w")] + [d["u"].clone().requires_grad_(True)]
    y = WKV_6_VARLEN_REV.apply(total, C, H, *leaves, d["cu"], max(lens), rev, ALL)
    assert y.shape == (1, total, C) and same(y[0], raw["y"])
    for again in (False, True):
        for t in leaves:
            t.grad = None
        y.backward(d1["gy"].view(1, total, C), retain_graph=not again)
        torch.cuda.synchronize()
        for t, n in zip(leaves, GRADS):
            assert same(t.grad[0], raw[n]), (again, n)
        assert same(leaves[4].grad, _sum_bf16(raw["gu"], (H, 64))), again
    plain = run(ops, d, None, 0)
    l0 = [d[n].clone().requires_grad_(True) for n in ("r", "k", "v", "w")]
    l1 = [d1[n].clone().requires_grad_(True) for n in ("r", "k", "v", "w")]
    u = d["u"].clone().requires_grad_(True)
    y0, y1 = WKV_6_VARLEN_PAIR.apply(total, C, H, *l0, *l1, u, d["cu"], max(lens), rev, ALL)
    assert same(y0, plain["y"]) and same(y1, raw["y"])
    for again in (False, True):
        for t in l0 + l1 + [u]:
            t.grad = None
        torch.autograd.backward([y0, y1], [d["gy"], d1["gy"]], retain_graph=not again)
        torch.cuda.synchronize()
        for t, n in zip(l0, GRADS):
            assert same(t.grad, plain[n]), (again, 0, n)
        for t, n in zip(l1, GRADS):
            assert same(t.grad, raw[n]), (again, 1, n)
        assert same(u.grad, _sum_bf16(plain["gu"], (H, 64)) + _sum_bf16(raw["gu"], (H, 64))), again


# ---- modules -------------------------------------------------------------------------------------------------------------------------
MODULE_REV = [1, 0, 17, 64, 33, 65, 0, 3]
GRAD_NAMES = ("time_faaaa", "key.weight", "time_maa_k", "time_maa_x", "time_decay", "output.weight")


def _module_case(comp, pair_launch):
    """(out, dx, parameter gradients) of the packed composition on the in-kernel path."""
    from oracle import caller_weights as cw
    from test_rev_gpu import _tmix, rnd
    from varlen_common import CALLER_LENS
    tm = _tmix()
    tm.pair_launch = pair_launch
    total = sum(CALLER_LENS)
    x = rnd(1, total, cw.N_EMBD, seed=61).requires_grad_(True)
    dout = rnd(1, total, cw.N_EMBD, seed=62)
    cu = torch.from_numpy(cu_of(CALLER_LENS)).cuda()
    assert tm._packed_in_kernel(x)
    kw = dict(cu_seqlens=cu, max_seqlen=max(CALLER_LENS), rev_n=dev_i32(MODULE_REV))
    out = tm.forward_bi_b(x, **kw) if comp == "b" else tm.forward_bi_c(x, None, **kw)
    out.backward(dout)
    torch.cuda.synchronize()
    params = dict(tm.named_parameters())
    return tm, x, dout, [out.detach(), x.grad] + [params[n].grad for n in GRAD_NAMES]


@pytest.mark.parametrize("comp", ["b", "c"])
def test_packed_compositions_against_the_dense_module_on_each_sequence(comp):
    """Bound: _close of tests/test_rev_gpu.py with its ulp counts (2 for out / dx, 4 for the parameter gradients).  The per-sequence
    parameter gradients are summed in fp32, so that the expectation carries one rounding per sequence and none of the sum."""
    from rwkv_lm_ext_amd import callers
    from test_rev_gpu import _close
    from varlen_common import CALLER_LENS
    tm, x, dout, got = _module_case(comp, True)
    _, _, _, two_calls = _module_case(comp, False)
    for name, a, b in zip(("out", "dx") + GRAD_NAMES, got, two_calls):
        assert same(a, b), (comp, name, "pair_launch True / False")
    params = dict(tm.named_parameters())
    outs, dxs, gsum, t0 = [], [], {n: 0.0 for n in GRAD_NAMES}, 0
    for n, nr in zip(CALLER_LENS, MODULE_REV):
        if n == 0:
            continue
        xs = x.detach()[:, t0:t0 + n].clone().requires_grad_(True)
        mask = (torch.arange(n, device="cuda") < nr).to(torch.int).view(1, n)
        assert tm._in_kernel_reversal(xs)
        o = tm.forward_bi_b(xs, mask) if comp == "b" else tm.forward_bi_c(xs, callers.reverse_x_idx(mask, n), mask)
        g = torch.autograd.grad(o, [xs] + [params[k] for k in GRAD_NAMES], dout[:, t0:t0 + n])
        outs.append(o.detach())
        dxs.append(g[0])
        for k, t in zip(GRAD_NAMES, g[1:]):
            gsum[k] = gsum[k] + t.float()
        t0 += n
    torch.cuda.synchronize()
    want = [torch.cat(outs, 1), torch.cat(dxs, 1)] + [gsum[k] for k in GRAD_NAMES]
    for name, a, b in zip(("out", "dx") + GRAD_NAMES, got, want):
        _close(a, b, f"packed composition {comp}: {name}", ulps=2.0 if name in ("out", "dx") else 4.0)


def test_packed_encoder_sentence_vectors_against_the_padded_encoder():
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import callers
    from test_rev_gpu import _close
    enc = callers.RwkvEncoder(cw.VOCAB, cw.N_EMBD, cw.N_LAYER, cw.DIM_ATT, cw.DIM_FFN)
    enc.load_state_dict(cw.encoder_weights(), strict=True)
    enc = enc.cuda().to(bf)
    g = torch.Generator().manual_seed(63)
    lens = [5, 1, 70, 2, 33, 64]                                                # ordinary tokens + the emb_id marker
    rows = [torch.cat([torch.randint(2, cw.VOCAB, (n - 1,), generator=g), torch.tensor([enc.emb_id])]) for n in lens]
    T = max(lens)
    padded = torch.stack([torch.cat([r, torch.full((T - len(r),), enc.pad_id)]) for r in rows]).cuda()
    packed = torch.cat(rows).view(1, -1).cuda()
    cu = torch.from_numpy(cu_of(lens)).cuda()
    with torch.no_grad():
        assert enc.blocks[0].att._packed_in_kernel(enc.emb(packed))
        want = enc.encode_sentence(padded)
        got = enc.encode_sentence(packed, cu_seqlens=cu, max_seqlen=T)
    torch.cuda.synchronize()
    assert got.shape == want.shape
    _close(got, want, "packed encode_sentence")
