"""The packed variable-length WKV6 operator where a batch stops looking like tests/test_varlen_gpu.py's twelve or 48 sequences:

A. hundreds of sequences.  varlen_prepare_kernel is one workgroup of 256 threads: past 256 sequences a thread owns several (serial inner
   loops, clamped ownership for the threads that own none, a prefix over part[] with more than one slot per thread), and the kernels behind it
   read gu / s0 / s_out / gs / checkpoint slots at sequence indices no other test reaches.  Sets: varlen_common.MANY_SETS (256, 257, 513,
   600 lengths around the block and checkpoint edges, a tenth of them empty; 300 with every non-empty length tied).  Full oracle parity at
   the suite's tolerances (test_varlen_gpu: check_bf16 / check_f32 / compare), bit identity with the same data run as packed calls of at
   most 200 sequences, and the four prepared int arrays against varlen_common.prepare_model.
   (One oracle run serves both paths: the fp32 path gets the bf16 inputs widened, so that the reference is computed once per set.)

B. rows that belong to no sequence (before cu[0], from cu[n_seq] on, behind a max_seqlen cut): +0 in y, gr, gk, gv, gw, inputs there never
   read (include/wkv6_amd.h).  The outputs are filled with NaN before the call and the inputs with NaN on the gaps, so a row that nobody
   writes, or an input that somebody reads, shows."""
import numpy as np
import pytest
import torch

from conftest import max_norm_err
from oracle.contract import F32_TOL
from test_varlen_gpu import GRADS, check_bf16, compare, host, make, ops, oracle_of, run, same          # noqa: F401  (ops: fixture)
from varlen_common import EDGE_LENS, MANY_SETS, cu_of, prepare_model

pytestmark = pytest.mark.gpu
bf, f32 = torch.bfloat16, torch.float32
NAN = float("nan")
IO = {"chunk_bf16": bf, "scan_f32": f32}


def widen(d):
    """The same problem with fp32 I/O (every value is the bf16 one, exactly)."""
    return {n: (t.float() if isinstance(t, torch.Tensor) and t.dtype == bf else t) for n, t in d.items()}


# ---- A. many sequences ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many():
    """many(name, oracle=None, with_s0=False) -> inputs of a set (bf16), its per-sequence s0 and, when an oracle is given, its expectation:
    made once, shared among the tests of this module, never written, released with the module."""
    cache = {}

    def get(name, oracle=None, with_s0=False):
        if name not in cache:
            d = make(MANY_SETS[name], 2, bf, seed=20 + len(MANY_SETS[name]))
            g = torch.Generator(device="cuda").manual_seed(21)
            cache[name] = dict(d=d, s0=(torch.randn(len(d["lens"]), 2, 64, 64, device="cuda", generator=g) * 0.3).to(bf))
        e = cache[name]
        key = "want_s0" if with_s0 else "want"
        if oracle is not None and key not in e:
            e[key] = oracle_of(oracle, e["d"], s0=e["s0"] if with_s0 else None)
        return e["d"], e["s0"], e.get(key)

    yield get
    cache.clear()


@pytest.mark.parametrize("path", sorted(IO))
@pytest.mark.parametrize("name", ["257", "600"])
def test_oracle_parity_on_every_sequence(ops, oracle, many, name, path):
    d, _, want = many(name, oracle)
    io = IO[path]
    compare(run(ops, d if io == bf else widen(d)), want, io, f"{name} sequences {path}")


@pytest.mark.parametrize("path", sorted(IO))
def test_per_sequence_states_of_600_sequences(ops, oracle, many, path):
    """s0 / s_out / gs [600,2,64,64] (WKV6_S0_PER_BATCH), bounds of test_varlen_gpu.test_per_sequence_states."""
    d, s0, want = many("600", oracle, with_s0=True)
    io = IO[path]
    if io == f32:
        d, s0 = widen(d), s0.float()
    got = run(ops, d, s0=s0, want_state=True)
    compare(got, want, io, f"600 per-sequence states {path}")
    for n in ("s_out", "gs"):
        a = host(got[n])
        if io == bf and n == "s_out":
            check_bf16(a, want[n], f"600 per-sequence states {path} {n}")
        else:
            e = max_norm_err(a, want[n])
            print(f"600 per-sequence states {path} {n}: {e:.2e}")
            assert e <= (1e-3 if io == bf else F32_TOL), (n, e)
    empties = [s for s, n in enumerate(d["lens"]) if n == 0]
    assert len(empties) == 56
    for s in empties:
        assert same(got["s_out"][s], s0[s]), s
    idx = torch.tensor(empties, device="cuda")
    assert not bool(got["gu"][idx].any()) and not bool(got["gs"][idx].any())


@pytest.mark.parametrize("keep", [True, False], ids=["keep", "nokeep"])
@pytest.mark.parametrize("name", sorted(MANY_SETS))
def test_one_call_equals_calls_of_at_most_200_sequences(ops, many, name, keep):
    """Bit identity across the 256-sequence boundary: no piece has a thread of the preparation kernel own two sequences."""
    d, _, _ = many(name)
    lens, cu = d["lens"], cu_of(d["lens"])
    whole = run(ops, d, want_state=True, keep=keep)
    for a in range(0, len(lens), 200):
        b = min(a + 200, len(lens))
        t0, t1 = int(cu[a]), int(cu[b])
        if t1 == t0:    # nothing but empty sequences (no call can have total_T = 0): zero gu, s_out = the zero initial state
            assert not bool(whole["gu"][a:b].any()) and not bool(whole["s_out"][a:b].view(torch.int16).any()), (name, a)
            continue
        piece = dict(d, lens=lens[a:b], cu=torch.from_numpy((cu[a:b + 1] - cu[a]).astype(np.int32)).cuda(),
                     max_seqlen=max(max(lens[a:b]), 1), **{n: d[n][t0:t1] for n in ("r", "k", "v", "w", "gy")})
        got = run(ops, piece, want_state=True, keep=keep)
        for n in ("y",) + GRADS:
            assert same(got[n], whole[n][t0:t1]), (name, a, n)
        assert same(got["gu"], whole["gu"][a:b]) and same(got["s_out"], whole["s_out"][a:b]), (name, a)


@pytest.mark.parametrize("cut", [None, 64], ids=["whole", "cut64"])
@pytest.mark.parametrize("name", sorted(MANY_SETS))
def test_prepared_arrays_equal_the_model(ops, many, name, cut):
    """The leading four int32 [n_seq] arrays of the workspace (lens, tok_off, ck_off, order: include/wkv6_amd.h)."""
    d, _, _ = many(name)
    n_seq, (total, C) = len(d["lens"]), d["r"].shape
    max_seqlen = cut or d["max_seqlen"]
    ws = ops.new_varlen_workspace(total, n_seq, C, 2, "cuda")
    ws[:16 * n_seq].fill_(0xA5)
    y = torch.full_like(d["r"], NAN)
    ops.forward_varlen_ex(d["r"], d["k"], d["v"], d["w"], d["u"], 2, d["cu"], max_seqlen, y=y, ws=ws)
    torch.cuda.synchronize()
    got = ws[:16 * n_seq].view(torch.int32).view(4, n_seq).cpu().numpy()
    want = prepare_model(cu_of(d["lens"]), total, max_seqlen, total // 64 + n_seq)
    assert sorted(got[3].tolist()) == list(range(n_seq)), "order is no permutation"
    for a, b, what in zip(got, want, ("lens", "tok_off", "ck_off", "order")):
        assert np.array_equal(a, b), (name, what, np.flatnonzero(a != b)[:8])
    # the rows that the cut leaves outside every sequence (hundreds of gaps, more than one per thread of a fill workgroup) are +0
    inside = covered_mask(zip(want[1].tolist(), want[0].tolist()), total)
    assert int((~inside).sum()) == total - int(want[0].sum()) and bool(inside.all()) == (max(d["lens"]) <= max_seqlen)
    assert bool(torch.isfinite(y[inside]).all()) and not bool(y[~inside].view(torch.int16).any())


# ---- B. rows outside every sequence -----------------------------------------------------------------------------------------------------
BASE_LENS = [100, 300, 50]                  # the three sequences of every layout; rows 0, 100, 400 of the gap-free base problem
# layout: (cu_seqlens, total_T, max_seqlen, [(first row, rows served) per sequence])
LAYOUTS = {
    "front": ([37, 137, 437, 487], 487, 300, [(37, 100), (137, 300), (437, 50)]),
    "tail": ([0, 100, 400, 450], 514, 300, [(0, 100), (100, 300), (400, 50)]),
    "cut": ([0, 100, 400, 450], 450, 128, [(0, 100), (100, 128), (400, 50)]),
    "all": ([37, 137, 437, 487], 551, 128, [(37, 100), (137, 128), (437, 50)]),
    "empty": ([0, 0, 0, 0], 450, 300, [(0, 0), (0, 0), (0, 0)]),
}
PATHS = {"chunk_bf16": (bf, None), "scan_f32": (f32, None), "scan_bf16": (bf, "scan")}


def covered_mask(spans, total):
    m = torch.zeros(total, dtype=torch.bool, device="cuda")
    for t0, n in spans:
        m[t0:t0 + n] = True
    return m


def gapped(base, layout):
    """The base problem laid out with gaps: NaN in r, k, v, w, gy wherever no sequence is served."""
    cu, total, max_seqlen, spans = LAYOUTS[layout]
    d = dict(base, cu=torch.tensor(cu, dtype=torch.int32, device="cuda"), max_seqlen=max_seqlen, lens=[n for _, n in spans])
    src = cu_of(BASE_LENS)
    for name in ("r", "k", "v", "w", "gy"):
        t = torch.full((total, base[name].shape[1]), NAN, device="cuda", dtype=base[name].dtype)
        for s, (t0, n) in enumerate(spans):
            t[t0:t0 + n] = base[name][int(src[s]):int(src[s]) + n]
        d[name] = t
    return d


def gap_free(base, layout):
    """The same served rows packed back to back."""
    spans = LAYOUTS[layout][3]
    src = cu_of(BASE_LENS)
    rows = torch.cat([torch.arange(int(src[s]), int(src[s]) + n) for s, (_, n) in enumerate(spans)]).cuda()
    lens = [n for _, n in spans]
    return dict(base, lens=lens, cu=torch.from_numpy(cu_of(lens)).cuda(), max_seqlen=max(lens),
                **{n: base[n][rows].contiguous() for n in ("r", "k", "v", "w", "gy")})


def run_prefilled(ops, d, algo, keep):
    """Forward + backward into buffers that hold NaN everywhere: the backward through the C symbol, whose outputs the wrapper would
    allocate itself."""
    from rwkv_lm_ext_amd import _lib
    from rwkv_lm_ext_amd.wkv6_op import _ptr, _stream_ptr
    H, n_seq = d["H"], len(d["lens"])
    total, C = d["r"].shape
    io = d["r"].dtype
    nan = lambda *shape, dtype=io: torch.full(shape, NAN, device="cuda", dtype=dtype)
    out = dict(y=nan(total, C), s_out=nan(n_seq, H, 64, 64), gu=nan(n_seq, C, dtype=f32), **{n: nan(total, C) for n in GRADS})
    ws = ops.new_varlen_workspace(total, n_seq, C, H, "cuda")
    ops.forward_varlen_ex(d["r"], d["k"], d["v"], d["w"], d["u"], H, d["cu"], d["max_seqlen"], s_out=out["s_out"], y=out["y"], algo=algo,
                          ws=ws if keep else None)
    flags = _lib.W_RAW | _lib.PARTIALS_F32 | (_lib.IO_F32 if io == f32 else 0) | (_lib.ALGO_SCAN if algo == "scan" else 0)
    if keep and io == bf and algo != "scan":
        flags |= _lib.CKPT_VALID
    rc = _lib.load().wkv6_backward_varlen_ex(total, n_seq, int(d["max_seqlen"]), C, H, _ptr(d["cu"]), _ptr(d["r"]), _ptr(d["k"]),
                                             _ptr(d["v"]), _ptr(d["w"]), _ptr(d["u"]), None, _ptr(d["gy"]), _ptr(out["gr"]),
                                             _ptr(out["gk"]), _ptr(out["gv"]), _ptr(out["gw"]), _ptr(out["gu"]), None, _ptr(ws),
                                             ws.numel(), flags, _stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("keep", [True, False], ids=["keep", "nokeep"])
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_rows_outside_every_sequence_are_zero(ops, layout, path, keep):
    io, algo = PATHS[path]
    base = make(BASE_LENS, 2, io, seed=30)
    d = gapped(base, layout)
    total, spans = LAYOUTS[layout][1], LAYOUTS[layout][3]
    got = run_prefilled(ops, d, algo, keep)
    inside = covered_mask(spans, total)
    assert int((~inside).sum()) == total - sum(n for _, n in spans) > 0
    for n in ("y",) + GRADS:
        stray = got[n][~inside].view(torch.int16 if io == bf else torch.int32)      # +0: no bit set
        assert not bool(stray.any()), (layout, path, n, "rows", torch.flatnonzero(stray.any(1))[:8].tolist())
    if layout == "empty":
        assert not bool(got["gu"].any()) and not bool(got["s_out"].view(torch.int16 if io == bf else torch.int32).any())
        return
    ref = run(ops, gap_free(base, layout), algo=algo, want_state=True, keep=keep)
    for n in ("y",) + GRADS:
        assert same(got[n][inside], ref[n]), (layout, path, n)
    assert same(got["gu"], ref["gu"]) and same(got["s_out"], ref["s_out"]), (layout, path)


def test_autograd_functions_on_a_buffer_with_a_tail_gap(ops):
    """WKV_6_VARLEN / WKV_6STATE_VARLEN: the leaves' gradients are zero on the gap, gu / gs are those of the exact-fit call."""
    from rwkv_lm_ext_amd.wkv import RUN_CUDA_RWKV6_VARLEN, RUN_CUDA_RWKV6_STATE_VARLEN
    base = make(BASE_LENS, 2, bf, seed=31)
    d = gapped(base, "tail")
    total, fit, C = 514, 450, 128
    s = (torch.randn(2, 64, 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 0.3).to(bf)

    def grads(p, rows, state):
        leaves = [p[n].clone().requires_grad_(True) for n in ("r", "k", "v", "w", "u")] + ([s.clone().requires_grad_(True)] if state else [])
        fn = RUN_CUDA_RWKV6_STATE_VARLEN if state else RUN_CUDA_RWKV6_VARLEN
        y = fn(rows, C, 2, *leaves, p["cu"], 300)
        y.backward(p["gy"].view(y.shape))
        torch.cuda.synchronize()
        return y.detach().view(rows, C), [t.grad for t in leaves]

    for state in (False, True):
        y, g = grads(d, total, state)
        y0, g0 = grads(base, fit, state)
        assert same(y[:fit], y0) and not bool(y[fit:].view(torch.int16).any())
        for t, t0 in zip(g[:4], g0[:4]):
            assert same(t[:fit], t0) and not bool(t[fit:].view(torch.int16).any())
        for t, t0 in zip(g[4:], g0[4:]):                                         # gu (and gs)
            assert same(t, t0)


def test_time_mix_module_on_a_buffer_with_spare_rows():
    """Tmix_x060(cu_seqlens=) on a fixed-capacity buffer, 64 rows more than the batch fills, gy = 0 there: every parameter gradient is
    finite and within the 2 * OP_TOL that test_varlen_gpu.test_time_mix_module_on_a_packed_batch holds, against the exact-fit buffer.
    A supplement at the module level: the operator's outputs are allocated inside the module (torch.empty), so whether a lost zero fill
    shows here depends on what the allocator hands out -- the NaN written into freed blocks below makes that likely, not certain.  The
    contract itself is held deterministically by test_rows_outside_every_sequence_are_zero, on buffers that hold NaN before the call."""
    from oracle import caller_weights as cw
    from rwkv_lm_ext_amd import callers
    from test_callers_gpu import OP_TOL
    from varlen_common import CALLER_LENS
    tm = callers.Tmix_x060(cw.N_EMBD, cw.DIM_ATT)
    tm.load_state_dict(cw.tmix_weights(torch.Generator().manual_seed(11), layer_id=1), strict=True)
    tm = tm.cuda().to(bf)
    lens, fit = CALLER_LENS, sum(CALLER_LENS)
    x = torch.randn(1, fit + 64, cw.N_EMBD, generator=torch.Generator().manual_seed(5)).cuda().to(bf)
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(6)).cuda().to(bf)
    gy[:, fit:] = 0
    cu = torch.from_numpy(cu_of(lens)).cuda()
    assert tm._use_fused(x)
    want = tm(x[:, :fit].contiguous(), cu_seqlens=cu, max_seqlen=max(lens))
    tm.zero_grad()
    want.backward(gy[:, :fit].contiguous())
    gwant = {n: p.grad.clone() for n, p in tm.named_parameters()}
    # dirty the allocator's free blocks: the operator's outputs are torch.empty
    for _ in range(2):
        junk = [torch.full((fit + 64, cw.DIM_ATT), NAN, device="cuda", dtype=bf) for _ in range(8)]
        del junk
    got = tm(x, cu_seqlens=cu, max_seqlen=max(lens))
    tm.zero_grad()
    got.backward(gy)
    torch.cuda.synchronize()
    e = max_norm_err(host(got[:, :fit]), host(want))
    assert e <= OP_TOL, e
    for n, p in tm.named_parameters():
        assert bool(torch.isfinite(p.grad).all()), n
        eg = max_norm_err(host(p.grad), host(gwant[n]))
        print(f"  grad {n}: {eg:.2e}")
        assert eg <= 2 * OP_TOL, (n, eg)


def test_graph_replay_zeroes_a_tail_gap_that_new_boundaries_open(ops):
    """The idea of test_varlen_gpu.test_forward_and_backward_replay_from_a_graph, one replay further: boundaries written into the captured
    cu_seqlens leave the last 130 rows outside every sequence, the buffers hold NaN -- the replay zeroes them, not the host."""
    lens = EDGE_LENS
    d = make(lens, 2, bf, seed=12)
    H, n_seq = 2, len(lens)
    total, C = d["r"].shape
    ws = ops.new_varlen_workspace(total, n_seq, C, H, "cuda")
    y = torch.empty_like(d["r"])
    outs = {}

    def step():
        ops.forward_varlen_ex(d["r"], d["k"], d["v"], d["w"], d["u"], H, d["cu"], d["max_seqlen"], y=y, ws=ws)
        outs["g"] = ops.backward_varlen_ex(d["r"], d["k"], d["v"], d["w"], d["u"], d["gy"], H, d["cu"], d["max_seqlen"], ws=ws,
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
    lens2 = lens[:-1] + [200]                                             # the last sequence ends 130 rows early
    fit = sum(lens2)
    assert total - fit == 130
    short = dict(d, lens=lens2, cu=torch.from_numpy(cu_of(lens2)).cuda(), **{n: d[n][:fit] for n in ("r", "k", "v", "w", "gy")})
    ref = run(ops, short)
    d["cu"].copy_(short["cu"])
    for n in ("r", "k", "v", "w", "gy"):
        d[n][fit:] = NAN
    y.fill_(NAN)
    for t in captured[:5]:
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    for n, t in zip(("y",) + GRADS, (y,) + tuple(captured[:4])):
        assert same(t[:fit], ref[n]), n
        assert not bool(t[fit:].view(torch.int16).any()), n
    assert same(captured[4], ref["gu"])
