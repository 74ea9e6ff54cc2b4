"""CPU tier of the device-side sampler (include/wkv6_amd.h: rwkv6_sample_slots_bf16 / _fp16 / _fp32): the symbols are exported with the
documented argument lists, every documented refusal returns its code before anything is launched and in the documented order,
mix_op.sample_slots refuses what it can see is wrong before it calls the library, and the eager restatement infctx.sample_packed(
kernels=False) agrees with the numpy oracle of tests/sample_numpy.py on CPU tensors.

The pointers passed to the library are dummies (multiples of 64 far apart, never dereferenced), as in test_lora_packed_abi_cpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sample_numpy as sn

EINVAL, ENULL, EUNSUPPORTED = -1, -2, -4
LOGITS, POOL, P = 1 << 40, 2 << 40, 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rwkv6_sample_slots_bf16", "rwkv6_sample_slots_fp16", "rwkv6_sample_slots_fp32")
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def lib():
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


def args(n_seq=5, V=997, ld=1000, logits=LOGITS, pool=POOL, n_slots=9, slot=P, slot_out=P, params=P, u=P, tokens=P, logprob=P):
    return (n_seq, V, ld, logits, pool, n_slots, slot, slot_out, params, u, tokens, logprob, None)


def test_symbols_and_signatures(lib):
    from rwkv_lm_ext_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "wkv6_amd.h")).read()
    I, VP = ctypes.c_int, ctypes.c_void_p
    argtypes = [I, I, I, VP, VP, I, VP, VP, VP, VP, VP, VP, VP]
    params = ["int n_seq", "int V", "int ld", "const void* logits", "float* occ_pool", "int n_slots", "const int* slot", "const int* slot_out",
              "const float* params", "const float* u", "int* tokens", "float* logprob", "void* stream"]
    for name in NAMES:
        fn = getattr(lib, name)
        res, table = _lib.SIGNATURES[name]
        assert res is I and list(table) == argtypes
        assert fn.restype is I and list(fn.argtypes) == argtypes
        decl = re.search("int " + name + r"\(([^;]*)\);", header).group(1)
        assert [" ".join(p.split()) for p in decl.split(",")] == params
    assert "wkv6_sample.hip" in _build.SOURCES and "wkv6_sample.h" in _build.HEADERS


@pytest.mark.parametrize("name", NAMES)
def test_refusals_and_their_order(lib, name):
    fn = getattr(lib, name)
    size = 4 if name.endswith("fp32") else 2
    # (1) WKV6_EINVAL: sizes ...
    for kw in ({"n_seq": 0}, {"n_seq": -1}, {"V": 0}, {"V": -5}, {"n_slots": 0}, {"n_slots": -2}, {"ld": 996}, {"ld": 992}, {"ld": 1004},
               {"V": 1000, "ld": 999}, {"slot": None, "n_slots": 4}):
        assert fn(*args(**kw)) == EINVAL, kw
        assert fn(*args(**dict(kw, logits=None))) == EINVAL, kw              # ... in front of the NULL check
    assert fn(*args(V=70000, ld=70004)) == EINVAL                            # ... and of the vocabulary limit
    assert fn(*args(V=70000, ld=70000, n_seq=0)) == EINVAL
    assert fn(*args(slot=None, n_slots=5, tokens=None)) == ENULL             # n_slots == n_seq is enough
    # ... alignment: 16 bytes for logits and the pool, 4 for the rest ...
    for p, base in (("logits", LOGITS), ("pool", POOL)):
        for off in (1, 2, 4, 8, 12):
            assert fn(*args(**{p: base + off})) == EINVAL, (p, off)
            assert fn(*args(**dict({p: base + off}, u=None))) == EINVAL, (p, off)
    for p in ("slot", "slot_out", "params", "u", "tokens", "logprob"):
        for off in (1, 2, 3):
            assert fn(*args(**{p: P + off})) == EINVAL, (p, off)
            assert fn(*args(**dict({p: P + off}, V=70000, ld=70000))) == EINVAL, (p, off)
        assert fn(*args(**dict({p: P + 4}, V=70000, ld=70000))) == EUNSUPPORTED, p          # 4-byte aligned: accepted so far
    # ... and the pool [n_slots,ld] fp32 against logits [n_seq,ld]: touching at either end is an overlap, adjacent is not (probed through the
    # check that comes next)
    n_seq, ld, n_slots = 5, 1000, 9
    for pool in (LOGITS, LOGITS - n_slots * ld * 4 + 16, LOGITS + n_seq * ld * size - 16):
        assert fn(*args(pool=pool)) == EINVAL, pool
        assert fn(*args(pool=pool, params=None)) == EINVAL, pool
    for pool in (LOGITS - n_slots * ld * 4, LOGITS + n_seq * ld * size):
        assert fn(*args(pool=pool, params=None)) == ENULL, pool
    # (2) WKV6_EUNSUPPORTED: V > 65536, in front of the NULL check
    for V in (65537, 65544, 1 << 20):
        ld = (V + 7) // 8 * 8
        assert fn(*args(V=V, ld=ld)) == EUNSUPPORTED, V
        assert fn(*args(V=V, ld=ld, logits=None, pool=None)) == EUNSUPPORTED, V
    assert fn(*args(V=65536, ld=65536, u=None)) == ENULL                     # the limit itself goes on to the next check
    # (3) WKV6_ENULL; slot, slot_out and logprob may be NULL
    for p in ("logits", "pool", "params", "u", "tokens"):
        assert fn(*args(**{p: None})) == ENULL, p
    assert fn(*args(slot=None, slot_out=None, logprob=None, tokens=None)) == ENULL


def test_sample_slots_refuses_before_calling_the_library(monkeypatch):
    from rwkv_lm_ext_amd import _lib, mix_op

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", no_library)
    bf, i32 = torch.bfloat16, torch.int32
    n, V, ld, n_slots = 3, 997, 1000, 4
    good = dict(logits=torch.zeros(n, ld, dtype=bf)[:, :V], pool=torch.zeros(n_slots, ld)[:, :V], slots=torch.zeros(n, dtype=i32),
                params=torch.ones(n, 8), u=torch.zeros(n), out_slots=None)

    def call(**o):
        a = dict(good, **o)
        return mix_op.sample_slots(a["logits"], a["pool"], a["slots"], a["params"], a["u"], out_slots=a["out_slots"])

    with pytest.raises(RuntimeError, match="must be on the GPU"):            # everything else is right: no CPU path
        call()
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        call(logits=torch.zeros(n, ld)[:, :V], slots=None, out_slots=good["slots"])
    for bad in (good["logits"].double(), torch.zeros(n, ld, dtype=bf)[:, :V].t(), torch.zeros(ld, dtype=bf)[:V], torch.zeros(n, 0, dtype=bf), None):
        with pytest.raises(RuntimeError, match="logits must be"):
            call(logits=bad)
    for bad in (torch.zeros(n, V, dtype=bf), torch.zeros(n, 1004, dtype=bf)[:, :V], torch.zeros((n - 1) * ld + V, dtype=bf).as_strided((n, V), (ld, 1))):
        with pytest.raises(RuntimeError, match="rows must lie ld elements apart"):
            call(logits=bad)
    with pytest.raises(RuntimeError, match="at most 65536"):
        call(logits=torch.zeros(1, 65544, dtype=bf), pool=torch.zeros(1, 65544))
    for bad in (good["pool"].double(), torch.zeros(n_slots, ld)[:, :V - 1], torch.zeros(n_slots, 1008)[:, :V], torch.zeros(n_slots, V), torch.zeros(ld)[:V],
                None):
        with pytest.raises(RuntimeError, match="occ_pool must be"):
            call(pool=bad)
    for bad in (good["params"].double(), torch.ones(n, 7), torch.ones(n + 1, 8), torch.ones(n, 16)[:, ::2], None):
        with pytest.raises(RuntimeError, match="params must be"):
            call(params=bad)
    for bad in (good["u"].double(), torch.zeros(n + 1), torch.zeros(2 * n)[::2], 0.5):
        with pytest.raises(RuntimeError, match="u must be"):
            call(u=bad)
    with pytest.raises(RuntimeError, match="slots = None"):
        call(slots=None, pool=torch.zeros(2, ld)[:, :V])
    for name in ("slots", "out_slots"):
        for bad in (good["slots"].long(), torch.zeros(n + 1, dtype=i32), torch.zeros(2 * n, dtype=i32)[::2], [0, 1, 2]):
            with pytest.raises(RuntimeError, match=name + " must be"):
                call(**{name: bad})
    for t in ("logits", "pool", "params", "u"):
        with pytest.raises(RuntimeError, match="has no backward"):
            call(**{t: (torch.zeros(n, ld, requires_grad=True)[:, :V] if t == "logits" else good[t].detach().requires_grad_())})
    with torch.no_grad(), pytest.raises(RuntimeError, match="must be on the GPU"):      # ... which no_grad lifts
        call(params=good["params"].clone().requires_grad_())


# ---- the eager restatement against the oracle, on CPU tensors
def eager(rows, dtype, ld, slots=None, out_slots=None, occ=None):
    from rwkv_lm_ext_amd import infctx
    n, V = len(rows), rows[0][0].shape[0]
    occ = np.stack([r[1] for r in rows]) if occ is None else occ
    lg = torch.full((n, ld), 77.0, dtype=dtype)
    lg[:, :V] = torch.from_numpy(np.stack([r[0] for r in rows])).to(dtype)
    pool = infctx.SamplingPool.create(occ.shape[0], V, "cpu", ld=ld)
    pool.occ.fill_(-5.0)
    pool.occ[:, :V] = torch.from_numpy(occ)
    tok, lp = infctx.sample_packed(lg, pool, slots, torch.from_numpy(np.stack([r[2] for r in rows])), torch.tensor([r[3] for r in rows]),
                                   out_slots=out_slots, kernels=False)
    assert tok.dtype == torch.int32 and lp.dtype == torch.float32
    assert (pool.occ[:, V:] == -5.0).all()
    return tok.numpy(), lp.numpy(), pool.occ[:, :V].numpy()


def small(case):
    """The cases the eager code (a sort per row on the CPU) is run on: every shape, up to 3 rows."""
    return case[3] <= 3


@pytest.mark.parametrize("dname,V,ld,n_seq", [c for c in sn.CASES if small(c)])
def test_eager_restatement_matches_the_oracle(dname, V, ld, n_seq):
    rows = sn.case_rows(dname, V, n_seq)
    tok, lp, occ = eager(rows, DTYPES[dname], ld)
    for s, r in enumerate(rows):
        want = sn.sample_row(*r)
        if want["decisive"]:
            assert tok[s] == want["token"], (s, r[2], r[3])
            assert abs(lp[s] - want["logprob"]) <= 1e-5
            assert np.allclose(occ[s], want["occ"], rtol=1e-6, atol=0)


def test_at_most_one_row_in_twenty_is_not_decisive():
    """The condition on the parametrisation, on the oracle alone: over all rows of sn.CASES."""
    total = open_rows = 0
    for dname, V, ld, n_seq in sn.CASES:
        for r in sn.case_rows(dname, V, n_seq):
            total += 1
            open_rows += not sn.sample_row(*r)["decisive"]
    print(open_rows, "of", total, "rows are not decisive")
    assert total > 2000 and open_rows <= 0.05 * total


def test_top_p_of_one_keeps_everything():
    """The first documented deviation: the reference's fp32 cumsum can stay under 1.0, its argmax of all-false is 0 and it goes greedy."""
    V = 64
    logits = np.linspace(0, -6, V).astype(np.float32)
    params = np.array([1.0, 1.0, 0, 0, 0, 1, 1, 0], np.float32)
    assert sn.sample_row(logits, np.zeros(V, np.float32), params, 0.5)["kept"].all()
    u = (np.arange(400) + 0.5) / 400
    tok, _, _ = eager([(logits, np.zeros(V, np.float32), params, float(x)) for x in u], torch.float32, V)
    want = [sn.sample_row(logits, np.zeros(V, np.float32), params, float(np.float32(x)))["token"] for x in u]
    assert tok.tolist() == want and len(set(want)) > 20 and max(want) > 40


def test_top_k_and_top_p_intersect():
    """The second: in the reference's generate(), min_tokens_to_keep = top_k makes top-p a no-op whenever top_k > 0."""
    V = 64
    logits = (np.arange(V) * -0.5).astype(np.float32)
    o = np.zeros(V, np.float32)
    for top_p, k, n_kept in ((0.5, 20, 2), (0.99, 3, 3), (0.9, 0, 5)):
        params = np.array([1.0, top_p, k, 0, 0, 1, 1, 0], np.float32)
        kept = sn.sample_row(logits, o, params, 0.5)["kept"]
        assert kept.sum() == n_kept and kept[:n_kept].all(), (top_p, k)
        u = (np.arange(200) + 0.5) / 200
        tok, _, _ = eager([(logits, o, params, float(x)) for x in u], torch.float32, V)
        assert set(tok.tolist()) == set(range(n_kept)), (top_p, k)


def test_eager_slots_poison_and_greedy():
    V, ld, n_slots = 61, 64, 5
    rng = np.random.default_rng(3)
    rows = [list(sn.make_case(rng, V, torch.float32)) for _ in range(5)]
    rows[4][0] = rows[4][0].copy()
    rows[4][0][7] = np.nan                                                    # poisoned: its destination keeps its bits
    rows[3][2] = rows[3][2].copy()
    rows[3][2][0] = 0.0                                                       # greedy
    occ = np.zeros((n_slots, V), np.float32)
    occ[2, [1, 5]] = 2.0, 0.5
    src, dst = [2, 2, -1, 0, 1], [0, 1, 3, n_slots, 4]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    tok, lp, after = eager([tuple(r) for r in rows], torch.float32, ld, slots=i32(src), out_slots=i32(dst), occ=occ)
    for s in range(5):
        o = occ[src[s]] if 0 <= src[s] < n_slots else np.zeros(V, np.float32)
        want = sn.sample_row(rows[s][0], o, rows[s][2], rows[s][3])
        if want["poisoned"]:
            assert tok[s] == -1 and np.isnan(lp[s]) and np.array_equal(after[dst[s]], occ[dst[s]])
            continue
        if want["decisive"]:
            assert tok[s] == want["token"] and abs(lp[s] - want["logprob"]) <= 1e-5, s
            if 0 <= dst[s] < n_slots:
                assert np.allclose(after[dst[s]], want["occ"], rtol=1e-6, atol=0), s
    assert np.array_equal(after[2], occ[2])                                  # a source that nobody writes
    assert lp[3] == 0.0 and tok[3] == sn.sample_row(rows[3][0], occ[0], rows[3][2], rows[3][3])["token"]


def test_sampling_pool_and_params():
    from rwkv_lm_ext_amd import infctx
    pool = infctx.SamplingPool.create(3, 50277, "cpu")
    assert tuple(pool.occ.shape) == (3, 50280) and pool.occ.dtype == torch.float32 and pool.vocab == 50277 and not pool.occ.any()
    assert tuple(infctx.SamplingPool.create(2, 65536, "cpu", ld=65536).occ.shape) == (2, 65536)
    for ld in (50277, 50284, 1000):
        with pytest.raises(ValueError):
            infctx.SamplingPool.create(3, 50277, "cpu", ld=ld)
    p = infctx.sampling_params(4, "cpu", temperature=0.7, top_p=0.85, top_k=50, alpha_decay=0.996)
    assert tuple(p.shape) == (4, 8) and p.dtype == torch.float32
    assert p[2].tolist() == [np.float32(v) for v in (0.7, 0.85, 50, 0, 0, 0.996, 1, 0)]
    assert [f.name for f in __import__("dataclasses").fields(infctx.PackedPools)] == ["shift_att", "shift_ffn", "wkv"]      # unchanged
