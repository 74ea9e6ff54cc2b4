"""CPU tier of the beam-search candidate entry points (include/wkv6_amd.h: rwkv6_beam_candidates_bf16 / _fp16 / _fp32 and
rwkv6_beam_candidates_workspace_bytes): the symbols are exported with the documented argument lists, every documented refusal returns its
code before anything is launched and in the documented order, and mix_op.beam_candidates refuses what it can see is wrong before it calls
the library.

The pointers passed to the library are dummies (multiples of 64 far apart, never dereferenced), as in test_sample_slots_cpu.py."""
import ctypes
import os
import re

import pytest
import torch

EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4
LOGITS, POOL, WS = 1 << 40, 2 << 40, 3 << 40
CUM, CU, SLOT, PEN, PARENT, TOKEN, SCORE = ((4 << 40) + i * (1 << 30) for i in range(7))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rwkv6_beam_candidates_bf16", "rwkv6_beam_candidates_fp16", "rwkv6_beam_candidates_fp32")
BIG = 1 << 30


@pytest.fixture(scope="module")
def lib():
    from rwkv_lm_ext_amd import _lib
    return _lib.load()


def args(n_rows=6, V=997, ld=1000, logits=LOGITS, cum=CUM, n_groups=2, cu=CU, K=5, pool=POOL, n_slots=9, slot=SLOT, pen=PEN, parent=PARENT,
         token=TOKEN, score=SCORE, ws=WS, ws_bytes=BIG):
    return (n_rows, V, ld, logits, cum, n_groups, cu, K, pool, n_slots, slot, pen, parent, token, score, ws, ws_bytes, None)


def test_symbols_and_signatures(lib):
    from rwkv_lm_ext_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "wkv6_amd.h")).read()
    I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    argtypes = [I, I, I, VP, VP, I, VP, I, VP, I, VP, VP, VP, VP, VP, VP, SZ, VP]
    params = ["int n_rows", "int V", "int ld", "const void* logits", "const float* cum", "int n_groups", "const int* cu_rows", "int K",
              "const float* occ_pool", "int n_slots", "const int* slot", "const float* penalty", "int* parent", "int* token", "float* score",
              "void* workspace", "size_t workspace_bytes", "void* stream"]
    for name in NAMES:
        fn = getattr(lib, name)
        res, table = _lib.SIGNATURES[name]
        assert res is I and list(table) == argtypes
        assert fn.restype is I and list(fn.argtypes) == argtypes
        decl = re.search("int " + name + r"\(([^;]*)\);", header).group(1)
        assert [" ".join(p.split()) for p in decl.split(",")] == params
    name = "rwkv6_beam_candidates_workspace_bytes"
    assert _lib.SIGNATURES[name] == (SZ, [I, I]) and getattr(lib, name).restype is SZ
    assert re.search(r"size_t " + name + r"\(int n_rows, int K\);", header)
    assert "wkv6_beam.hip" in _build.SOURCES and "wkv6_beam.h" in _build.HEADERS


def test_workspace_bytes(lib):
    ws = lib.rwkv6_beam_candidates_workspace_bytes
    for n_rows, K in ((0, 5), (-1, 5), (3, 0), (3, 65), (3, -1)):
        assert ws(n_rows, K) == 0, (n_rows, K)
    for n_rows, K in ((1, 1), (10, 30), (80, 30), (64, 64), (1000, 64)):
        got = ws(n_rows, K)
        assert got >= 2 * 4 * n_rows * K and got % 256 == 0 and got <= 2 * 4 * n_rows * K + 512, (n_rows, K, got)
    assert ws(81, 30) >= ws(80, 30) and ws(80, 31) >= ws(80, 30)


@pytest.mark.parametrize("name", NAMES)
def test_refusals_and_their_order(lib, name):
    fn = getattr(lib, name)
    size = 4 if name.endswith("fp32") else 2
    need = lib.rwkv6_beam_candidates_workspace_bytes(6, 5)
    assert fn(*args(logits=None)) == ENULL and fn(*args(ws_bytes=0)) == EWORKSPACE         # the arguments are good up to the probe
    # (1) WKV6_EINVAL: sizes ...
    for kw in ({"n_rows": 0}, {"n_rows": -1}, {"V": 0}, {"V": -5}, {"n_groups": 0}, {"n_groups": -2}, {"ld": 996}, {"ld": 992}, {"ld": 1004},
               {"V": 1000, "ld": 999}, {"K": 0}, {"K": -1}, {"K": 65}, {"n_slots": 0}, {"n_slots": -2}, {"slot": None, "n_slots": 5}):
        assert fn(*args(**kw)) == EINVAL, kw
        assert fn(*args(**dict(kw, logits=None))) == EINVAL, kw              # ... in front of the NULL check
        assert fn(*args(**dict(kw, ws_bytes=0))) == EINVAL, kw               # ... and of the workspace check
    assert fn(*args(V=70000, ld=70004)) == EINVAL                            # ... and of the vocabulary limit
    assert fn(*args(V=70000, ld=70000, K=65)) == EINVAL
    assert fn(*args(slot=None, n_slots=6, token=None)) == ENULL              # n_slots == n_rows is enough
    assert fn(*args(pool=None, slot=None, pen=None, n_slots=0, token=None)) == ENULL       # without a pool n_slots is not judged
    assert fn(*args(K=64, ws_bytes=0)) == EWORKSPACE and fn(*args(K=1, ws_bytes=0)) == EWORKSPACE
    # ... alignment: 16 bytes for logits and the pool, 4 for the rest ...
    for p, base in (("logits", LOGITS), ("pool", POOL)):
        for off in (1, 2, 4, 8, 12):
            assert fn(*args(**{p: base + off})) == EINVAL, (p, off)
            assert fn(*args(**dict({p: base + off}, cum=None))) == EINVAL, (p, off)
    rest = dict(cum=CUM, cu=CU, slot=SLOT, pen=PEN, parent=PARENT, token=TOKEN, score=SCORE, ws=WS)
    for p, base in rest.items():
        for off in (1, 2, 3):
            assert fn(*args(**{p: base + off})) == EINVAL, (p, off)
            assert fn(*args(**dict({p: base + off}, V=70000, ld=70000))) == EINVAL, (p, off)
        assert fn(*args(**dict({p: base + 4}, V=70000, ld=70000))) == EUNSUPPORTED, p       # 4-byte aligned: accepted so far
    # ... and the outputs and the workspace against every input: touching at either end is an overlap, adjacent is not (probed through
    # the check that comes next)
    n_rows, ld, n_groups, K, n_slots = 6, 1000, 2, 5, 9
    ins = dict(logits=(LOGITS, n_rows * ld * size), cum=(CUM, n_rows * 4), cu=(CU, (n_groups + 1) * 4), pool=(POOL, n_slots * ld * 4),
               slot=(SLOT, n_rows * 4), pen=(PEN, n_groups * 4))
    outs = dict(parent=n_groups * K * 4, token=n_groups * K * 4, score=n_groups * K * 4, ws=need)
    for o, o_bytes in outs.items():
        for i, (base, i_bytes) in ins.items():
            for at in (base, base - o_bytes + 4, base + i_bytes - 4):
                assert fn(*args(**{o: at})) == EINVAL, (o, i, at)
                assert fn(*args(**{o: at, "ws_bytes": 0})) == EINVAL, (o, i, at)
            for at in (base - o_bytes, base + i_bytes):
                assert fn(*args(**{o: at, "ws_bytes": 0})) == EWORKSPACE, (o, i, at)
    # (2) WKV6_EUNSUPPORTED: V > 65536, in front of the NULL check
    for V in (65537, 65544, 1 << 20):
        ld = (V + 7) // 8 * 8
        assert fn(*args(V=V, ld=ld)) == EUNSUPPORTED, V
        assert fn(*args(V=V, ld=ld, logits=None, cum=None)) == EUNSUPPORTED, V
        assert fn(*args(V=V, ld=ld, pen=None)) == EUNSUPPORTED, V
    assert fn(*args(V=65536, ld=65536, cum=None)) == ENULL                   # the limit itself goes on to the next check
    # (3) WKV6_ENULL: a missing pointer, or a partial penalty triple ...
    for p in ("logits", "cum", "cu", "parent", "token", "score", "ws"):
        assert fn(*args(**{p: None})) == ENULL, p
        assert fn(*args(**{p: None, "ws_bytes": 0})) == ENULL, p             # ... in front of the workspace check
    for kw in ({"pool": None}, {"pen": None}, {"pool": None, "pen": None}, {"pool": None, "slot": None}, {"pen": None, "slot": None}):
        assert fn(*args(**kw)) == ENULL, kw
        assert fn(*args(**dict(kw, ws_bytes=0))) == ENULL, kw
    # (4) WKV6_EWORKSPACE; the whole triple and slot alone may be NULL
    for kw in ({}, {"slot": None}, {"pool": None, "slot": None, "pen": None}):
        assert fn(*args(**dict(kw, ws_bytes=need - 1))) == EWORKSPACE, kw
        assert fn(*args(**dict(kw, ws_bytes=0))) == EWORKSPACE, kw


def test_beam_candidates_refuses_before_calling_the_library(monkeypatch):
    from rwkv_lm_ext_amd import _lib, mix_op

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", no_library)
    bf, i32 = torch.bfloat16, torch.int32
    n, V, ld, n_slots, G = 6, 997, 1000, 7, 2
    good = dict(logits=torch.zeros(n, ld, dtype=bf)[:, :V], cum=torch.zeros(n), cu=torch.tensor([0, 3, 6], dtype=i32), K=5,
                pool=torch.zeros(n_slots, ld)[:, :V], slots=torch.zeros(n, dtype=i32), penalty=torch.ones(G))

    def call(**o):
        a = dict(good, **o)
        return mix_op.beam_candidates(a["logits"], a["cum"], a["cu"], a["K"], occ_pool=a["pool"], slots=a["slots"], penalty=a["penalty"])

    with pytest.raises(RuntimeError, match="must be on the GPU"):            # everything else is right: no CPU path
        call()
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        call(pool=None, slots=None, penalty=None, logits=torch.zeros(n, ld)[:, :V])
    for bad in (good["logits"].double(), torch.zeros(n, ld, dtype=bf)[:, :V].t(), torch.zeros(ld, dtype=bf)[:V], torch.zeros(n, 0, dtype=bf), None):
        with pytest.raises(RuntimeError, match="logits must be"):
            call(logits=bad)
    for bad in (torch.zeros(n, V, dtype=bf), torch.zeros(n, 1004, dtype=bf)[:, :V]):
        with pytest.raises(RuntimeError, match="rows must lie ld elements apart"):
            call(logits=bad)
    with pytest.raises(RuntimeError, match="at most 65536"):
        call(logits=torch.zeros(n, 65544, dtype=bf), pool=torch.zeros(n_slots, 65544))
    for bad in (0, 65, -1, 5.0, None):
        with pytest.raises(RuntimeError, match="K must be"):
            call(K=bad)
    for bad in (good["cum"].double(), torch.zeros(n + 1), torch.zeros(2 * n)[::2], 0.5):
        with pytest.raises(RuntimeError, match="cum must be"):
            call(cum=bad)
    for bad in (good["cu"].long(), torch.zeros(1, dtype=i32), torch.zeros(6, dtype=i32)[::2], [0, 3, 6]):
        with pytest.raises(RuntimeError, match="cu_rows must be"):
            call(cu=bad)
    for kw in ({"pool": None}, {"penalty": None}, {"pool": None, "penalty": None}):
        with pytest.raises(RuntimeError, match="go together"):
            call(**kw)
    for bad in (good["pool"].double(), torch.zeros(n_slots, ld)[:, :V - 1], torch.zeros(n_slots, 1008)[:, :V], torch.zeros(n_slots, V), torch.zeros(ld)[:V]):
        with pytest.raises(RuntimeError, match="occ_pool must be"):
            call(pool=bad)
    for bad in (good["penalty"].double(), torch.ones(G + 1), torch.ones(2 * G)[::2], 1.1):
        with pytest.raises(RuntimeError, match="penalty must be"):
            call(penalty=bad)
    with pytest.raises(RuntimeError, match="slots = None"):
        call(slots=None, pool=torch.zeros(2, ld)[:, :V])
    for bad in (good["slots"].long(), torch.zeros(n + 1, dtype=i32), torch.zeros(2 * n, dtype=i32)[::2], [0] * n):
        with pytest.raises(RuntimeError, match="slots must be"):
            call(slots=bad)
    for t in ("logits", "cum", "pool", "penalty"):
        with pytest.raises(RuntimeError, match="has no backward"):
            call(**{t: (torch.zeros(n, ld, requires_grad=True)[:, :V] if t == "logits" else good[t].detach().requires_grad_())})
    with torch.no_grad(), pytest.raises(RuntimeError, match="must be on the GPU"):      # ... which no_grad lifts
        call(cum=good["cum"].clone().requires_grad_())
