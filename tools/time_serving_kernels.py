"""The serving kernels that share csrc/wkv6_tile16.h and csrc/wkv6_rows.h -- per-sequence LoRA (wkv6_lora.hip), the low-rank time-mix pairs
(wkv6_lowrank.hip), the sampler (wkv6_sample.hip) and the beam-search candidates (wkv6_beam.hip) -- of this tree's library against another
build of the library, normally the parent commit's: first every output bit for bit, then the time per call.

Both libraries are loaded through ctypes in one process and called with pre-bound arguments on the same inputs.  Equality: every output
buffer starts from the same contents on each side (NaN, or what the call updates in place: y of the LoRA pair, the occurrence pool of the
sampler) and is compared as bits; the first difference is printed and the exit code is 1.  Of the beam kernels' workspace the two lists of
n_rows x K entries are compared, not the padding between them.  The inputs are the GPU tests' own (tests/lora_common.py,
tests/lowrank_common.py, tests/sample_numpy.py, tests/beam_numpy.py and the tie rows of tests/test_sample_slots_gpu.py).  Speed: the method
of tools/timing.py, --repeats rounds of parent, tree and parent again ("parent-2").  A row is "level" when the tree's median lies inside the
parent's min..max or differs from the parent's by less than parent-2's does.

    git archive <parent> | tar -x -C build_ab/parent_tree
    bash tools/build_tree_variant.sh parent build_ab/parent_tree/rwkv_lm_ext_amd/csrc ""
    python tools/time_serving_kernels.py --parent-lib build_ab/parent/lib.so [--out profiles/serving_kernels_fold.txt]

--dry: no GPU and no library -- the cases are built on the CPU and every call is checked against the argument lists of
rwkv_lm_ext_amd/_lib.py (a rehearsal of the tool itself).
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import timing
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beam_numpy as bn                    # noqa: E402
import lora_common as lc                   # noqa: E402
import lowrank_common as lw                # noqa: E402
import sample_numpy as sn                  # noqa: E402
from test_sample_slots_gpu import tie_row  # noqa: E402
from rwkv_lm_ext_amd import _lib           # noqa: E402

bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = {"bf16": bf, "fp16": f16, "fp32": f32}
SIGS = _lib.SIGNATURES


class Lib:
    """One build of the library, typed from the binding's tables."""

    def __init__(self, path):
        self.h = timing.load_library(path, SIGS)

    def size(self, name, *args):
        return getattr(self.h, name)(*args)

    def bind(self, name, *args):
        return timing.bound(getattr(self.h, name), *args)


class DryLib:
    """--dry: checks the number of arguments of every call, launches nothing."""

    def size(self, name, *args):
        assert len(args) == len(SIGS[name][1]), name
        return 1 << 20

    def bind(self, name, *args):
        assert len(args) == len(SIGS[name][1]), (name, len(args), len(SIGS[name][1]))
        for a, t in zip(args, SIGS[name][1]):
            assert a is None or isinstance(a, int), (name, a)
            assert t is ctypes.c_void_p or a is not None, (name, "None for a scalar")
        return lambda: None


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def first_difference(a, b):
    """None when a and b hold the same bits, else a description of the first element that differs."""
    x, y = bits(a).flatten(), bits(b).flatten()
    if torch.equal(x, y):
        return None
    i = int((x != y).nonzero()[0])
    return f"{int((x != y).sum())} of {x.numel()} elements differ, first at flat index {i}: {a.flatten()[i].item()!r} vs {b.flatten()[i].item()!r}"


TIES = {64: (2, 4, 3, 4), 997: (3, 40, 20, 24), 65536: (2, 300, 50, 151)}          # V: n_top, n_tied, n_low, k of test_ties_that_straddle_*


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", required=True, help="the other build of librwkv6_amd.so (tools/build_tree_variant.sh)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warm", type=float, default=0.3, help="seconds of warm-up per contender")
    ap.add_argument("--per-timing", type=float, default=0.05, help="seconds of back-to-back calls per timing (at least 3 calls)")
    ap.add_argument("--no-speed", action="store_true", help="the equality pass only")
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    log = timing.Log()
    say = log.say

    if a.dry:
        device, stream = "cpu", 0
        tree, parent = DryLib(), DryLib()
        assert first_difference(torch.zeros(4), torch.zeros(4)) is None and first_difference(torch.zeros(4), torch.tensor([0., 0, 1, 0]))
        assert first_difference(torch.full((3,), float("nan")), torch.full((3,), float("nan"))) is None
    else:
        device = "cuda"
        tree, parent = Lib(_lib.load()._name), Lib(a.parent_lib)
        stream = torch.cuda.current_stream().cuda_stream
        say(timing.device_header())
        say(f"tree: {_lib.load()._name}")
        say(f"parent: {os.path.abspath(a.parent_lib)}")
    keep = []                                              # every buffer a bound call points into

    def p(t):
        return None if t is None else t.data_ptr()

    def dev(t):
        t = (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).contiguous().to(device)
        keep.append(t)
        return t

    def ints(xs):
        return dev(torch.tensor([int(v) for v in xs], dtype=torch.int32))

    def out(*shape, dtype=f32):
        return dev(torch.full(shape, float("nan"), dtype=dtype))

    def scratch(nbytes):
        return dev(torch.full((max(int(nbytes), 16),), 0x5a, dtype=torch.uint8))

    def padded(x, ld, fill, dtype):
        """[n, V] values as the first V columns of a [n, ld] tensor of `dtype`"""
        x = torch.from_numpy(np.ascontiguousarray(x, np.float32)) if isinstance(x, np.ndarray) else x
        t = torch.full((x.shape[0], ld), fill, dtype=dtype)
        t[:, :x.shape[1]] = x.to(dtype)
        return dev(t)

    # ---- the cases: build(lib) -> (outputs {name: tensor}, [bound calls]); build is called once per side ------------------------------------
    def lora(K, N, R, cu, adapters, total, n_adapters, tensors=None):
        x, y0, A, B, scale = (dev(t) for t in (tensors or lc.case(K, N, R, total, n_adapters=n_adapters)))
        cu_d, ad_d = ints(cu), ints(adapters)

        def build(L):
            o = {"y": dev(y0.clone())}
            ws = scratch(L.size("wkv6_lora_packed_workspace_bytes", total, R))
            return o, [L.bind("wkv6_lora_packed_bf16", total, len(adapters), K, N, R, n_adapters, p(cu_d), p(ad_d), p(x), p(A), p(B), p(scale), p(o["y"]), p(ws),
                              ws.numel(), stream)]
        return build

    def lerp(C, D, rows, packed, tensors=None):
        """dense: 3 sequences of rows / 3 with a front token each; packed: the batch CU / SLOTS of the parity tests over a pool of 4"""
        q = tensors or lw.make_inputs(C, D, 64, rows)
        W1t, W2t, _, _ = lw.kernel_weights(q)
        x, front, maa_x, maa5, W1t, W2t = (dev(t) for t in (q["x"], q["front"], q["maa_x"], q["maa5"], W1t, W2t))
        if packed:
            cu = tensors["cu"] if tensors else lw.cu_of(rows)
            slots = tensors["slots"] if tensors else lw.SLOTS
            cu_d, sl_d, n_seq = ints(cu), ints(slots), len(cu) - 1
        else:
            cu_d, sl_d, n_seq = None, None, tensors["n_seq"] if tensors else 3
        assert packed or (rows % n_seq == 0 and front.shape[0] >= n_seq)

        def build(L):
            o = {"out": out(5, rows, C, dtype=bf)}
            ws = scratch(L.size("wkv6_lowrank_workspace_bytes", rows, 5 * D))
            return o, [L.bind("wkv6_tmix_lerp_lowrank_bf16", rows, n_seq, C, D, p(cu_d), p(x), p(front), front.shape[0], p(sl_d), p(maa_x), p(W1t), p(W2t), p(maa5),
                              p(o["out"]), p(ws), ws.numel(), stream)]
        return build

    def decay(C, N, Dd, rows):
        q = lw.make_inputs(C, 32, Dd, rows, N=N)
        _, _, D1t, D2t = lw.kernel_weights(q)
        xw, D1t, D2t, td = (dev(t) for t in (q["x"], D1t, D2t, q["time_decay"]))

        def build(L):
            o = {"w": out(rows, N, dtype=bf)}
            ws = scratch(L.size("wkv6_lowrank_workspace_bytes", rows, Dd))
            return o, [L.bind("wkv6_decay_lowrank_bf16", rows, C, Dd, N, p(xw), p(D1t), p(D2t), p(td), p(o["w"]), p(ws), ws.numel(), stream)]
        return build

    def sample(rows, dname, slots=None, slots_out=None):
        """rows: (logits [V], o [V], params [8], u) each; the pool holds one slot per row and as many again, filled with 9, behind them"""
        V, n = rows[0][0].shape[0], len(rows)
        ld = (V + 7) // 8 * 8
        lg = padded(np.stack([r[0] for r in rows]), ld, 77.0, DTYPES[dname])
        pool0 = padded(np.concatenate([np.stack([r[1] for r in rows]), np.full((n, V), 9.0, np.float32)]), ld, -5.0, f32)
        params, u = dev(np.stack([r[2] for r in rows]).astype(np.float32)), dev(np.array([r[3] for r in rows], np.float32))
        sl, so = (None if s is None else ints(s) for s in (slots, slots_out))

        def build(L):
            o = {"tokens": dev(torch.full((n,), -7, dtype=torch.int32)), "logprob": out(n), "pool": dev(pool0.clone())}
            return o, [L.bind("rwkv6_sample_slots_" + dname, n, V, ld, p(lg), p(o["pool"]), 2 * n, p(sl), p(so), p(params), p(u), p(o["tokens"]), p(o["logprob"]), stream)]
        return build

    def sample_rows(V, dname):
        """top-p alone, top-k alone, both, greedy, the two tie rows under three draws each, a poisoned row, and rows of the tests' family"""
        rng = np.random.default_rng(V + ord(dname[0]))
        rows = [sn.make_case(rng, V, DTYPES[dname]) for _ in range(6)]
        lg, o, prm, u = sn.make_case(rng, V, DTYPES[dname])
        k = min(5, V - 1)
        for t, top_p, top_k in ((1.0, 0.85, 0), (1.0, 1.0, k), (0.7, 0.85, k), (0.0, 0.9, k)):
            q = prm.copy()
            q[0], q[1], q[2] = t, top_p, top_k
            rows.append((lg, o, q, u))
        n_top, n_tied, n_low, k = TIES[V]
        tl, top, tied = tie_row(V, n_top, n_tied, n_low, np.random.default_rng(V))
        tl = sn.round_to(tl, DTYPES[dname])
        pr = np.exp(tl.astype(np.float64))
        pr /= pr.sum()
        cut = np.array([1.0, pr[top].sum() + 0.4 * pr[tied].sum(), 0, 0, 0, 1, 1, 0], np.float32)
        for uu in (0.01, 0.5, 0.999):
            rows.append((tl, np.zeros(V, np.float32), cut, uu))
            rows.append((tl, np.zeros(V, np.float32), np.array([1.0, 1.0, k, 0, 0, 1, 1, 0], np.float32), uu))
        bad = lg.copy()
        bad[min(3, V - 1)] = np.nan
        rows.append((bad, o, prm, u))
        return rows

    def beam(d, K, dname):
        n_rows, V = d["logits"].shape
        ld, n_groups = (V + 7) // 8 * 8, len(d["cu"]) - 1
        lg = padded(d["logits"], ld, 77.0, DTYPES[dname])
        cum, cu = dev(d["cum"].astype(np.float32)), ints(d["cu"])
        occ = slot = pen = None
        n_slots = 0
        if d["occ"] is not None:
            occ, pen, n_slots = padded(d["occ"], ld, 5.0, f32), dev(d["penalty"].astype(np.float32)), d["occ"].shape[0]
            slot = None if d["slot"] is None else ints(d["slot"])

        def build(L):
            o = {n: dev(torch.full((n_groups, K), -7, dtype=torch.int32)) for n in ("parent", "token")}
            o["score"] = out(n_groups, K)
            ws = scratch(L.size("rwkv6_beam_candidates_workspace_bytes", n_rows, K))
            lists = ws.view(torch.int32)
            half = (n_rows * K * 4 + 255) // 256 * 256 // 4                    # the second list starts on the next multiple of 256 bytes
            o["keys"], o["ids"] = lists[:n_rows * K], lists[half:half + n_rows * K]
            return o, [L.bind("rwkv6_beam_candidates_" + dname, n_rows, V, ld, p(lg), p(cum), n_groups, p(cu), K, p(occ), n_slots, p(slot), p(pen), p(o["parent"]),
                              p(o["token"]), p(o["score"]), p(ws), ws.numel(), stream)]
        return build

    def beam_edge_rows(dname):
        """the rows of test_dead_poisoned_and_short_rows"""
        V = 1003
        rng = np.random.default_rng(3)
        lg = bn.round_to(rng.normal(0, 2, (8, V)), dname)
        lg[0, 5:], lg[1], lg[2, 3], lg[4], lg[5, 900] = -np.inf, np.nan, np.inf, -np.inf, np.nan
        lg[6, ::2] = -np.inf
        return dict(logits=lg, cum=np.array([-1, -np.inf, -2, -3, -4, -5, -6, -7], np.float32), cu=np.array([0, 2, 4, 6, 8], np.int32), occ=None, slot=None,
                    penalty=None)

    cases = []
    many_cu, many_ad = (list(v) for v in lc.many_batch())
    for K, N, R in ((64, 64, 8), (576, 1088, 64), (2688, 768, 16)):
        t = f"lora K{K} N{N} R{R}"
        cases.append((f"{t} 1 row", lora(K, N, R, [0, 1], [2], 1, lc.N_ADAPTERS)))
        cases.append((f"{t} 17 rows, the last on an adapter outside the pool", lora(K, N, R, [0, 16, 17], [2, lc.N_ADAPTERS], 17, lc.N_ADAPTERS)))
        cases.append((f"{t} 75 rows, sixteen adapters in a tile", lora(K, N, R, lc.cu_of(lc.GROUPS_LENS, 0), lc.GROUPS_ADAPTERS, lc.GROUPS_TOTAL, lc.MANY_ADAPTERS)))
        cases.append((f"{t} 4100 rows, adapters -1, 20 and INT_MIN among them", lora(K, N, R, many_cu, many_ad, lc.MANY_TOTAL, lc.MANY_ADAPTERS)))
    for C, D in ((64, 32), (576, 64), (768, 32), (4096, 32)):
        cases.append((f"lowrank lerp C{C} D{D} dense 3 x 11 rows", lerp(C, D, 33, False)))
        cases.append((f"lowrank lerp C{C} D{D} packed 33 rows, cu_seqlens and a slot pool", lerp(C, D, 33, True)))
    for C, N in ((768, 512), (64, 4096)):
        cases.append((f"lowrank decay C{C} N{N} Dd64 33 rows", decay(C, N, 64, 33)))
    for V in (64, 997, 65536):
        for dname in DTYPES:
            rows = sample_rows(V, dname)
            n = len(rows)
            cases.append((f"sample {dname} V{V} {n} rows: top-p, top-k, both, greedy, ties, poisoned", sample(rows, dname)))
            # (read from the first half of the pool, written to the second: no sequence reads a row that another writes)
            cases.append((f"sample {dname} V{V} {n} rows, permuted slots into other output slots, one of each outside the pool",
                          sample(rows, dname, slots=[(i + 1) % n for i in range(n - 1)] + [2 * n], slots_out=[n + i for i in range(n - 1)] + [-1])))
    for dname in DTYPES:
        for V in (9, 1000, 65536):
            for penalty in (False, True):
                d = bn.make_inputs(V + 7 * penalty + ord(dname[0]), [0, 2, 2, 7], V, dname, penalty=penalty)
                for K in (1, 30):
                    cases.append((f"beam {dname} V{V} K{K} groups of 2, 0, 5 rows" + (", penalty" if penalty else ""), beam(d, K, dname)))
        z = np.random.default_rng(11).integers(-8, 3, 1000).astype(np.float32) * 0.5
        same = dict(logits=np.stack([z] * 3), cum=np.array([-1.0] * 3, np.float32), cu=np.array([0, 3], np.int32), occ=None, slot=None, penalty=None)
        cases.append((f"beam {dname} V1000 K30 three identical rows", beam(same, 30, dname)))
        cases.append((f"beam {dname} V1003 K30 dead, poisoned and short rows", beam(beam_edge_rows(dname), 30, dname)))

    def sync():
        if not a.dry:
            torch.cuda.synchronize()

    say()
    say(f"equality: {len(cases)} cases, every output of the tree's library against the parent's, as bits")
    bad = 0
    n_out = 0
    for title, build in cases:
        sides = []
        for L in (parent, tree):
            o, calls = build(L)
            for c in calls:
                c()
            sync()
            sides.append(o)
        diffs = {n: first_difference(sides[0][n], sides[1][n]) for n in sides[0]}
        n_out += len(diffs)
        wrong = {n: d_ for n, d_ in diffs.items() if d_}
        bad += len(wrong)
        say(f"  {'same' if not wrong else 'DIFFERENT':9s} {title}: {', '.join(diffs)}")
        for n, d_ in wrong.items():
            say(f"            {n}: {d_}")
    say(f"equality: {n_out - bad} of {n_out} outputs identical" + ("" if not bad else f", {bad} DIFFERENT"))
    if bad or a.no_speed:
        log.write(a.out)
        sys.exit(1 if bad else 0)

    # ---- speed -------------------------------------------------------------------------------------------------------------------------
    rows = []
    toy = a.dry                                             # (--dry builds the rows at a toy size and stops in front of the timing)
    g = torch.Generator().manual_seed(0)

    def each(title, build):
        sides = {name: build(L)[1][0] for name, L in (("parent", parent), ("tree", tree), ("parent-2", parent))}
        rows.append((title, sides))

    KN, C, V = (64, 64, 64) if toy else (2048, 2048, 65536)
    for n_ad in (1, 16):
        T = 256
        tensors = (torch.randn(T, KN, generator=g).to(bf), torch.randn(T, KN, generator=g).to(bf), (torch.randn(n_ad, 8, KN, generator=g) / KN ** 0.5).to(bf),
                   (torch.randn(n_ad, KN, 8, generator=g) / 8 ** 0.5).to(bf), torch.ones(n_ad))
        each(f"lora 256 decode rows K = N = {KN} r8, {n_ad} adapter" + ("s" if n_ad > 1 else ""),
             lora(KN, KN, 8, list(range(T + 1)), [i % n_ad for i in range(T)], T, n_ad, tensors=tensors))
    for n_rows, packed in ((256, True), (16 if toy else 8192, False)):
        q = lw.make_inputs(C, 32, 64, n_rows, n_front=256 if packed else 8)
        q.update(cu=list(range(n_rows + 1)), slots=list(range(n_rows)), n_seq=8)
        each(f"lowrank lerp C{C} D32 " + ("256 decode rows, slot pool" if packed else f"8 x {n_rows // 8} rows dense"), lerp(C, 32, n_rows, packed, tensors=q))
        each(f"lowrank decay C{C} N{C} Dd64 {n_rows} rows", decay(C, C, 64, n_rows))
    rng = np.random.default_rng(0)
    for n_seq in (1, 256):
        base = [sn.make_case(rng, V, bf) for _ in range(n_seq)]
        for what, t, top_p, k in (("top-p 0.85 + top-k 50", 1.0, 0.85, min(50, V - 1)), ("greedy", 0.0, 1.0, 0)):
            sel = []
            for lg, o, prm, u in base:
                lg = sn.round_to(rng.normal(0, 3, V), bf)       # a dense row: every pass has work to do
                q = prm.copy()
                q[0], q[1], q[2] = t, top_p, k
                sel.append((lg, o, q, u))
            each(f"sample bf16 V{V} {n_seq} sequence" + ("s" if n_seq > 1 else "") + f", {what}", sample(sel, "bf16"))
    for penalty in (False, True):
        d = bn.make_inputs(5, list(range(0, 81, 10)), V, "bf16", penalty=penalty, n_slots=80)
        each(f"beam bf16 V{V} 80 rows (8 x 10) K30" + (", penalty" if penalty else ""), beam(d, 30, "bf16"))

    if a.dry:
        say(f"speed: {len(rows)} rows built: " + "; ".join(t for t, _ in rows))
        return

    timed = lambda fn, iters: timing.event_time(fn, iters) * 1e3         # us per call
    say()
    say(f"speed: us per call, {a.repeats} rounds of parent, tree, parent-2; {a.warm:.1f} s warm-up each, about {a.per_timing * 1e3:.0f} ms of calls per timing")
    outside = 0
    for title, contenders in rows:
        for fn in contenders.values():
            timing.warm(fn, seconds=a.warm)
        iters = max(3, min(500, int(a.per_timing * 1e6 / max(timed(contenders["parent"], 3), 1.0))))
        res = timing.alternate(contenders, lambda fn: timed(fn, iters), a.repeats)
        med = {n: timing.median(xs) for n, xs in res.items()}
        spread = abs(med["parent-2"] - med["parent"])
        inside = min(res["parent"]) <= med["tree"] <= max(res["parent"])
        level = inside or abs(med["tree"] - med["parent"]) < spread
        faster = not level and med["tree"] < med["parent"]
        outside += not (level or faster)
        say(f"  {title}   ({iters} calls per timing)")
        for n, xs in res.items():
            say(f"    {n:9s} " + timing.stats(xs, 9, 2))
        say(f"    tree - parent = {med['tree'] - med['parent']:+.2f} us ({100 * (med['tree'] / med['parent'] - 1):+.2f} %), "
            f"|parent-2 - parent| = {spread:.2f} us, ranges {'apart' if timing.apart(res['tree'], res['parent']) else 'overlap'}: "
            f"{'level' if level else 'FASTER' if faster else 'SLOWER'}")
    say(f"speed: {len(rows) - outside} of {len(rows)} rows level or faster" + ("" if not outside else f", {outside} SLOWER (repeat the command once before judging)"))
    log.write(a.out)


if __name__ == "__main__":
    main()
