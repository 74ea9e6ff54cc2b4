"""The exact token-serial kernels (csrc/wkv6_scan.hip, csrc/wkv5_scan.hip) of this tree's library against another build of the library,
normally the parent commit's: first every output bit for bit, then the time per call.

Both libraries are loaded through ctypes in one process and called with pre-bound arguments on the same inputs.  Equality: every output
buffer is filled with NaN (a state pool: with the same initial states) before each side's call and compared as bits; the first difference is
printed and the exit code is 1.  Speed: the method of tools/timing.py, --repeats rounds of parent, tree and parent again ("parent-2").  A
row is "inside" when the tree's median is no further above the parent's than parent-2's is from the parent's.

    git archive <parent> | tar -x -C build_ab/parent_tree
    bash tools/build_tree_variant.sh parent build_ab/parent_tree/rwkv_lm_ext_amd/csrc ""
    python tools/time_scan_kernels.py --parent-lib build_ab/parent/lib.so [--out profiles/scan_fold_gpu.txt]

--dry: no GPU and no library -- the cases are built on the CPU and every call is checked against the argument lists of
rwkv_lm_ext_amd/_lib.py (a rehearsal of the tool itself).
"""
import argparse
import ctypes
import os
import sys

import timing
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rwkv_lm_ext_amd import _lib          # noqa: E402

bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
SUFFIX = {bf: "bf16", f16: "fp16", f32: "fp32"}
SIGS = {**_lib.SIGNATURES, **_lib.SIGNATURES_WKV5}


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
        return 64

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
    g = torch.Generator().manual_seed(0)
    keep = []                                              # every buffer a bound call points into

    def p(t):
        return None if t is None else t.data_ptr()

    def rnd(*shape, scale=0.5, dtype=f32):
        t = (torch.randn(*shape, generator=g) * scale).to(dtype).to(device)
        keep.append(t)
        return t

    def ints(xs):
        t = torch.tensor(xs, dtype=torch.int32, device=device)
        keep.append(t)
        return t

    def out(*shape, dtype=f32):
        t = torch.full(shape, float("nan"), dtype=dtype, device=device)
        keep.append(t)
        return t

    def scratch(nbytes):
        t = torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=device)
        keep.append(t)
        return t

    def problem(shape, H, io, gy=True):
        """r, k, v, raw w, u(, gy) of a WKV6 problem with [*shape, C] tensors in the I/O type"""
        C = 64 * H
        d = {n: rnd(*shape, C, dtype=io) for n in ("r", "k", "v")}
        d["w"] = rnd(*shape, C, dtype=f32).mul_(1.0).sub_(1.0).to(io)
        d["u"] = rnd(H, 64, scale=0.3, dtype=io)
        if gy:
            d["gy"] = rnd(*shape, C, scale=1.0, dtype=io)
        keep.extend(d.values())
        return d

    # ---- the cases: name -> build(lib) -> (outputs {name: tensor}, [bound calls]); build is called once per side --------------------------
    cases = []
    SCAN, RAW, F32, PB, PART = _lib.ALGO_SCAN, _lib.W_RAW, _lib.IO_F32, _lib.S0_PER_BATCH, _lib.PARTIALS_F32
    iof = lambda io: F32 if io == f32 else 0

    def wkv6_dense(B, T, H, io):
        C = 64 * H
        d = problem((B, T), H, io)
        s0 = rnd(B, H, 64, 64, dtype=io)

        def build(L):
            o = {n: out(B, T, C, dtype=io) for n in ("y", "gr", "gk", "gv", "gw")}
            o["s_out"] = out(B, H, 64, 64, dtype=io)
            o["gu"], o["gs"] = out(B, C), out(B, H, 64, 64)
            ws = scratch(L.size("wkv6_backward_workspace_bytes", B, T, C, H))
            fl = RAW | iof(io) | PB | SCAN
            fwd = L.bind("wkv6_forward_ex", B, T, C, H, p(d["r"]), p(d["k"]), p(d["v"]), p(d["w"]), p(d["u"]), p(s0), p(o["s_out"]), p(o["y"]), fl, stream)
            bwd = L.bind("wkv6_backward_ex", B, T, C, H, p(d["r"]), p(d["k"]), p(d["v"]), p(d["w"]), p(d["u"]), p(s0), p(d["gy"]), p(o["gr"]), p(o["gk"]),
                         p(o["gv"]), p(o["gw"]), p(o["gu"]), p(o["gs"]), p(ws), ws.numel(), fl | PART, stream)
            return o, [fwd, bwd]
        return build

    def wkv6_bi(io):
        B, T, H = 3, 97, 1
        C = 64 * H
        d = problem((B, T), H, io)
        lens = ints([0, 33, 97])

        def build(L):
            o = {n: out(B, T, C, dtype=io) for n in ("y", "gr", "gk", "gv", "gw")}
            o["gu"] = out(B, C)
            ws = scratch(L.size("wkv6bi_workspace_bytes", B, T, C, H))
            fl = RAW | iof(io) | SCAN
            fwd = L.bind("wkv6bi_forward_ex", B, T, C, H, None, p(lens), p(d["r"]), p(d["k"]), p(d["v"]), p(d["w"]), p(d["u"]), p(o["y"]), p(ws), ws.numel(),
                         fl, stream)
            bwd = L.bind("wkv6bi_backward_ex", B, T, C, H, None, p(lens), p(d["r"]), p(d["k"]), p(d["v"]), p(d["w"]), p(d["u"]), p(d["gy"]), p(o["gr"]),
                         p(o["gk"]), p(o["gv"]), p(o["gw"]), p(o["gu"]), p(ws), ws.numel(), fl | PART, stream)
            return o, [fwd, bwd]
        return build

    def wkv6_rev(io, mask):
        B, T, H = 2, 50, 1
        C = 64 * H
        d = problem((B, T), H, io)
        rev_n = ints([0, 37])

        def build(L):
            o = {n: out(B, T, C, dtype=io) for n in ("y", "gr", "gk", "gv", "gw")}
            o["gu"] = out(B, C)
            ws = scratch(L.size("wkv6_backward_workspace_bytes", B, T, C, H))
            fl = RAW | iof(io) | SCAN
            fwd = L.bind("wkv6_forward_rev_ex", B, T, C, H, p(d["r"]), p(d["k"]), p(d["v"]), p(d["w"]), p(d["u"]), p(o["y"]), None, 0, p(rev_n), mask, fl, stream)
            bwd = L.bind("wkv6_backward_rev_ex", B, T, C, H, p(d["r"]), p(d["k"]), p(d["v"]), p(d["w"]), p(d["u"]), p(d["gy"]), p(o["gr"]), p(o["gk"]), p(o["gv"]),
                         p(o["gw"]), p(o["gu"]), p(ws), ws.numel(), p(rev_n), mask, fl | PART, stream)
            return o, [fwd, bwd]
        return build

    def wkv6_varlen(io):
        seqs, H = [1, 16, 45, 0], 2
        C, total, n = 64 * H, sum(seqs), len(seqs)
        d = problem((total,), H, io)
        cu = ints([0] + [sum(seqs[:i + 1]) for i in range(n)])

        def build(L):
            o = {m: out(total, C, dtype=io) for m in ("y", "gr", "gk", "gv", "gw")}
            o["gu"] = out(n, C)
            ws = scratch(L.size("wkv6_varlen_workspace_bytes", total, n, C, H))
            fl = RAW | iof(io) | SCAN
            fwd = L.bind("wkv6_forward_varlen_ex", total, n, max(seqs), C, H, p(cu), p(d["r"]), p(d["k"]), p(d["v"]), p(d["w"]), p(d["u"]), None, None, p(o["y"]),
                         p(ws), ws.numel(), fl, stream)
            bwd = L.bind("wkv6_backward_varlen_ex", total, n, max(seqs), C, H, p(cu), p(d["r"]), p(d["k"]), p(d["v"]), p(d["w"]), p(d["u"]), None, p(d["gy"]),
                         p(o["gr"]), p(o["gk"]), p(o["gv"]), p(o["gw"]), p(o["gu"]), None, p(ws), ws.numel(), fl | PART, stream)
            return o, [fwd, bwd]
        return build

    def decode_inputs(shape, H, io):
        """r, k, v, u in the I/O type and the fp32 decay of the stateful inference calls"""
        C = 64 * H
        d = {m: rnd(*shape, C, dtype=io) for m in ("r", "k", "v")}
        d["w"] = torch.exp(-torch.exp(rnd(*shape, C, scale=1.0) - 2.0)).contiguous()
        d["u"] = rnd(H, 64, scale=0.3, dtype=io)
        keep.append(d["w"])
        return d

    def rwkv6_dense(B, T, H, io):
        C = 64 * H
        d = decode_inputs((B, T), H, io)
        state0 = rnd(B, H, 64, 64)

        def build(L):
            o = {"y": out(B, T, C, dtype=io), "state": state0.clone()}
            keep.append(o["state"])
            run = L.bind("rwkv6_cuda_forward_" + SUFFIX[io], B, T, C, H, p(o["state"]), p(d["r"]), p(d["k"]), p(d["v"]), p(d["w"]), p(d["u"]), p(o["y"]), stream)
            return o, [run]
        return build

    def rwkv6_varlen(seqs, H, io, snap, state_slot=None, state_slot_out=None, snap_every=0, cu_snap=None, snap_slot=None, n_slots=None, flags=SCAN):
        C, total, n = 64 * H, sum(seqs), len(seqs)
        n_slots = n_slots or n
        d = decode_inputs((total,), H, io)
        cu = ints([0] + [sum(seqs[:i + 1]) for i in range(n)])
        pool0 = rnd(n_slots, H, 64, 64)
        slot, slot_out = (None if x is None else ints(x) for x in (state_slot, state_slot_out))
        cus, sns = (None if x is None else ints(x) for x in (cu_snap, snap_slot))

        def build(L):
            o = {"y": out(total, C, dtype=io), "pool": pool0.clone()}
            keep.append(o["pool"])
            ws = scratch(L.size("rwkv6_varlen_workspace_bytes", n))
            base = (total, n, max(seqs), C, H, p(cu), p(slot), n_slots, p(o["pool"]), p(d["r"]), p(d["k"]), p(d["v"]), p(d["w"]), p(d["u"]), p(o["y"]), p(ws),
                    ws.numel(), flags, stream)
            if not snap:
                return o, [L.bind("rwkv6_forward_varlen_" + SUFFIX[io], *base)]
            return o, [L.bind("rwkv6_forward_varlen_snap_" + SUFFIX[io], *base, p(slot_out), snap_every, p(cus), p(sns), 0 if snap_slot is None else len(snap_slot))]
        return build

    def wkv5(B, T, H, io):
        C = 64 * H
        d = problem((B, T), H, io)
        w = rnd(H, 64, scale=1.0).sub_(1.0).to(io)          # raw w [H,N]
        keep.append(w)

        def build(L):
            o = {m: out(B, T, C, dtype=io) for m in ("y", "gr", "gk", "gv")}
            o["gw"], o["gu"] = out(B, C), out(B, C)
            fl = RAW | iof(io)
            fwd = L.bind("wkv5_forward_ex", B, T, C, H, p(d["r"]), p(d["k"]), p(d["v"]), p(w), p(d["u"]), p(o["y"]), fl, stream)
            bwd = L.bind("wkv5_backward_ex", B, T, C, H, p(d["r"]), p(d["k"]), p(d["v"]), p(w), None, p(d["u"]), p(d["gy"]), p(o["gr"]), p(o["gk"]), p(o["gv"]),
                         p(o["gw"]), p(o["gu"]), fl | PART, stream)
            return o, [fwd, bwd]
        return build

    for io in (f32, bf):
        for T in (1, 16, 17, 33, 300):
            cases.append((f"wkv6 scan fwd+bwd {SUFFIX[io]} B2 T{T} H2 (s0, s_out, gs, gu)", wkv6_dense(2, T, 2, io)))
        cases.append((f"wkv6bi_*_ex scan {SUFFIX[io]} B3 T97 H1 lens 0,33,97", wkv6_bi(io)))
        for mask, mname in ((_lib.REV_K | _lib.REV_V | _lib.REV_Y, "K|V|Y"), (_lib.REV_ALL, "ALL")):
            cases.append((f"wkv6_*_rev_ex scan {SUFFIX[io]} B2 T50 H1 rev_n 0,37 REV_{mname}", wkv6_rev(io, mask)))
        cases.append((f"wkv6_*_varlen_ex scan {SUFFIX[io]} sequences 1,16,45,0 H2", wkv6_varlen(io)))
        for T in (1, 16, 33, 160):
            cases.append((f"wkv5 fwd+bwd {SUFFIX[io]} B2 T{T} H2 raw w", wkv5(2, T, 2, io)))
    for io in (bf, f16, f32):
        for B, T in ((4, 1), (2, 20)):
            cases.append((f"rwkv6_cuda_forward_{SUFFIX[io]} B{B} T{T} H2", rwkv6_dense(B, T, 2, io)))
        served = dict(seqs=[1, 1, 20, 130], H=2, io=io, n_slots=8, state_slot=[2, 9, 0, 1])      # slot 9: outside the pool
        cases.append((f"rwkv6_forward_varlen_{SUFFIX[io]} scan sequences 1,1,20,130, permuted slots", rwkv6_varlen(snap=False, **served)))
        cases.append((f"rwkv6_forward_varlen_snap_{SUFFIX[io]} scan, snap_every 64, separate output slots",
                      rwkv6_varlen(snap=True, state_slot_out=[3, 4, 9, 5], snap_every=64, cu_snap=[0, 0, 0, 0, 2], snap_slot=[6, 7], **served)))

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
        left = [n for n, t in sides[1].items() if t.is_floating_point() and bool(torch.isnan(t.float()).any())]
        n_out += len(diffs)
        wrong = {n: d_ for n, d_ in diffs.items() if d_}
        bad += len(wrong)
        say(f"  {'same' if not wrong else 'DIFFERENT':9s} {title}: {', '.join(diffs)}" + (f"   (NaN left in: {', '.join(left)})" if left and not a.dry else ""))
        for n, d_ in wrong.items():
            say(f"            {n}: {d_}")
    say(f"equality: {n_out - bad} of {n_out} outputs identical" + ("" if not bad else f", {bad} DIFFERENT"))
    if bad or a.no_speed:
        log.write(a.out)
        sys.exit(1 if bad else 0)

    # ---- speed -------------------------------------------------------------------------------------------------------------------------
    H = 32
    rows = []
    big = (lambda B, T: (1, 16)) if a.dry else (lambda B, T: (B, T))       # (--dry builds the rows at a toy size and stops in front of the timing)

    def each(title, build, which):
        """one row per bound call of the case (which: their names)"""
        sides = {name: build(L)[1] for name, L in (("parent", parent), ("tree", tree), ("parent-2", parent))}
        for i, w_ in enumerate(which):
            rows.append((f"{title} {w_}", {name: calls[i] for name, calls in sides.items()}))

    each("(a) wkv6 scan bf16 B8 T4096 H32", wkv6_dense(*big(8, 4096), H, bf), ("forward", "backward (S + G)"))
    each("(b) wkv6 scan fp32 B4 T2048 H32", wkv6_dense(*big(4, 2048), H, f32), ("forward", "backward (S + G)"))
    each("(c) wkv5 bf16 B8 T4096 H32", wkv5(*big(8, 4096), H, bf), ("forward", "backward (A + G)"))
    for B, T in ((64, 1), (256, 1), (8, 16)):
        each(f"(d) rwkv6_cuda_forward_bf16 B{B} T{T} H32", rwkv6_dense(B, T, H, bf), ("",))
    each("(e) rwkv6_forward_varlen_bf16 256 x 1 token", rwkv6_varlen([1] * 256, H, bf, snap=False, flags=0), ("",))
    each("(e) rwkv6_forward_varlen_snap_bf16 256 x 1 token, state_slot_out", rwkv6_varlen([1] * 256, H, bf, snap=True, flags=0, n_slots=512,
                                                                                          state_slot_out=list(range(256, 512))), ("",))

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
        ok = med["tree"] - med["parent"] <= spread
        outside += not ok
        say(f"  {title}   ({iters} calls per timing)")
        for n, xs in res.items():
            say(f"    {n:9s} " + timing.stats(xs, 9, 1))
        say(f"    tree - parent = {med['tree'] - med['parent']:+.1f} us ({100 * (med['tree'] / med['parent'] - 1):+.2f} %), "
            f"|parent-2 - parent| = {spread:.1f} us: {'inside' if ok else 'OUTSIDE'}")
    say(f"speed: {len(rows) - outside} of {len(rows)} rows inside" + ("" if not outside else f", {outside} OUTSIDE (repeat the command once before judging)"))
    log.write(a.out)


if __name__ == "__main__":
    main()
