"""Time the packed stateful inference call with long sequences cut over T (rwkv6_forward_varlen_split_bf16, seg_len in {512, 1024, 2048})
against the uncut packed call (rwkv6_forward_varlen_bf16) and against the dense operator, bf16, H=32, C=2048:

  (a) one prompt of 16384 tokens                       dense: one rwkv6_cuda_forward_bf16(B = 1) call (it cuts T itself: chunk_forward)
  (b) one prompt of 4096 tokens + 56 decode tokens     dense: 57 B = 1 calls, the only correct way to serve that batch without the packed call
  (c) 8 prompts of 512 tokens, seg_len = 512           nobody is cut: what asking costs
  (d) 8 prompts of 4096 tokens                         dense: one B = 8 call

The uncut packed call goes to --parent-lib when one is given (a librwkv6_amd.so built from the commit before the split call existed), else to
this tree's library.  Every call is made through ctypes with pre-bound arguments and a caller workspace, the same way on all sides.  Method of
tools/time_rwkv6_varlen.py: everything is allocated first, each contender is warmed for --warm seconds, then --repeats rounds alternate the
contenders in one process, each timing --iters back-to-back calls with device events; the uncut contender runs twice per round ("uncut-2") to
show the spread of a contender against itself.

    python tools/time_rwkv6_split.py [--parent-lib PATH] [--out profiles/rwkv6_split_time.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rwkv_lm_ext_amd import _lib          # noqa: E402

bf = torch.bfloat16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=32)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warm", type=float, default=0.5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H = a.H
    C = 64 * H
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lib = _lib.load()
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent.rwkv6_forward_varlen_bf16.restype = ctypes.c_int
        parent.rwkv6_forward_varlen_bf16.argtypes = lib.rwkv6_forward_varlen_bf16.argtypes
        assert not hasattr(parent, "rwkv6_forward_varlen_split_bf16"), "--parent-lib already has the split call: not the parent commit's library"
    else:
        parent = lib
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    keep = []                                                                # every buffer a bound call points into
    SEGS = (512, 1024, 2048)

    def batch(lens, segs):
        total = sum(lens)
        r, k, v = (torch.randn(total, C, device="cuda", generator=g).mul_(0.5).to(bf) for _ in range(3))
        w = torch.exp(-torch.exp(torch.randn(total, C, device="cuda", generator=g) - 2.0)).contiguous()
        y = torch.empty(total, C, device="cuda", dtype=bf)
        cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device="cuda")
        pool = torch.zeros(len(lens), H, 64, 64, device="cuda")
        ws = torch.empty(max(lib.rwkv6_varlen_split_workspace_bytes(total, len(lens), s, C, H) for s in segs), dtype=torch.uint8, device="cuda")
        keep.extend((r, k, v, w, y, cu, pool, ws))
        return dict(r=r, k=k, v=v, w=w, y=y, cu=cu, pool=pool, ws=ws, lens=lens, total=total, segs=segs)

    u = (torch.randn(H, 64, device="cuda", generator=g) * 0.3).to(bf)
    p = lambda t: t.data_ptr()

    def plain_args(d):
        return (d["total"], len(d["lens"]), max(d["lens"]), C, H, p(d["cu"]), None, len(d["lens"]), p(d["pool"]), p(d["r"]), p(d["k"]), p(d["v"]),
                p(d["w"]), p(u), p(d["y"]), p(d["ws"]), d["ws"].numel(), 0, stream)

    def uncut_call(d):
        args, fn = plain_args(d), parent.rwkv6_forward_varlen_bf16

        def run():
            rc = fn(*args)
            assert rc == 0, rc
        return run

    def split_call(d, seg_len):
        args = plain_args(d) + (None, 0, None, None, 0, seg_len)

        def run():
            rc = lib.rwkv6_forward_varlen_split_bf16(*args)
            assert rc == 0, rc
        return run

    def dense_calls(d, rows):
        """rows: (first token, B, T, first slot) per dense call"""
        bound = []
        for t0, B, T, slot in rows:
            el = t0 * C
            bound.append((B, T, C, H, p(d["pool"]) + slot * H * 4096 * 4, p(d["r"]) + el * 2, p(d["k"]) + el * 2, p(d["v"]) + el * 2,
                          p(d["w"]) + el * 4, p(u), p(d["y"]) + el * 2, stream))

        def run():
            for args in bound:
                rc = lib.rwkv6_cuda_forward_bf16(*args)
                assert rc == 0, rc
        return run

    prop = torch.cuda.get_device_properties(0)
    say(f"device: {prop.name}, {prop.multi_processor_count} CUs; torch {torch.__version__}; hip {torch.version.hip}")
    where = "the parent commit's library" if a.parent_lib else "this library"
    say(f"bf16, H={H}, C={C}; uncut packed call from {where}; split and dense calls from this library; "
        f"{a.iters} calls per timing, {a.repeats} alternated repeats, {a.warm:.1f} s warm-up each; times in us per call")
    say()

    one16k, mixed, short8, long8 = batch([16384], SEGS), batch([4096] + [1] * 56, SEGS), batch([512] * 8, (512,)), batch([4096] * 8, SEGS)
    starts = mixed["cu"].tolist()
    cases = {
        "(a) 1 x 16384": (one16k, [(0, 1, 16384, 0)]),
        "(b) 1 x 4096 + 56 x 1": (mixed, [(starts[s], 1, n, s) for s, n in enumerate(mixed["lens"])]),
        "(c) 8 x 512": (short8, [(0, 8, 512, 0)]),
        "(d) 8 x 4096": (long8, [(0, 8, 4096, 0)]),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters * 1e3

    summary = []
    for title, (d, rows) in cases.items():
        contenders = {"uncut": uncut_call(d), "uncut-2": uncut_call(d), "dense": dense_calls(d, rows)}
        for s in d["segs"]:
            contenders[f"split-{s}"] = split_call(d, s)
        # results first, from zero states: y of every split call against the uncut call
        d["pool"].zero_()
        contenders["uncut"]()
        want = d["y"].float()
        for s in d["segs"]:
            d["pool"].zero_()
            d["y"].zero_()
            contenders[f"split-{s}"]()
            torch.cuda.synchronize()
            err = float((d["y"].float() - want).abs().max()) / float(want.abs().max())
            say(f"{title}: split-{s} y against uncut: max |diff| / max |y| = {err:.2e}" + (" (bit-identical)" if torch.equal(d["y"].float(), want) else ""))
        for fn in contenders.values():
            t0 = time.time()
            while time.time() - t0 < a.warm:
                fn()
            torch.cuda.synchronize()
        res = {n: [] for n in contenders}
        for _ in range(a.repeats):
            for n, fn in contenders.items():
                d["pool"].zero_()
                res[n].append(timed(fn))
        for n, xs in res.items():
            say(f"  {n:10s} " + " ".join(f"{x:8.1f}" for x in xs) + f"   median {statistics.median(xs):8.1f}  min {min(xs):8.1f}  max {max(xs):8.1f}")
        m = {n: statistics.median(xs) for n, xs in res.items()}
        lo, hi = min(res["uncut"] + res["uncut-2"]), max(res["uncut"] + res["uncut-2"])
        say(f"  uncut against itself: {m['uncut-2'] / m['uncut']:.3f}, range [{lo:.1f}, {hi:.1f}]; dense / uncut = {m['dense'] / m['uncut']:.3f}")
        best = min(d["segs"], key=lambda s: m[f"split-{s}"])
        for s in d["segs"]:
            xs = res[f"split-{s}"]
            apart = "ranges do not overlap" if max(xs) < lo or min(xs) > hi else "ranges overlap"
            say(f"  split-{s} / uncut = {m[f'split-{s}'] / m['uncut']:.3f} ({apart}); split-{s} / dense = {m[f'split-{s}'] / m['dense']:.3f}")
        xs = res[f"split-{best}"]
        summary.append(f"{title}: best seg_len {best}: {m[f'split-{best}']:.1f} against uncut {m['uncut']:.1f} = "
                       f"{m[f'split-{best}'] / m['uncut']:.3f} ({'faster' if max(xs) < lo else 'slower' if min(xs) > hi else 'within the spread'}), "
                       f"dense {m['dense']:.1f}")
        say()
    for s in summary:
        say(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
