"""Time the packed stateful inference call with long sequences cut over T (rwkv6_forward_varlen_split_bf16, seg_len in {512, 1024, 2048})
against the uncut packed call (rwkv6_forward_varlen_bf16) and against the dense operator, bf16, H=32, C=2048:

  (a) one prompt of 16384 tokens                       dense: one rwkv6_cuda_forward_bf16(B = 1) call (it cuts T itself: chunk_forward)
  (b) one prompt of 4096 tokens + 56 decode tokens     dense: 57 B = 1 calls, the only correct way to serve that batch without the packed call
  (c) 8 prompts of 512 tokens, seg_len = 512           nobody is cut: what asking costs
  (d) 8 prompts of 4096 tokens                         dense: one B = 8 call

The uncut packed call goes to --parent-lib when one is given (a librwkv6_amd.so built from the commit before the split call existed), else to
this tree's library.  Every call is made through ctypes with pre-bound arguments and a caller workspace, the same way on all sides.  Method:
tools/timing.py (--warm seconds of warm-up each, --repeats rounds in one process, --iters calls per timing, the state pool zeroed in front of
every timing); the uncut contender runs twice per round ("uncut-2").

    python tools/time_rwkv6_split.py [--parent-lib PATH] [--out profiles/rwkv6_split_time.txt]
"""
import argparse
import os
import sys

import timing
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
    log = timing.Log()
    say = log.say

    lib = _lib.load()
    parent = lib
    if a.parent_lib:
        parent = timing.load_library(a.parent_lib, {"rwkv6_forward_varlen_bf16": _lib.SIGNATURES["rwkv6_forward_varlen_bf16"]},
                                     lacks=("rwkv6_forward_varlen_split_bf16", "the split call"))
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    SEGS = (512, 1024, 2048)

    def batch(lens, segs):
        ws_bytes = max(lib.rwkv6_varlen_split_workspace_bytes(sum(lens), len(lens), s, C, H) for s in segs)
        return dict(timing.packed_batch(lens, H, g, ws_bytes), segs=segs)

    u = (torch.randn(H, 64, device="cuda", generator=g) * 0.3).to(bf)
    p = lambda t: t.data_ptr()

    def plain_args(d):
        return (d["total"], len(d["lens"]), max(d["lens"]), C, H, p(d["cu"]), None, len(d["lens"]), p(d["pool"]), p(d["r"]), p(d["k"]), p(d["v"]),
                p(d["w"]), p(u), p(d["y"]), p(d["ws"]), d["ws"].numel(), 0, stream)

    def uncut_call(d):
        return timing.bound(parent.rwkv6_forward_varlen_bf16, *plain_args(d))

    def split_call(d, seg_len):
        return timing.bound(lib.rwkv6_forward_varlen_split_bf16, *plain_args(d), None, 0, None, None, 0, seg_len)

    def dense_calls(d, rows):
        return timing.dense_calls(lib.rwkv6_cuda_forward_bf16, d, rows, H, u, stream)

    say(timing.device_header())
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

    timed = lambda fn: timing.event_time(fn, a.iters) * 1e3
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
            timing.warm(fn, seconds=a.warm)
        res = timing.alternate(contenders, timed, a.repeats, before=d["pool"].zero_)
        for n, xs in res.items():
            say(f"  {n:10s} " + timing.values_and_stats(xs, 8, 1))
        m = {n: timing.median(xs) for n, xs in res.items()}
        lo, hi = min(res["uncut"] + res["uncut-2"]), max(res["uncut"] + res["uncut-2"])
        say(f"  uncut against itself: {m['uncut-2'] / m['uncut']:.3f}, range [{lo:.1f}, {hi:.1f}]; dense / uncut = {m['dense'] / m['uncut']:.3f}")
        best = min(d["segs"], key=lambda s: m[f"split-{s}"])
        for s in d["segs"]:
            xs = res[f"split-{s}"]
            apart = "ranges do not overlap" if timing.apart(xs, (lo, hi)) else "ranges overlap"
            say(f"  split-{s} / uncut = {m[f'split-{s}'] / m['uncut']:.3f} ({apart}); split-{s} / dense = {m[f'split-{s}'] / m['dense']:.3f}")
        xs = res[f"split-{best}"]
        summary.append(f"{title}: best seg_len {best}: {m[f'split-{best}']:.1f} against uncut {m['uncut']:.1f} = "
                       f"{m[f'split-{best}'] / m['uncut']:.3f} ({'faster' if max(xs) < lo else 'slower' if min(xs) > hi else 'within the spread'}), "
                       f"dense {m['dense']:.1f}")
        say()
    for s in summary:
        say(s)
    log.write(a.out)


if __name__ == "__main__":
    main()
