"""Time the packed stateful inference call (rwkv6_forward_varlen_bf16) against what serves the same batch without it, bf16, H=32, C=2048:

  (a) mixed batch     8 prompts of 66..512 tokens + 56 decode sequences of 1 token: one packed call against the only correct way to serve
                      that batch with the dense operator, 64 rwkv6_cuda_forward_bf16(B = 1) calls (padding a stateful operator is wrong)
  (b) uniform decode  256 sequences of 1 token, identity slots: packed against the dense B = 256, T = 1 call
  (c) uniform prefill 8 sequences of 512 tokens: packed against the dense B = 8, T = 512 call

The dense calls go to --parent-lib when one is given (a librwkv6_amd.so built from the commit before the packed call existed), else to this
tree's library.  Every call is made through ctypes with pre-bound arguments, the same way on both sides, so that the host cost per call is
the same few microseconds.  Method: tools/timing.py (--warm seconds of warm-up each, --repeats rounds in one process, --iters calls per
timing); the dense contender runs twice per round ("dense-2").

    python tools/time_rwkv6_varlen.py [--parent-lib PATH] [--out profiles/rwkv6_varlen_time.txt]
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
    ap.add_argument("--iters", type=int, default=50)
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
        parent = timing.load_library(a.parent_lib, {"rwkv6_cuda_forward_bf16": _lib.SIGNATURES["rwkv6_cuda_forward_bf16"]},
                                     lacks=("rwkv6_forward_varlen_bf16", "the packed call"))
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)

    def batch(lens):
        return timing.packed_batch(lens, H, g, lib.rwkv6_varlen_workspace_bytes(len(lens)))

    u = (torch.randn(H, 64, device="cuda", generator=g) * 0.3).to(bf)
    p = lambda t: t.data_ptr()

    def packed_call(d):
        return timing.bound(lib.rwkv6_forward_varlen_bf16, d["total"], len(d["lens"]), max(d["lens"]), C, H, p(d["cu"]), None, len(d["lens"]),
                            p(d["pool"]), p(d["r"]), p(d["k"]), p(d["v"]), p(d["w"]), p(u), p(d["y"]), p(d["ws"]), d["ws"].numel(), 0, stream)

    def dense_calls(d, rows):
        return timing.dense_calls(parent.rwkv6_cuda_forward_bf16, d, rows, H, u, stream)

    say(timing.device_header())
    where = "the parent commit's library" if a.parent_lib else "this library"
    say(f"bf16, H={H}, C={C}; dense calls from {where}; "
        f"{a.iters} calls per timing, {a.repeats} alternated repeats, {a.warm:.1f} s warm-up each")
    say()

    prompts = [66 + round(i * (512 - 66) / 7) for i in range(8)]
    mixed = batch(prompts + [1] * 56)
    starts = mixed["cu"].tolist()
    decode, prefill = batch([1] * 256), batch([512] * 8)
    cases = {
        "(a) mixed 8 x 66..512 + 56 x 1": (mixed, [(starts[s], 1, n, s) for s, n in enumerate(mixed["lens"])]),
        "(b) decode 256 x 1": (decode, [(0, 256, 1, 0)]),
        "(c) prefill 8 x 512": (prefill, [(0, 8, 512, 0)]),
    }

    timed = lambda fn: timing.event_time(fn, a.iters) * 1e3                 # us per call (or per loop of dense calls)
    med = {}
    for title, (d, rows) in cases.items():
        contenders = {"packed": packed_call(d), "dense": dense_calls(d, rows), "dense-2": dense_calls(d, rows)}
        # same results first: y and the pool, bit for bit (from zero states)
        d["pool"].zero_()
        contenders["dense"]()
        want = (d["y"].clone(), d["pool"].clone())
        d["pool"].zero_()
        d["y"].zero_()
        contenders["packed"]()
        torch.cuda.synchronize()
        say(f"{title}: packed y and states == dense, bit for bit: {bool(torch.equal(d['y'], want[0]) and torch.equal(d['pool'], want[1]))}")
        for fn in contenders.values():
            timing.warm(fn, seconds=a.warm)
        res = timing.alternate(contenders, timed, a.repeats)
        for n, xs in res.items():
            say(f"  {n:8s} us: " + timing.values_and_stats(xs, 8, 1))
        m = {n: timing.median(xs) for n, xs in res.items()}
        med[title] = m
        lo, hi = min(res["dense"] + res["dense-2"]), max(res["dense"] + res["dense-2"])
        say(f"  packed / dense = {m['packed'] / m['dense']:.3f} ({m['packed'] - m['dense']:+.1f} us, {100 * (m['packed'] / m['dense'] - 1):+.1f} %); "
            f"dense against itself: {m['dense-2'] / m['dense']:.3f}, range [{lo:.1f}, {hi:.1f}] us; "
            f"{'ranges do not overlap' if timing.apart(res['packed'], (lo, hi)) else 'ranges overlap'}")
        say()
    ta, tb, tc = (med[t] for t in cases)
    say(f"(a) one packed call is {ta['dense'] / ta['packed']:.2f}x the speed of the loop of 64 dense B = 1 calls"
        f" -> {'packed is faster' if ta['packed'] < ta['dense'] else 'PACKED IS NOT FASTER: the routing is wrong'}")
    say(f"(b) overhead of the packed decode step: {tb['packed'] - tb['dense']:+.1f} us over the dense call (one preparation launch more; 2-4 us "
        f"for that launch alone in profiles/varlen_time.txt)")
    say(f"(c) packed prefill against dense: {100 * (tc['packed'] / tc['dense'] - 1):+.1f} % (the packed training forward: +2.9 %; here the packed call "
        f"has a preparation launch and a scan launch, whose workgroups all leave at once, beside the chunked one)")
    log.write(a.out)


if __name__ == "__main__":
    main()
