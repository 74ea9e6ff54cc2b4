"""Time the WKV5 operator against the two ways the library could already do its job (B=8, T=4096, C=2048, H=32 by default):

  (a) wkv5       the static-decay kernels (csrc/wkv5_scan.hip): WKV_5's forward and backward calls
  (b) wkv6-scan  w expanded to [B,T,C], the exact WKV6 scan kernels (WKV6_ALGO_SCAN), gw summed over batch and time
  (c) wkv6-chunk the same composition on the chunked MFMA kernels (the library's default WKV6 path, checkpoints kept)

Each contender's forward, backward and step (forward + backward) are timed.  Method: tools/timing.py (--warm seconds of warm-up each,
--repeats rounds, --iters calls per timing of each phase).  Also printed: the bf16 report of each contender's gw [H,N] against the WKV6 scan kernels in
fp32 I/O reduced in fp64 (oracle/contract.py: bf16_report_torch, floor 0.1).

    python tools/time_wkv5.py [--out profiles/wkv5_time.txt]
"""
import argparse
import os
import sys

import timing
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.contract import bf16_report_torch      # noqa: E402
from rwkv_lm_ext_amd import wkv6_op as op          # noqa: E402

bf = torch.bfloat16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=4096)
    ap.add_argument("--H", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warm", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, T, H = a.B, a.T, a.H
    C = 64 * H
    log = timing.Log()
    say = log.say

    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g, device="cuda") * scale).to(bf)
    r, k, v = (rnd(B, T, C, scale=0.5) for _ in range(3))
    gy = rnd(B, T, C)
    u = rnd(H, 64, scale=0.3)
    n = torch.arange(C, dtype=torch.float32, device="cuda")
    w = (-6 + 5 * (n / (C - 1)) ** 0.7).view(H, 64).to(bf)          # the model's initial decay ramp (src/model.py:318-321)
    hn = (H, 64)
    ckpt = op.new_checkpoint(B, T, C, H, r.device)
    state = {}

    def a_fwd():
        return op.wkv5_forward_ex(r, k, v, w, u, H)

    def a_bwd():
        gr, gk, gv, gw, gu = op.wkv5_backward_ex(r, k, v, w, u, gy, H)
        return gr, gk, gv, gw.sum(0).to(bf).view(hn), gu.sum(0).to(bf).view(hn)

    def w6_fwd(algo):
        state["wb"] = w.view(1, 1, C).expand(B, T, C).contiguous()
        return op.forward_ex(r, k, v, state["wb"], u, H, algo=algo, ckpt=None if algo else ckpt)

    def w6_bwd(algo):
        gr, gk, gv, gw, gu, _ = op.backward_ex(r, k, v, state["wb"], u, gy, H, algo=algo, ckpt=None if algo else ckpt)
        return gr, gk, gv, gw.float().sum((0, 1)).to(bf).view(hn), gu.sum(0).to(bf).view(hn)

    contenders = {"(a) wkv5": (a_fwd, a_bwd), "(b) wkv6-scan": (lambda: w6_fwd("scan"), lambda: w6_bwd("scan")),
                  "(c) wkv6-chunk": (lambda: w6_fwd(None), lambda: w6_bwd(None))}

    say(timing.device_header())
    say(f"shape: B={B} T={T} C={C} H={H}; {a.iters} calls per timing, {a.repeats} alternated repeats, {a.warm:.1f} s warm-up each")
    say("bytes per token-channel: wkv5 fwd 8 (r,k,v in; y out), bwd 14 (r,k,v,gy in; gr,gk,gv out); wkv6 fwd 10, bwd 18")
    say()

    # ---- gw / gu [H,N] of every contender against the fp32 scan path reduced in fp64
    f = [t.float() for t in (r, k, v)]
    wb32 = w.float().view(1, 1, C).expand(B, T, C).contiguous()
    g32 = op.backward_ex(f[0], f[1], f[2], wb32, u.float(), gy.float(), H, algo="scan")
    gw_ref, gu_ref = g32[3].double().sum((0, 1)), g32[4].double().sum(0)
    del f, wb32, g32
    for name, (fwd, bwd) in contenders.items():
        fwd()
        out = bwd()
        rms, off, ulps = bf16_report_torch(out[3].view(-1), gw_ref.view(-1), 0.1)
        rms_u, off_u, ulps_u = bf16_report_torch(out[4].view(-1), gu_ref.view(-1), 1e-3)
        say(f"{name:15s} gw [H,N] bf16_report: rel-rms {rms:.2e}, {off * 100:.1f}% not correctly rounded, max {ulps:.2f} ulp"
            f"   | gu: rel-rms {rms_u:.2e}, {off_u * 100:.1f}%, max {ulps_u:.2f} ulp")
    say()

    for fwd, bwd in contenders.values():
        timing.warm(lambda: (fwd(), bwd()), seconds=a.warm)
    rounds = timing.alternate(contenders, lambda pair: timing.phase_times(*pair, a.iters), a.repeats)
    res = {name: dict(zip(("fwd", "bwd", "step"), zip(*rows))) for name, rows in rounds.items()}
    tc = B * T * C
    for name, d in res.items():
        for ph, xs in d.items():
            say(f"{name:15s} {ph:4s} ms: " + timing.values_and_stats(xs, 7, 3))
    say()
    for name, d in res.items():
        mf, mb, ms = (timing.median(d[ph]) for ph in ("fwd", "bwd", "step"))
        say(f"{name:15s} median: fwd {tc * 8 / mf / 1e9:6.3f} TB/s of 8 B/token-channel, bwd {tc * 14 / mb / 1e9:6.3f} TB/s of 14 B, "
            f"step {B * T / ms / 1e3:8.2f} Mtok/s")
    ra, rb = res["(a) wkv5"], res["(b) wkv6-scan"]
    for ph in ("fwd", "bwd", "step"):
        say(f"acceptance {ph}: (a) median {timing.median(ra[ph]):.3f} ms [{min(ra[ph]):.3f}, {max(ra[ph]):.3f}] vs "
            f"(b) median {timing.median(rb[ph]):.3f} ms [{min(rb[ph]):.3f}, {max(rb[ph]):.3f}] -> "
            f"{'(a) not slower' if timing.median(ra[ph]) <= max(rb[ph]) else '(a) SLOWER'}")
    log.write(a.out)


if __name__ == "__main__":
    main()
