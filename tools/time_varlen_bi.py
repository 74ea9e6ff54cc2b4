"""Time the operator calls of bidirectional composition C (two problems: the forward-direction call and the call on the reversed
stream's own projections under rev_mask = ALL) on a ragged batch, H=32, C=2048, 48 sequences by default:

  (a) packed-pair       forward_varlen_pair_ex / backward_varlen_pair_ex on 48 sequences with lengths drawn as bench.py's ragged config
                        draws them (randint(64, 513), seed 1), packed into [total_T, C]; rev_n = every sequence's length
  (b) packed-two-calls  the same as the plain packed call + forward_varlen_rev_ex (and their backwards)
  (c) dense-pair        forward_pair_ex / backward_pair_ex (WKV_6_PAIR's calls) on the same rows padded to [48, 512, C]
  (d) packed-pair-full  the packed pair on 48 full rows of 512 against
  (e) dense-pair-full   the dense pair on the same tensor viewed as [48, 512, C]

All keep their checkpoints from the forward to the backward.  Method: tools/timing.py (--warm seconds of warm-up each, --repeats
rounds, --iters calls per timing of the forward, the backward and the step).

    python tools/time_varlen_bi.py [--out profiles/varlen_bi_time.txt]
"""
import argparse
import os
import sys

import timing
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rwkv_lm_ext_amd import wkv6_op as op          # noqa: E402

bf = torch.bfloat16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=48)
    ap.add_argument("--T", type=int, default=512)
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
    ramp = torch.tensor([-6 + 5 * (n / (C - 1)) ** (0.7 + 1.3 * 0.5) for n in range(C)], device="cuda")
    u = rnd(H, 64, scale=0.3)

    def problem():      # dense tensors [B,T,C]: r, k, v, w, gy
        r, k, v = (rnd(B, T, C, scale=0.5) for _ in range(3))
        w = (ramp.view(1, 1, C) + 0.1 * torch.randn(B, T, C, generator=g, device="cuda")).to(bf)
        return [r, k, v, w, rnd(B, T, C)]

    dense = [problem(), problem()]
    lens = torch.randint(64, 513, (B,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).clamp(max=T)
    cu_r = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), lens.cumsum(0)]).to(torch.int32)
    total_r = int(cu_r[-1])
    keep = (torch.arange(T, device="cuda").view(1, T) < lens.view(B, 1))
    ragged = [[t[keep].contiguous() for t in p] for p in dense]                      # [total_r, C]
    full = [[t.view(B * T, C) for t in p] for p in dense]
    cu_f = (torch.arange(B + 1, device="cuda") * T).to(torch.int32)
    rev_r = lens.to(torch.int32).contiguous()
    rev_f = torch.full((B,), T, dtype=torch.int32, device="cuda")

    def sets_of(p, ckpts, rev_n):
        return [dict(r=p[0][0], k=p[0][1], v=p[0][2], w=p[0][3], gy=p[0][4], ckpt=ckpts[0], y=torch.empty_like(p[0][0])),
                dict(r=p[1][0], k=p[1][1], v=p[1][2], w=p[1][3], gy=p[1][4], ckpt=ckpts[1], y=torch.empty_like(p[1][0]), rev_n=rev_n,
                     rev_mask=op.REV_ALL)]

    def packed_pair(p, cu, total, rev_n):
        s = sets_of(p, [op.new_varlen_workspace(total, B, C, H, "cuda") for _ in range(2)], rev_n)
        return (lambda: op.forward_varlen_pair_ex(H, u, s, cu, T), lambda: op.backward_varlen_pair_ex(H, u, s, cu, T))

    def packed_two(p, cu, total, rev_n):
        ws = [op.new_varlen_workspace(total, B, C, H, "cuda") for _ in range(2)]
        p0, p1 = p

        def fwd():
            op.forward_varlen_ex(p0[0], p0[1], p0[2], p0[3], u, H, cu, T, ws=ws[0])
            op.forward_varlen_rev_ex(p1[0], p1[1], p1[2], p1[3], u, H, cu, T, rev_n, op.REV_ALL, ws=ws[1])

        def bwd():
            op.backward_varlen_ex(p0[0], p0[1], p0[2], p0[3], u, p0[4], H, cu, T, ws=ws[0], ckpt_valid=True)
            op.backward_varlen_rev_ex(p1[0], p1[1], p1[2], p1[3], u, p1[4], H, cu, T, rev_n, op.REV_ALL, ws=ws[1], ckpt_valid=True)
        return fwd, bwd

    def dense_pair(rev_n):
        s = sets_of(dense, [op.new_checkpoint(B, T, C, H, "cuda") for _ in range(2)], rev_n)
        return (lambda: op.forward_pair_ex(H, u, s), lambda: op.backward_pair_ex(H, u, s))

    contenders = {"(a) packed-pair": packed_pair(ragged, cu_r, total_r, rev_r), "(b) packed-two-calls": packed_two(ragged, cu_r, total_r, rev_r),
                  "(c) dense-pair": dense_pair(rev_r), "(d) packed-pair-full": packed_pair(full, cu_f, B * T, rev_f),
                  "(e) dense-pair-full": dense_pair(rev_f)}

    groups = int(((lens + 63) // 64).sum())
    say(timing.device_header())
    say(f"shape: 2 problems x {B} sequences, T={T}, C={C}, H={H}; ragged lengths {int(lens.min())}..{int(lens.max())}, total {total_r} of "
        f"{B * T} tokens ({100.0 * total_r / (B * T):.1f} % fill); 64-token groups: {groups} ragged vs {B * ((T + 63) // 64)} padded")
    say(f"{a.iters} calls per timing, {a.repeats} alternated repeats, {a.warm:.1f} s warm-up each")
    say()
    yd = contenders["(e) dense-pair-full"][0]()
    yp = contenders["(d) packed-pair-full"][0]()
    say(f"packed-pair-full y == dense-pair y bit for bit: {all(bool(torch.equal(p.view(B, T, C), d)) for p, d in zip(yp, yd))}")

    for fwd, bwd in contenders.values():
        timing.warm(lambda: (fwd(), bwd()), seconds=a.warm)
    rounds = timing.alternate(contenders, lambda pair: timing.phase_times(*pair, a.iters), a.repeats)
    res = {name: dict(zip(("fwd", "bwd", "step"), zip(*rows))) for name, rows in rounds.items()}
    for name, d in res.items():
        for ph, xs in d.items():
            say(f"{name:22s} {ph:4s} ms: " + timing.values_and_stats(xs, 7, 3))
    say()
    med = lambda n, ph: timing.median(res[n][ph])
    A, Bn, Cn, D, E = list(contenders)
    for ph in ("fwd", "bwd", "step"):
        say(f"ragged {ph}: (a) packed pair {med(A, ph):.3f} ms, (b) two calls {med(Bn, ph):.3f} ms, (c) dense pair padded {med(Cn, ph):.3f} ms: "
            f"(a)/(c) {med(A, ph) / med(Cn, ph):.3f} (forecast from group counts {groups / (B * ((T + 63) // 64)):.3f}), "
            f"(a)/(b) {med(A, ph) / med(Bn, ph):.3f}")
    for ph in ("fwd", "bwd", "step"):
        say(f"full {ph}: (d) packed pair {med(D, ph):.3f} ms [{min(res[D][ph]):.3f}, {max(res[D][ph]):.3f}] vs (e) dense pair {med(E, ph):.3f} ms "
            f"[{min(res[E][ph]):.3f}, {max(res[E][ph]):.3f}]: {100.0 * (med(D, ph) / med(E, ph) - 1.0):+.1f} %")
    log.write(a.out)


if __name__ == "__main__":
    main()
