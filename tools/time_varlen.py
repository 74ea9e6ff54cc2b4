"""Time the packed variable-length WKV6 operator against what a user runs today (H=32, C=2048, 48 sequences by default):

  (a) packed-ragged   forward_varlen_ex / backward_varlen_ex on 48 sequences with lengths drawn as bench.py's ragged config draws them
                      (randint(64, 513), seed 1), packed into [total_T, C]
  (b) dense-padded    forward_ex / backward_ex (WKV_6's calls) on the same rows padded to [48, 512, C]: every padded token is scanned
  (c) packed-full     the packed op on 48 full rows of 512  -- the no-padding case, where packing must cost nothing --
  (d) dense-full      the dense op on the same tensor viewed as [48, 512, C]
  (e) dense-full-2    (d) again, as a contender of its own: the spread the dense op shows against itself in this run

All keep their checkpoints from the forward to the backward, as the autograd functions do.  Method: tools/timing.py (--warm seconds
of warm-up each, --repeats rounds, --iters calls per timing of the forward, the backward and the step).

    python tools/time_varlen.py [--out profiles/varlen_time.txt]
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
    # dense tensors [B,T,C]; the full packed batch is the same memory viewed as [B*T, C]
    r, k, v = (rnd(B, T, C, scale=0.5) for _ in range(3))
    w = (ramp.view(1, 1, C) + 0.1 * torch.randn(B, T, C, generator=g, device="cuda")).to(bf)
    gy = rnd(B, T, C)
    lens = torch.randint(64, 513, (B,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).clamp(max=T)
    cu_r = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), lens.cumsum(0)]).to(torch.int32)
    total_r = int(cu_r[-1])
    keep = (torch.arange(T, device="cuda").view(1, T) < lens.view(B, 1))
    pr, pk, pv, pw, pgy = (t[keep].contiguous() for t in (r, k, v, w, gy))          # the ragged rows packed: [total_r, C]
    assert pr.shape == (total_r, C)
    cu_f = (torch.arange(B + 1, device="cuda") * T).to(torch.int32)
    fr, fk, fv, fw, fgy = (t.view(B * T, C) for t in (r, k, v, w, gy))
    ws_r = op.new_varlen_workspace(total_r, B, C, H, "cuda")
    ws_f = op.new_varlen_workspace(B * T, B, C, H, "cuda")
    ckpts = [op.new_checkpoint(B, T, C, H, "cuda") for _ in range(3)]

    def packed(tensors, cu, ws):
        x = tensors
        return (lambda: op.forward_varlen_ex(x[0], x[1], x[2], x[3], u, H, cu, T, ws=ws),
                lambda: op.backward_varlen_ex(x[0], x[1], x[2], x[3], u, x[4], H, cu, T, ws=ws, ckpt_valid=True))

    def dense(ckpt):
        return (lambda: op.forward_ex(r, k, v, w, u, H, ckpt=ckpt), lambda: op.backward_ex(r, k, v, w, u, gy, H, ckpt=ckpt))

    contenders = {"(a) packed-ragged": packed((pr, pk, pv, pw, pgy), cu_r, ws_r), "(b) dense-padded": dense(ckpts[0]),
                  "(c) packed-full": packed((fr, fk, fv, fw, fgy), cu_f, ws_f), "(d) dense-full": dense(ckpts[1]),
                  "(e) dense-full-2": dense(ckpts[2])}

    prop = torch.cuda.get_device_properties(0)
    say(timing.device_header())
    say(f"shape: {B} sequences, T={T}, C={C}, H={H}; ragged lengths {int(lens.min())}..{int(lens.max())}, total {total_r} of {B * T} tokens "
        f"({100.0 * total_r / (B * T):.1f} % fill); 64-token groups: {int(((lens + 63) // 64).sum())} ragged vs {B * ((T + 63) // 64)} padded")
    say(f"{a.iters} calls per timing, {a.repeats} alternated repeats, {a.warm:.1f} s warm-up each")
    say()

    # the packed results are the dense ones, bit for bit (full rows: the whole tensor; ragged: every row's own tokens)
    yd = op.forward_ex(r, k, v, w, u, H)
    yf = op.forward_varlen_ex(fr, fk, fv, fw, u, H, cu_f, T)
    say(f"packed-full y == dense y bit for bit: {bool(torch.equal(yf.view(B, T, C), yd))}")
    del yd, yf

    for fwd, bwd in contenders.values():
        timing.warm(lambda: (fwd(), bwd()), seconds=a.warm)
    rounds = timing.alternate(contenders, lambda pair: timing.phase_times(*pair, a.iters), a.repeats)
    res = {name: dict(zip(("fwd", "bwd", "step"), zip(*rows))) for name, rows in rounds.items()}
    for name, d in res.items():
        for ph, xs in d.items():
            say(f"{name:18s} {ph:4s} ms: " + timing.values_and_stats(xs, 7, 3))
    say()
    med = lambda n, ph: timing.median(res[n][ph])
    A, Bn, Cn, D, E = list(contenders)
    for ph in ("fwd", "bwd", "step"):
        say(f"ragged {ph}: (a) packed {med(A, ph):.3f} ms [{min(res[A][ph]):.3f}, {max(res[A][ph]):.3f}] vs (b) padded {med(Bn, ph):.3f} ms "
            f"[{min(res[Bn][ph]):.3f}, {max(res[Bn][ph]):.3f}]: ratio {med(A, ph) / med(Bn, ph):.3f} (forecast from group counts "
            f"{float(((lens + 63) // 64).sum()) / (B * ((T + 63) // 64)):.3f}) -> "
            f"{'ranges do not overlap, (a) faster' if max(res[A][ph]) < min(res[Bn][ph]) else 'RANGES OVERLAP or (a) slower'}")
    for ph in ("fwd", "bwd", "step"):
        lo = min(min(res[D][ph]), min(res[E][ph]))
        hi = max(max(res[D][ph]), max(res[E][ph]))
        diff = med(Cn, ph) - med(D, ph)
        say(f"full {ph}: (c) packed {med(Cn, ph):.3f} ms [{min(res[Cn][ph]):.3f}, {max(res[Cn][ph]):.3f}] vs dense (d) {med(D, ph):.3f} / (e) "
            f"{med(E, ph):.3f} ms, dense-vs-dense range [{lo:.3f}, {hi:.3f}] -> "
            f"{'(c) within the dense range' if lo <= med(Cn, ph) <= hi or med(Cn, ph) <= hi else '(c) OUTSIDE the dense range'}"
            f"; difference {diff * 1e3:+.1f} us = {diff * 1e6 / (B * H / prop.multi_processor_count):+.0f} ns per row of a CU "
            f"({B * H / prop.multi_processor_count:.1f} rows per CU)")
    log.write(a.out)


if __name__ == "__main__":
    main()
