"""Time the fused low-rank time-mix inputs (mix_op.tmix_inputs + mix_op.decay_lowrank: four launches, csrc/wkv6_lowrank.hip) against the
chains they stand for in Tmix_x060.jit_func (ddlerp_slots, matmul, tanh, transpose copy + bmm, cat + ddlerp_slots; matmul, tanh, matmul,
add: eleven launches), bf16, C = 2048, D = 32, Dd = 64, on packed batches with the token-shift state in a slot pool:

  (i)   256 x 1                      a decode step of 256 sequences
  (ii)  8 x 66..512 + 56 x 1         8 prompts of 66..512 tokens + 56 decode tokens
  (iii) 8 x 1024                     8 prompts of 1024 tokens

each eagerly and replayed from a captured graph; then the graph-replayed 24-layer serving step of tools/time_packed_step.py case (i)
(infctx.step_packed, dim_ffn = 7168, 256 slots) with Tmix_x060.fuse_lowrank on against off.

Method: tools/timing.py.  One process, one box; everything is allocated first, every contender is warmed (--warm seconds, synchronised
after every call), then the contenders alternate round by round (--repeats rounds, --iters / --iters-step calls per timing between two
device events); reported is the median [min, max] over the rounds, and two contenders are called apart only when their ranges do not
overlap.  The lines "outputs" compare what the two contenders computed on the timed inputs: the share of elements whose bits differ and
the largest difference.

    python tools/time_lowrank.py [--out profiles/lowrank_time.txt]
"""
import argparse
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, H, DIM_FFN, LAYERS, N_SLOTS = 2048, 32, 7168, 24, 256
CASES = {
    "(i) 256 x 1": [1] * 256,
    "(ii) 8 x 66..512 + 56 x 1": [66 + (i * (512 - 66)) // 7 for i in range(8)] + [1] * 56,
    "(iii) 8 x 1024": [1024] * 8,
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=LAYERS)
    ap.add_argument("--iters", type=int, default=50, help="calls per timing of the two pairs")
    ap.add_argument("--iters-step", type=int, default=3, help="calls per timing of the serving step")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warm", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from rwkv_lm_ext_amd import callers, infctx, mix_op, train_dp
    bf = torch.bfloat16
    log = timing.Log()
    say = log.say
    i32 = lambda v: torch.tensor(list(v), dtype=torch.int32, device="cuda")
    torch.manual_seed(0)
    say(timing.device_header())
    say(f"bf16, C={C}, D=32, Dd=64; {a.iters} calls per timing ({a.iters_step} of the step), {a.repeats} alternated rounds in one process, "
        f"{a.warm:.1f} s warm-up each; us per call: median [min, max]")
    say("fused: mix_op.tmix_inputs + mix_op.decay_lowrank (4 launches).  today: the chains of Tmix_x060.jit_func (11 launches).")
    say()

    with torch.no_grad():
        # ---- the two pairs alone
        tm = callers.Tmix_x060(C, C).cuda()
        for n, p in tm.named_parameters():
            if n.startswith("time_maa_") and p.dim() == 3 and p.shape[0] == 1:
                torch.nn.init.uniform_(p, 0.0, 1.0)
            else:
                torch.nn.init.normal_(p, 0.0, 0.02)
        tm.time_decay.add_(-5.0)
        tm = tm.to(bf).requires_grad_(False)
        pool = torch.randn(N_SLOTS, C, device="cuda").to(bf)
        summary = []
        for case, lens in CASES.items():
            n, total = len(lens), sum(lens)
            cu = [0]
            for m in lens:
                cu.append(cu[-1] + m)
            x, cu_t, slots = torch.randn(1, total, C, device="cuda").to(bf), i32(cu), i32(range(n))
            maa_x, W1t, W2t, maa5, D1t, D2t, td = tm._lowrank_weights()

            def fused():
                out = mix_op.tmix_inputs(x, maa_x, W1t, W2t, maa5, cu_t, None, pool, slots)
                return out, mix_op.decay_lowrank(out[0], D1t, D2t, td)

            def today():
                lead = mix_op.ddlerp_slots(x, tm.time_maa_x.view(1, C), None, pool, slots, cu_t)[0]
                low = torch.tanh(lead @ tm.time_maa_w1).view(total, 5, -1).transpose(0, 1)
                corr = torch.bmm(low, tm.time_maa_w2).view(5, 1, total, C)
                out = mix_op.ddlerp_slots(x, tm._maa5(), corr, pool, slots, cu_t)
                return out, tm.time_decay + torch.tanh(out[0] @ tm.time_decay_w1) @ tm.time_decay_w2

            (fo, fw), (to, tw) = fused(), today()
            torch.cuda.synchronize()
            say(case + f"  ({total} rows)")
            for name, p, q in (("out", fo, to), ("w", fw, tw)):
                differ = float((p.view(torch.int16) != q.contiguous().view(torch.int16)).float().mean())
                say(f"  outputs {name:3s}: {differ * 100:.4f} % of the elements differ in their bits, largest |fused - today| = "
                    f"{float((p.float() - q.float()).abs().max()):.4g} (largest |today| = {float(q.float().abs().max()):.4g})")
            for mode in ("eager", "graph"):
                cont = {"fused": fused, "today": today}
                if mode == "graph":
                    cont = {k: timing.graphed(f)[0] for k, f in cont.items()}
                for f in cont.values():
                    timing.warm(f, seconds=a.warm, sync="each")
                res = timing.alternate(cont, lambda f: timing.event_time(f, a.iters) * 1e3, a.repeats)
                m = {k: timing.median(v) for k, v in res.items()}
                fmt = lambda k: f"{k} {m[k]:9.1f} [{min(res[k]):9.1f}, {max(res[k]):9.1f}]"
                apart = "ranges do not overlap" if timing.apart(res["fused"], res["today"]) else "ranges overlap"
                say(f"  {mode:5s}  {fmt('fused')}   {fmt('today')}   fused / today = {m['fused'] / m['today']:.3f} ({apart})")
                summary.append(f"{case}, the two pairs, {mode}: {m['fused']:.1f} against {m['today']:.1f} us = {m['fused'] / m['today']:.3f} ({apart})")
            say()
        del tm, pool

        # ---- the serving step, graph-replayed, the attribute on against off
        with torch.device("cuda"):
            blocks = [train_dp.Block(C, C, DIM_FFN, i) for i in range(a.layers)]
        for b in blocks:
            for p in b.parameters():
                torch.nn.init.normal_(p, 0.0, 0.02)
            b.to(bf).requires_grad_(False)
        lens = CASES["(i) 256 x 1"]
        n = len(lens)
        x, cu_t, slots = torch.randn(1, n, C, device="cuda").to(bf), i32(range(n + 1)), i32(range(n))
        pools = infctx.PackedPools(torch.zeros(a.layers, N_SLOTS, C, device="cuda", dtype=bf), torch.zeros(a.layers, N_SLOTS, C, device="cuda", dtype=bf),
                                   torch.zeros(a.layers, N_SLOTS, H, 64, 64, device="cuda"))

        def step():
            return infctx.step_packed(blocks, x, cu_t, 1, pools, slots)

        cont = {}
        for name, on in (("on", True), ("off", False)):
            for b in blocks:
                b.att.fuse_lowrank = on
            cont[name] = timing.graphed(step)[0]                  # (graphed() calls step() once before it captures: the weight copies exist)
        for f in cont.values():
            timing.warm(f, seconds=a.warm, sync="each")
        res = timing.alternate(cont, lambda f: timing.event_time(f, a.iters_step) * 1e3, a.repeats)
        m = {k: timing.median(v) for k, v in res.items()}
        fmt = lambda k: f"{k} {m[k]:9.1f} [{min(res[k]):9.1f}, {max(res[k]):9.1f}]"
        apart = "ranges do not overlap" if timing.apart(res["on"], res["off"]) else "ranges overlap"
        say(f"(i) 256 x 1, infctx.step_packed x{a.layers}, dim_ffn={DIM_FFN}, {N_SLOTS} slots, graph replay, fuse_lowrank on against off")
        say(f"  graph  {fmt('on')}   {fmt('off')}   on / off = {m['on'] / m['off']:.3f} ({apart})")
        summary.append(f"(i) 256 x 1, step x{a.layers}, graph: {m['on']:.1f} against {m['off']:.1f} us = {m['on'] / m['off']:.3f} ({apart})")
        say()
    for s in summary:
        say(s)
    say("not measured: other C, a second box, HBM traffic")
    log.write(a.out)


if __name__ == "__main__":
    main()
