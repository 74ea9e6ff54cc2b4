"""Time the beam-search candidate kernels (mix_op.beam_candidates: rwkv6_beam_candidates_bf16, csrc/wkv6_beam.hip) against the eager
restatement (infctx._beam_candidates_eager: fp64 log_softmax, top-k per row and per group with the ties cut), in one process.

Candidate call: bf16 logits [n_rows, 65536], n_rows = 10 and 80 (1 and 8 requests of W = 10 beams, every row live), K = 30, without and
with the repetition penalty (an occurrence pool with 1 % of its entries set), called eagerly and replayed from a captured graph.
`eager-2` is the eager code a second time in every round: the spread of a contender against itself.

Whole step: one graph-replayed infctx.beam_step_packed -- emb, 24 blocks (C = 2048, H = 32, dim_ffn = 7168, the model of
tools/time_packed_step.py), ln_out, a head of 65536, candidates, bookkeeping -- for 8 requests of W = 10, two eos ids (K = 30), with the
penalty; kernels=True against kernels=False, each on a search state and pools of its own.

Method: tools/timing.py (warm-up calls of every contender, --repeats alternated rounds, --iters calls per timing; median [min, max]).  Two
contenders are called apart only when their ranges do not overlap.  The last line states the dispatch rule the figures give.

    python tools/time_beam.py [--out profiles/beam_time.txt]
"""
import argparse
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
V, W, K = 65536, 10, 30
C, H, DIM_FFN, LAYERS = 2048, 32, 7168, 24


def fmt(us):
    return f"{timing.median(us):9.1f} us [{min(us):9.1f}, {max(us):9.1f}]"


def verdict(times, say):
    """kernels against eager: the ratio of the medians, whether the ranges are apart; True where the kernels are not slower"""
    k, e = times["kernels"], times["eager"]
    apart = timing.apart(k, e)
    say(f"    eager / kernels = {timing.median(e) / timing.median(k):.2f}x ({'ranges do not overlap' if apart else 'RANGES OVERLAP'})")
    return timing.median(k) <= timing.median(e) or not apart


def candidate_calls(n_groups, penalised, iters, repeats, say):
    import torch
    from rwkv_lm_ext_amd import infctx
    n_rows = n_groups * W
    gen = torch.Generator(device="cuda").manual_seed(n_rows + penalised)
    logits = (torch.randn(n_rows, V, device="cuda", generator=gen) * 2).bfloat16()
    cum = -torch.rand(n_rows, device="cuda", generator=gen) * 20
    cu = torch.arange(0, n_rows + 1, W, dtype=torch.int32, device="cuda")
    kw = {}
    if penalised:
        pool = infctx.SamplingPool.create(n_rows, V, "cuda")
        pool.occ.copy_((torch.rand(n_rows, V, device="cuda", generator=gen) < 0.01).float() * 1.5)
        kw = dict(pool=pool, slots=torch.randperm(n_rows, device="cuda", generator=gen).int(), penalty=torch.full((n_groups,), 1.3, device="cuda"))

    def run(kernels):
        return lambda: infctx.beam_candidates(logits, cum, cu, K, kernels=kernels, **kw)

    with torch.no_grad():
        a, b = run(True)(), run(False)()
        same = (a[0] == b[0]) & (a[1] == b[1])
        say(f"  {n_groups} x {W} rows, {'penalty 1.3' if penalised else 'no penalty'}: {int(same.sum())} of {same.numel()} candidates equal those of "
            f"the eager code, largest score difference {float((a[2] - b[2]).abs().max()):.2e}")
        ok = True
        for graph in (False, True):
            fns = {"kernels": run(True), "eager": run(False), "eager-2": run(False)}
            if graph:
                fns = {name: timing.graphed(fn)[0] for name, fn in fns.items()}
            for fn in fns.values():
                timing.warm(fn, calls=5)
            times = timing.alternate(fns, lambda fn: timing.event_time(fn, iters) * 1e3, repeats)
            for name, us in times.items():
                say(f"    {'graph' if graph else 'eager'} call  {name:8s} {fmt(us)}")
            ok &= verdict(times, say)
    return ok


def whole_step(n_groups, iters, repeats, say):
    import torch
    from rwkv_lm_ext_amd import infctx, train_dp
    bf = torch.bfloat16
    torch.manual_seed(0)
    with torch.device("cuda"):
        blocks = [train_dp.Block(C, C, DIM_FFN, i) for i in range(LAYERS)]
        emb, ln_out, head = torch.nn.Embedding(V, C), torch.nn.LayerNorm(C), torch.nn.Linear(C, V, bias=False)
    for m in blocks + [emb, head]:
        for p in m.parameters():
            torch.nn.init.normal_(p, 0.0, 0.02)
    for m in blocks + [emb, ln_out, head]:
        m.to(bf).requires_grad_(False)
    n_slots = n_groups + 2 * W * n_groups

    def side(kernels):
        pools = infctx.PackedPools.create(LAYERS, n_slots, C, H, "cuda", bf)
        spool = infctx.SamplingPool.create(n_slots, V, "cuda")
        st = infctx.BeamSearch.create(n_groups, W, 64, (0, 1), 0.5, 1.3, list(range(5, 5 + n_groups)), list(range(n_groups)), n_groups, "cuda")
        assert st.K == K
        fn = lambda: infctx.beam_step_packed(emb, blocks, ln_out, head, st, pools, sampling_pool=spool, pool_kernels=True, kernels=kernels)
        return timing.graphed(fn)[0], st

    with torch.no_grad():
        sides = {"kernels": side(True), "eager": side(False), "eager-2": side(False)}
        fns = {name: s[0] for name, s in sides.items()}
        for fn in fns.values():
            timing.warm(fn, calls=3)
        times = timing.alternate(fns, lambda fn: timing.event_time(fn, iters) * 1e3, repeats)
    say(f"  graph-replayed beam_step_packed, {LAYERS} layers, C = {C}, head {V}, {n_groups} x {W} rows, K = {K}, penalty 1.3")
    for name, us in times.items():
        live = int((sides[name][1].cum > float("-inf")).sum())
        say(f"    {name:8s} {fmt(us)}   ({live} of {n_groups * W} rows live after {int(sides[name][1].step)} steps)")
    return verdict(times, say)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="the candidate calls only")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "no GPU: nothing is measured on a CPU"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    log = timing.Log()
    say = log.say
    say(f"# tools/time_beam.py; {timing.device_header()}; one box, one run")
    say(f"# {args.repeats} alternated rounds of {args.iters} calls each (the whole step: {max(1, args.iters // 4)}), device events; median [min, max]")
    say(f"candidate call: bf16 logits [n_rows, {V}], K = {K}")
    wins = {}
    for n_groups in (1, 8):
        for penalised in (False, True):
            wins[(n_groups * W, penalised)] = candidate_calls(n_groups, penalised, args.iters, args.repeats, say)
    if not args.no_step:
        say("whole step")
        wins["step"] = whole_step(8, max(1, args.iters // 4), args.repeats, say)
    lost = [k for k, w in wins.items() if not w]
    say("dispatch: the kernels are not slower than the eager code at any size measured: kernels=None takes them wherever they apply" if not lost
        else f"dispatch: the kernels are slower than the eager code at {lost}")
    log.write(args.out and os.path.join(ROOT, args.out))


if __name__ == "__main__":
    main()
