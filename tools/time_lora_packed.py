"""Time the serving step (infctx.step_packed, 24 layers, bf16, C = 2048, H = 32, dim_ffn = 7168, 256 slots) with per-sequence LoRA adapters
(adapters.inject_adapters, r = 8 on the six targets; csrc/wkv6_lora.hip) on

  (i)  256 decode tokens over 1, 3 and 16 adapters (sequence s on adapter s mod n: every tile of 16 rows holds min(16, n) adapters)
  (ii) 8 prompts of 66..512 tokens + 56 decode tokens over 3 adapters

against three baselines, eagerly and replayed from a captured graph:

  plain    the same step with no adapter (blocks that were never injected): what the adapters add
  masked   the same injected blocks with kernels=False: the eager masked loop, one pass over all rows per adapter
  groups   what serves such a batch without this feature: one step_packed per adapter group over that group's rows, the blocks under
           train_dp.inject_lora (one adapter; the groups reuse its weights, which does not change the time).  --parent-tree PATH names a
           checkout of the parent commit with its own built library, imported in a process of its own; without it the same code runs
           from this tree and the output says so.

Method: tools/timing.py, one child process per contender (--warm seconds of warm-up each, synchronised after every call; --repeats rounds;
--iters calls per timing); reported is the median [min, max] over the rounds.  The accuracy lines are mix_op.lora_packed on the inputs of
tests/test_lora_packed_gpu.py against the fp64 restatement of tests/lora_common.py.

    python tools/time_lora_packed.py [--parent-tree PATH] [--out profiles/lora_packed_time.txt]
"""
import argparse
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, H, DIM_FFN, LAYERS, N_SLOTS, RANK = 2048, 32, 7168, 24, 256, 8
PROMPTS = [66 + (i * (512 - 66)) // 7 for i in range(8)]
CASES = {
    "(i) 256 x 1, 1 adapter": dict(lens=[1] * 256, n_adapters=1),
    "(i) 256 x 1, 3 adapters": dict(lens=[1] * 256, n_adapters=3),
    "(i) 256 x 1, 16 adapters": dict(lens=[1] * 256, n_adapters=16),
    "(ii) 8 x 66..512 + 56 x 1, 3 adapters": dict(lens=PROMPTS + [1] * 56, n_adapters=3),
}
KINDS = ("multi", "plain", "masked", "groups")


def worker(tree, layers, kind):
    sys.path.insert(0, tree)
    import torch
    from rwkv_lm_ext_amd import infctx, train_dp
    assert os.path.abspath(infctx.__file__).startswith(os.path.abspath(tree) + os.sep), infctx.__file__
    bf = torch.bfloat16
    torch.manual_seed(0)
    with torch.device("cuda"):
        blocks = [train_dp.Block(C, C, DIM_FFN, i) for i in range(layers)]
    for b in blocks:
        for p in b.parameters():
            torch.nn.init.normal_(p, 0.0, 0.02)
        b.to(bf).requires_grad_(False)
    targets = ("att.key", "att.value", "att.receptance", "ffn.key", "ffn.value", "ffn.receptance")
    if kind == "groups":
        for b in blocks:
            train_dp.inject_lora(b, targets=targets, r=RANK, alpha=32.0)
            for m in b.modules():
                if isinstance(m, train_dp.LoraLinear):
                    torch.nn.init.normal_(m.lora_B, 0.0, 0.02)
    i32 = lambda v: torch.tensor(list(v), dtype=torch.int32, device="cuda")
    state, pool = {}, {"size": None}

    def setup(case):
        state.clear()
        torch.cuda.empty_cache()
        lens, n_ad = CASES[case]["lens"], CASES[case]["n_adapters"]
        n, total = len(lens), sum(lens)
        cu = [0]
        for m in lens:
            cu.append(cu[-1] + m)
        ad = [s % n_ad for s in range(n)]
        x = torch.randn(1, total, C, device="cuda").to(bf)
        pools = infctx.PackedPools(torch.zeros(layers, N_SLOTS, C, device="cuda", dtype=bf), torch.zeros(layers, N_SLOTS, C, device="cuda", dtype=bf),
                                   torch.zeros(layers, N_SLOTS, H, 64, 64, device="cuda"))
        state.update(x=x, cu=i32(cu), max_seqlen=max(lens), slots=i32(range(n)), pools=pools, graphs={})
        if kind in ("multi", "masked"):
            from rwkv_lm_ext_amd import adapters
            if pool["size"] != n_ad:
                for name, m in adapters.adapter_layers(blocks):            # a pool of another size: back to the base linears first
                    parent = blocks[int(name.split(".")[0])].get_submodule(".".join(name.split(".")[1:-1]))
                    lin = torch.nn.Linear(m.in_features, m.out_features, bias=False, device="cuda", dtype=bf)
                    lin.weight = m.weight
                    setattr(parent, name.split(".")[-1], lin)
                adapters.inject_adapters(blocks, n_ad, RANK)
                pool["size"] = n_ad
                for _, m in adapters.adapter_layers(blocks):
                    m.kernels = kind == "multi"
                    for a in range(n_ad):
                        m.set_weights(a, torch.randn(RANK, m.in_features, device="cuda") * 0.02, torch.randn(m.out_features, RANK, device="cuda") * 0.02, 32.0)
            state["adapter"] = i32(ad)
            adapters.set_adapters(blocks, state["cu"], state["adapter"])
        if kind == "groups":                                                # the rows, boundaries and slots of every adapter's group
            groups = []
            for a in range(n_ad):
                seqs = [s for s in range(n) if ad[s] == a]
                rows = [t for s in seqs for t in range(cu[s], cu[s + 1])]
                gcu = [0]
                for s in seqs:
                    gcu.append(gcu[-1] + lens[s])
                groups.append((x[:, rows].contiguous(), i32(gcu), max(lens[s] for s in seqs), i32(seqs)))
            state["groups"] = groups

    def run():
        s = state
        if kind == "groups":
            return [infctx.step_packed(blocks, gx, gcu, gmax, s["pools"], gslots) for gx, gcu, gmax, gslots in s["groups"]]
        return infctx.step_packed(blocks, s["x"], s["cu"], s["max_seqlen"], s["pools"], s["slots"])

    def contender(graph):
        if not graph:
            return run
        if "g" not in state["graphs"]:
            state["graphs"]["g"] = timing.graphed(run)                       # (the replay, and the output it writes)
        return state["graphs"]["g"][0]

    def accuracy():
        sys.path.insert(0, os.path.join(tree, "tests"))
        import lora_common as lc
        from rwkv_lm_ext_amd import mix_op
        out = []
        for K, N, R in lc.SHAPES:
            for total_T in lc.TOTALS:
                x, y0, A, B, scale = (t.cuda() for t in lc.case(K, N, R, total_T))
                y = mix_op.lora_packed(x, y0.clone(), A, B, scale, i32(lc.ADAPTERS), i32(lc.cu_of()))
                torch.cuda.synchronize()
                out.append([K, N, R, total_T, lc.worst_ratio(y.cpu(), *lc.reference(K, N, R, total_T))])
        return out

    ops = {
        "setup": setup,
        "warm": lambda graph, seconds: timing.warm(contender(graph), seconds=seconds, sync="each"),
        "time": lambda graph, iters: {"us": timing.event_time(contender(graph), iters) * 1e3},
        "accuracy": lambda: {"rows": accuracy()},
    }
    with torch.no_grad():
        timing.serve({"ready": True, **timing.device_record()}, ops)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--layers", type=int, default=LAYERS)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warm", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, choices=KINDS)
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.tree), a.layers, a.worker)
    log = timing.Log()
    say = log.say
    group_tree = os.path.abspath(a.parent_tree) if a.parent_tree else ROOT
    kids = {}
    for k in KINDS:
        tree = group_tree if k == "groups" else ROOT
        kids[k] = timing.Child([os.path.abspath(__file__), "--worker", k, "--tree", tree, "--layers", str(a.layers)], cwd=tree)
    try:
        say(timing.device_header(kids["multi"].hello))
        say(f"infctx.step_packed, bf16, C={C}, H={H}, dim_ffn={DIM_FFN}, {a.layers} layers, {N_SLOTS} slots, LoRA r={RANK} on the six targets; "
            f"{a.iters} calls per timing, {a.repeats} alternated rounds, {a.warm:.1f} s warm-up each; us per step: median [min, max]")
        say("multi: per-sequence adapters through the HIP kernels (this tree).  plain: no adapter (this tree).  masked: the eager masked loop "
            "(this tree, kernels=False).")
        say("groups: one step_packed per adapter group under train_dp.inject_lora, " +
            ("from the parent commit's tree, in a process of its own." if a.parent_tree else
             "NO PARENT TREE GIVEN -- the same code from this tree, in a process of its own."))
        say()
        for case in CASES:
            for k in kids.values():
                k.ask(op="setup", case=case)
            say(case)
            for graph in (True, False):
                for kid in kids.values():
                    kid.ask(op="warm", graph=graph, seconds=a.warm)
                res = timing.alternate(kids, lambda kid: kid.ask(op="time", graph=graph, iters=a.iters)["us"], a.repeats)
                m = {k: timing.median(v) for k, v in res.items()}
                mode = "graph" if graph else "eager"
                for k in KINDS:
                    say(f"  {mode:5s} {k:6s} {m[k]:10.1f} [{min(res[k]):10.1f}, {max(res[k]):10.1f}]" +
                        ("" if k == "multi" else f"   multi / {k} = {m['multi'] / m[k]:.3f}"))
                say(f"  {mode:5s} the adapters add {m['multi'] - m['plain']:.1f} us to the plain step ({(m['multi'] / m['plain'] - 1) * 100:.1f} %)")
            say()
        say("accuracy of mix_op.lora_packed on the GPU tests' inputs: max |out - E| / bound against the fp64 restatement (tests/lora_common.py)")
        for K, N, R, total_T, ratio in kids["multi"].ask(op="accuracy")["rows"]:
            say(f"  K={K} N={N} R={R} total_T={total_T}: {ratio:.3f}")
    finally:
        for k in kids.values():
            k.close()
    log.write(a.out)


if __name__ == "__main__":
    main()
